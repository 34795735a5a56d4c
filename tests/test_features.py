"""Feature buffers on the CPU: hand-worked cases of the reference fold (tests/features_ref.py), what the
oracle's G-buffer of the test streams looks like, and the binding of pt_set_feature_targets (no device call)."""
import types

import numpy as np
import pytest

import features_ref as FR
import helpers as H

F32 = np.float32


def _frames(name, still):
    """The recorded frames of a stream plus `still` still-camera frames (StreamPlayer.synth_frame)."""
    import babylon_pt as bp
    meta = H.stream(name)
    stub = types.SimpleNamespace(meta=meta)
    return meta, meta["frames"] + [bp.StreamPlayer.synth_frame(stub, k) for k in range(still)]


def _g(nrm=(0.0, 0.0, 0.0), col=(0.0, 0.0, 0.0), oid=0.0):
    g = np.zeros((1, 1, 11), F32)
    g[0, 0, 0:3], g[0, 0, 3:6], g[0, 0, 6] = nrm, col, oid
    return g


def _weights(frames, n):
    zero = np.zeros((1, 1, 4), F32)
    nid, alb, out = zero, zero, []
    for f in frames[:n]:
        nid, alb = FR.fold(nid, alb, _g(col=(1.0, 1.0, 1.0)), *FR.frame_state(f))
        out.append(float(alb[0, 0, 3]))
    return out, alb


def test_teapot_stream_takes_the_half_branch():
    """gltf_teapot_320x180 starts at uFrameCounter 2 with the camera moving: weights 0.5, 1.5, 2.5."""
    _, frames = _frames("gltf_teapot_320x180", 4)
    assert FR.frame_state(frames[0]) == (2.0, True)
    assert [FR.frame_state(f)[1] for f in frames[1:]] == [False] * (len(frames) - 1)   # ... then still frames
    w, alb = _weights(frames, 3)
    assert w == [0.5, 1.5, 2.5]
    assert alb[0, 0, :3].tolist() == [2.5, 2.5, 2.5]   # xyz / w = the mean colour 1


@pytest.mark.parametrize("name", ["cornell_256", "sky_256", "quadric_256", "hdri_helmet_320x180", "gltf_duck_320x180"])
def test_frame_one_stream_resets(name):
    """The other streams start at frame 1 (the reset branch) and go on still: weights 1, 2, 3."""
    meta, frames = _frames(name, 4)
    assert FR.frame_state(frames[0]) == (1.0, True)
    assert [FR.frame_state(f)[1] for f in frames[1:]] == [False] * (len(frames) - 1)
    w, _ = _weights(frames, 3)
    assert w == [1.0, 2.0, 3.0]


def test_reset_discards_any_history():
    old = np.full((1, 1, 4), np.nan, F32)
    nid, alb = FR.fold(old, old, _g(nrm=(0.25, -0.5, 1.0), col=(0.1, 0.2, 0.3), oid=7.0), 1.0, True)
    assert nid[0, 0].tolist() == [0.25, -0.5, 1.0, 7.0]
    assert FR.same_bits(alb[0, 0], np.array([0.1, 0.2, 0.3, 1.0], F32))


def test_negative_zero_sample_at_frame_one_lands_as_positive_zero():
    zero = np.zeros((1, 1, 4), F32)
    nid, alb = FR.fold(zero, zero, _g(nrm=(-0.0, 0.0, -0.0), col=(-0.0, -0.0, -0.0)), 1.0, False)
    assert not np.signbit(nid[0, 0, :3]).any() and not np.signbit(alb[0, 0, :3]).any()
    # ... whereas a later still frame keeps IEEE's -0 + -0 = -0
    neg = np.full((1, 1, 4), -0.0, F32)
    nid, _ = FR.fold(neg, neg, _g(nrm=(-0.0, -0.0, -0.0)), 5.0, False)
    assert np.signbit(nid[0, 0, :3]).all()


def test_moving_frame_halves_history_and_sample():
    old = np.array([[[2.0, 4.0, 8.0, 3.0]]], F32)
    nid, alb = FR.fold(old, old, _g(nrm=(1.0, 1.0, 1.0), col=(0.5, 0.5, 0.5), oid=2.0), 9.0, True)
    assert nid[0, 0].tolist() == [1.5, 2.5, 4.5, 2.0]
    assert alb[0, 0].tolist() == [1.25, 2.25, 4.25, 2.0]


def test_normal_id_w_is_the_last_draws_id():
    _, frames = _frames("cornell_256", 2)
    g = [_g(oid=3.0), _g(oid=11.0), _g(oid=5.0)]
    (nid, _), kept = FR.accumulate(frames, g, [0, 1, 2], keep={1})
    assert nid[0, 0, 3] == 5.0 and kept[1][0][0, 0, 3] == 11.0


@pytest.mark.parametrize("name,W,Hh", [("cornell_256", 48, 32), ("gltf_teapot_320x180", 96, 64),
                                        ("hdri_helmet_320x180", 96, 64), ("sky_256", 48, 32),
                                        ("quadric_256", 48, 32), ("gltf_duck_320x180", 33, 17)])
def test_oracle_gbuffer_of_the_test_streams(name, W, Hh):
    """What the GPU tests fold: no NaN, at least 6 distinct ids, a normal on a third to all of the pixels (the
    sky page's frames, the emptiest: 33.2 to 33.9 %)."""
    meta, frames = _frames(name, 1)
    maps = H.synthetic_pbr_maps(256) if name == "hdri_helmet_320x180" else None
    gb = FR.gbuffers("cpu-" + name, meta, frames, W, Hh, maps=maps)
    for g in gb:
        assert g.shape == (Hh, W, 11) and not np.isnan(g[..., :7]).any()
    ids = np.unique(np.concatenate([g[..., 6].ravel() for g in gb]))
    # (6 ids on the sky page to 17 on the quadric page; the megakernel keeps objectID in five bits)
    assert len(ids) >= 6 and ids.min() >= 0 and ids.max() < 32 and np.all(ids == np.floor(ids)), ids
    lit = np.mean([(g[..., 0:3] != 0).any(-1).mean() for g in gb])
    assert 0.33 <= lit <= 1.0, lit
    (nid, alb), _ = FR.accumulate(frames, gb, range(len(frames)))
    assert np.all(alb[..., 3] == alb[0, 0, 3]) and alb[0, 0, 3] > 0   # one weight for the whole frame
    assert FR.same_bits(nid[..., 3], gb[-1][..., 6])


def test_binding_declares_the_entry_point():
    import babylon_pt as bp
    assert "pt_set_feature_targets" in bp.SYMBOLS
    fn = bp.lib().pt_set_feature_targets
    assert len(fn.argtypes) == 3
    assert fn(None, None, None) == -1   # PT_ERR_ARG for no effect: no device call
    assert hasattr(bp.Effect, "setFeatureTargets")

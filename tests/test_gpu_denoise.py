"""pt_denoise on the device: bit for bit (uint32) the numpy reference of tests/denoise_ref.py, fed with what the
engine itself produced - the beauty and both feature targets as read back (tests/test_gpu_features.py pins those
to the oracle). Every program, the grid's edges, the parameters' ends, non-integer weights, half-empty and empty
feature targets, the call's place in the stream's order, the hand-off to screenOutput, a wrapped dst, the
refusals, and the JavaScript host. No tolerance anywhere.

Run on an MI355X: python -m pytest tests/test_gpu_denoise.py -m gpu
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch   # loaded before libpt.so, as in tests/test_distributed.py: test_wrapped_dst needs both on one HIP runtime

import denoise_ref as DR
import helpers as H
from test_gpu_compaction import _bits_equal, _diff_report, _issue, _player

pytestmark = pytest.mark.gpu

DEFAULTS = dict(iterations=3, sigma_normal=0.5, sigma_colour=1.0, demodulate=True)


def _maps():
    return H.synthetic_pbr_maps(256)


def _targets(e, player):
    import babylon_pt as bp
    size = (player.width, player.height)
    return (bp.RenderTargetTexture("featureNormalId", size, e), bp.RenderTargetTexture("featureAlbedoWeight", size, e),
            bp.RenderTargetTexture("denoised", size, e))


def _path_effect(player, frames):
    return player.wrappers[H.path_call(frames[0])["effect"]].effect


class _Scene:
    """A fresh engine with a stream's player, feature targets bound to its path-tracing effect, and a dst."""

    def __init__(self, meta, W, Hh, still=2, mesh=None, maps=None, devices=None, bind=True):
        import babylon_pt as bp
        self.e = bp.Engine(0) if devices is None else bp.Engine(devices=devices)
        self.player = _player(self.e, meta, W, Hh, mesh, maps)
        self.frames = meta["frames"] + [self.player.synth_frame(k) for k in range(still)]
        self.nid, self.alb, self.dst = _targets(self.e, self.player)
        self.fx = _path_effect(self.player, self.frames)
        if bind:
            self.fx.setFeatureTargets(self.nid, self.alb)
        self.beauty = self.player.textures["pathTracingRenderTarget"]

    def play(self, lo=0, hi=None):
        for calls in self.frames[lo:hi]:
            _issue(self.e, self.player, calls, 1)

    def inputs(self):
        return self.beauty.read(), self.nid.read(), self.alb.read()

    def check(self, what, dst=None, **params):
        """denoise with `params`, then the result against the reference over the inputs as read back."""
        p = dict(DEFAULTS, **params)
        dst = dst or self.dst
        self.e.denoise(self.beauty, self.nid, self.alb, dst, **p)
        got = dst.read()
        ref = DR.denoise(*self.inputs(), **p)
        assert _bits_equal(ref, got), "%s %s: %s" % (what, p, _diff_report(ref, got))
        return ref

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.dispose()


# ------------------------------------------------------------------ every program, five passes

@pytest.mark.parametrize("name,W,Hh,maps", [("cornell_256", 48, 32, False), ("sky_256", 48, 32, False),
                                             ("quadric_256", 48, 32, False), ("gltf_teapot_320x180", 96, 64, False),
                                             ("hdri_helmet_320x180", 96, 64, True)])
def test_programs_five_passes(name, W, Hh, maps):
    with _Scene(H.stream(name), W, Hh, maps=_maps() if maps else None) as s:
        s.play()
        ref = s.check(name, iterations=5)
        assert np.all(ref[..., 3] == 1.0) and (ref[..., :3] > 0).any()


# ------------------------------------------------------------------ edges of the grid

@pytest.mark.parametrize("name,W,Hh,iterations", [("gltf_duck_320x180", 33, 17, 5), ("gltf_teapot_320x180", 1, 1, 5),
                                                   ("gltf_teapot_320x180", 203, 117, 3)])
def test_grid_edges(name, W, Hh, iterations):
    """33 x 17 at five passes: a last tile of one row and one column, and spacing 16 >= the height, so taps leave
    the image on every side; one pixel; 203 x 117, no multiple of a tile either way."""
    with _Scene(H.stream(name), W, Hh) as s:
        s.play()
        s.check("%dx%d" % (W, Hh), iterations=iterations)


# ------------------------------------------------------------------ the parameters' ends

def test_parameter_ends():
    with _Scene(H.stream("gltf_teapot_320x180"), 96, 64) as s:
        s.play()
        seen = set()
        for iterations in (1, 5):
            for demodulate in (False, True):
                for sn in (0.1, 4.0):
                    for sc in (0.05, 16.0):
                        ref = s.check("parameters", iterations=iterations, demodulate=demodulate, sigma_normal=sn,
                                      sigma_colour=sc)
                        seen.add(ref.tobytes())
        assert len(seen) == 16   # every combination filters differently


# ------------------------------------------------------------------ weights that are not integers

def test_moving_camera_stream():
    """The teapot stream starts at uFrameCounter 2 with the camera moving: weights 0.5, 1.5, 2.5."""
    with _Scene(H.stream("gltf_teapot_320x180"), 96, 64, still=0) as s:
        for i, w in enumerate((0.5, 1.5, 2.5)):
            s.play(i, i + 1)
            assert np.all(s.alb.read()[..., 3] == w)
            s.check("weight %g" % w, iterations=4)


# ------------------------------------------------------------------ half-empty and empty feature targets

def test_features_bound_late_then_unbound():
    with _Scene(H.stream("gltf_teapot_320x180"), 96, 64, still=4, bind=False) as s:
        s.check("never folded")
        assert _bits_equal(s.dst.read(), np.tile(np.array([0, 0, 0, 1], np.float32), (64, 96, 1)))
        s.play(0, 2)
        s.check("still never folded", iterations=5)
        assert _bits_equal(s.dst.read(), np.tile(np.array([0, 0, 0, 1], np.float32), (64, 96, 1)))
        s.fx.setFeatureTargets(s.nid, s.alb)
        s.play(2, 4)
        s.check("bound for two frames")
        s.fx.setFeatureTargets(None, None)
        s.play(4, None)
        ref = s.check("unbound again", iterations=5)
        assert (ref[..., :3] > 0).any()


# ------------------------------------------------------------------ the call's place in the order

def _order_run(monkeypatch, with_denoise, cont):
    monkeypatch.setenv("PT_OVERLAP_DEPTH", "3")
    if cont:
        monkeypatch.setenv("PT_CONT", "1")
        monkeypatch.setenv("PT_OVERLAP_LAG", "0")
    out = {}
    with _Scene(H.stream("gltf_teapot_320x180"), 96, 64, still=9) as s:
        def traced():
            if with_denoise:   # right after the path-tracing draw, nothing synchronised
                s.e.denoise(s.beauty, s.nid, s.alb, s.dst, **DEFAULTS)

        for i, calls in enumerate(s.frames):
            _issue(s.e, s.player, calls, 1, traced if i in (4, 5, 8) else None)
            if with_denoise and i == 8:   # the inputs as they were when the call ran: nothing was drawn since
                got = s.dst.read()
                # (frame 8's copy and output drew after the call; they write neither the inputs nor dst)
                ref = DR.denoise(*s.inputs(), **DEFAULTS)
                assert _bits_equal(ref, got), _diff_report(ref, got)
        out["inputs"] = s.inputs()
        out["canvas"] = s.e.read_canvas(96, 64)
        out["cont"] = s.e.cont_stats()
        out["qs"] = s.e.queue_stats()
    return out


@pytest.mark.parametrize("cont", [False, True])
def test_order_and_nothing_else_changes(monkeypatch, cont):
    """pt_denoise right after a path-tracing draw with three frames in flight, then with compaction forced as
    well, more draws behind it: the beauty, both feature targets and the last canvas have the bits they have
    without the call, and the statistics count the same."""
    a = _order_run(monkeypatch, True, cont)
    b = _order_run(monkeypatch, False, cont)
    for name, x, y in zip(("beauty", "normal_id", "albedo_weight"), a["inputs"], b["inputs"]):
        assert _bits_equal(y, x), "%s: %s" % (name, _diff_report(y, x))
    assert np.array_equal(a["canvas"], b["canvas"])
    assert a["cont"] == b["cont"] and (a["cont"][1] > 0 or not cont), (a["cont"], b["cont"])
    assert a["qs"] == b["qs"] and a["qs"]["frames_in_flight"] == 3, (a["qs"], b["qs"])


# ------------------------------------------------------------------ the hand-off to screenOutput

def test_canvas_from_dst():
    """screenOutput with dst bound as its accumulation sampler: a plain tone map of it (every flag says 'do not
    blur'), the oracle's screen_output of the reference dst byte for byte."""
    import ptoracle as po
    with _Scene(H.stream("hdri_helmet_320x180"), 96, 64, maps=_maps()) as s:
        s.play()
        ref = s.check("canvas")
        s.player.textures["denoised"] = s.dst
        out = dict(H.output_call(s.frames[-1]))
        out["samplers"] = {k: "denoised" for k in out["samplers"]}
        s.player.play_call(out)
        can = s.e.read_canvas(96, 64)
        inv = out["uniforms"]["uOneOverSampleCounter"][1][0]
        exposure = out["uniforms"]["uToneMappingExposure"][1][0]
        want = po.screen_output(ref, inv, exposure)
        assert np.array_equal(want, can), _diff_report(want, can)
        # ... and that is the tone map alone: the filter found no neighbour to blend (two texels from the border
        # it counts the zero texels outside the texture, as it does for any accumulation)
        x = ref[2:-2, 2:-2, :3] * np.float32(inv) * np.float32(exposure)
        tone = 255.0 * np.clip(x / (1 + x), 0, 1) ** 0.4545
        assert np.abs(can[2:-2, 2:-2, :3].astype(np.float64) - tone).max() <= 1.0


# ------------------------------------------------------------------ a wrapped dst

def test_wrapped_dst():
    import babylon_pt as bp
    with _Scene(H.stream("gltf_teapot_320x180"), 96, 64) as s:
        t = torch.full((64, 96, 4), -7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        wrapped = bp.RenderTargetTexture("wrapped", (96, 64), s.e, device_ptr=t.data_ptr())
        s.play()
        ref = s.check("wrapped", dst=wrapped, iterations=5)
        s.e.sync()
        assert _bits_equal(ref, t.cpu().numpy())
        wrapped.dispose()


# ------------------------------------------------------------------ refusals

def test_errors_then_a_good_call():
    import babylon_pt as bp
    L = bp.lib()
    nan, inf = float("nan"), float("inf")
    with _Scene(H.stream("gltf_teapot_320x180"), 96, 64) as s:
        s.play()
        e2 = bp.Engine(0)
        try:
            foreign = bp.RenderTargetTexture("foreign", (96, 64), e2)
            small = bp.RenderTargetTexture("small", (95, 64), s.e)
            tall = bp.RenderTargetTexture("tall", (96, 65), s.e)
            data = s.player.textures["file:BlueNoise_RGBA256.png"]
            before = s.inputs()
            good = (s.beauty, s.nid, s.alb, s.dst)

            def call(tex=good, it=3, sn=0.5, sc=1.0, dm=1, ctx=s.e.ctx):
                return L.pt_denoise(ctx, *[t.handle if t is not None else None for t in tex], it, sn, sc, dm)

            bad = [dict(ctx=None)]
            for k in range(4):
                for other in (None, foreign, data, small, tall):
                    tex = list(good)
                    tex[k] = other
                    bad.append(dict(tex=tuple(tex)))
            bad += [dict(tex=(s.beauty, s.nid, s.alb, inp)) for inp in good[:3]]
            bad += [dict(it=v) for v in (0, 6, -1, 1 << 30)]
            bad += [dict(sn=v) for v in (0.0, -0.5, inf, -inf, nan)]
            bad += [dict(sc=v) for v in (0.0, -1.0, inf, -inf, nan)]
            bad += [dict(dm=v) for v in (2, -1)]
            for kw in bad:
                assert call(**kw) == -1, kw   # PT_ERR_ARG
            with pytest.raises(bp.PtError, match="PT_ERR_ARG"):
                s.e.denoise(s.beauty, s.nid, s.alb, s.dst, iterations=6)
            assert call() == 0
            after = s.inputs()
            for x, y in zip(before, after):
                assert _bits_equal(x, y)
            s.check("after the refusals", iterations=2)
        finally:
            e2.dispose()


def test_multi_part_context_is_unsupported():
    import babylon_pt as bp
    with _Scene(H.stream("gltf_teapot_320x180"), 96, 64, still=0, devices=[0, 0]) as s:
        s.play()
        with pytest.raises(bp.PtError, match="PT_ERR_UNSUPPORTED"):
            s.e.denoise(s.beauty, s.nid, s.alb, s.dst)
        # (bad arguments are still bad arguments there)
        assert bp.lib().pt_denoise(s.e.ctx, s.beauty.handle, s.nid.handle, s.alb.handle, None, 3, 0.5, 1.0, 1) == -1


# ------------------------------------------------------------------ the JavaScript host

@pytest.mark.skipif(not shutil.which("node"), reason="node not installed")
def test_node_denoise_matches_python(tmp_path):
    """js/replay_denoise.js replays the teapot stream with feature targets and denoises through the shim and the
    addon: byte for byte the Python binding's dst, which is the reference's."""
    meta = H.stream("gltf_teapot_320x180")
    W, Hh = meta["width"], meta["height"]
    H.bluenoise().tofile(tmp_path / "bluenoise.u8")
    for k, v in H.texture_payloads(meta, H.mesh(meta)).items():
        v.tofile(tmp_path / (k + ".f32"))
    out = str(tmp_path / "out")
    script = os.path.join(H.ROOT, "babylon.js-pathtracing-renderer_amd", "js", "replay_denoise.js")
    subprocess.run(["node", script, os.path.join(H.GOLD, "gltf_teapot_320x180.json"), str(tmp_path), out],
                   check=True, timeout=300)
    js = np.fromfile(out + ".denoised.f32", np.float32).reshape(Hh, W, 4)
    with _Scene(meta, W, Hh, still=0) as s:
        for i in range(len(meta["frames"])):
            s.player.play_frame(i)
        ref = s.check("python")
    assert js.tobytes() == ref.tobytes()

"""pt_targets_encode_exr on the GPU: every comparison is bytes == tests/exr_enc_ref.py (numpy and zlib), no
tolerance. The content is put into render targets with pt_write_pixels or a wrapped torch tensor, so only the last
test renders. The images are tests/exr_enc_cases.py's, the smallest at which each stage can go wrong; what each case
reaches (pieces per block, blocks past one trip of the scan, raw fall-backs, every deflate block type) is asserted
from the reference's certificate in tests/test_exr_enc_ref.py."""
import ctypes

import numpy as np
import pytest

import helpers as H
import exr_enc_cases as C
import exr_enc_ref as R

pytestmark = pytest.mark.gpu

PT_ERR_ARG, PT_ERR_UNSUPPORTED = -1, -7
CASES = C.cases()
COMPRESSION = {R.NONE: "none", R.ZIPS: "zips", R.ZIP: "zip"}
TYPE = {R.HALF: "half", R.FLOAT: "float"}


class Targets:
    """an engine and render targets per (slot, size), filled with pt_write_pixels"""

    def __init__(self):
        import torch
        import babylon_pt as bp
        torch.cuda.init()   # (before libpt's first device call, as in tests/test_gpu_ranks.py)
        self.bp = bp
        self.engine = bp.Engine(0)
        self.rt = {}

    def put(self, tex, slot=0):
        h, w = tex.shape[:2]
        key = (slot, w, h)
        if key not in self.rt:
            self.rt[key] = self.bp.RenderTargetTexture("t%d_%dx%d" % key, (w, h), self.engine)
        self.rt[key].write(tex)
        return self.rt[key]

    def channels(self, case):
        texs, specs, _ = case
        rts = [self.put(t, k) for k, t in enumerate(texs)]
        return [(name, rts[k], comp, scale, TYPE[kind]) for name, k, comp, scale, kind in specs], rts


@pytest.fixture(scope="module")
def tg():
    t = Targets()
    yield t
    t.engine.dispose()


@pytest.fixture(scope="module")
def want():
    """the reference's file of every case, computed once"""
    return {name: R.encode(C.channels(case), case[2]) for name, case in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_bytes_are_the_references(tg, want, name):
    case = CASES[name]
    chans, rts = tg.channels(case)
    got = tg.engine.encode_targets_exr(chans, COMPRESSION[case[2]])
    assert got == want[name], (name, len(got), len(want[name]))
    assert len(got) <= R.file_max(C.channels(case), case[2])
    for rt, tex in zip(rts, case[0]):   # the targets are only read
        assert np.array_equal(rt.read().view(np.uint32), tex.view(np.uint32))


@pytest.mark.parametrize("compression", [R.NONE, R.ZIPS, R.ZIP])
def test_every_compression(tg, compression):
    for name in ("names", "scale-third", "mixed-zips", "pieces-5", "zip-3x33"):
        case = (CASES[name][0], CASES[name][1], compression)
        chans, _ = tg.channels(case)
        assert tg.engine.encode_targets_exr(chans, COMPRESSION[compression]) == R.encode(C.channels(case), compression), name


def test_one_target_by_its_own_method(tg):
    tex = C.ramp(17, 21, 2)
    rt = tg.put(tex)
    assert rt.encode_exr() == R.encode([(n, tex, k, 1.0, R.HALF) for k, n in enumerate("RGB")], R.ZIP)
    assert rt.encode_exr(("Y", "x", "a", "id"), 0.25, "float", "zips") == \
        R.encode([(n, tex, k, 0.25, R.FLOAT) for k, n in enumerate(("Y", "x", "a", "id"))], R.ZIPS)


def test_wrapped_target_and_workspace_reuse(tg, want):
    """a wrapped torch tensor among the targets; a small file after a large one; the same call twice"""
    import torch
    bp = tg.bp
    big, _ = tg.channels(CASES["pieces-5"])
    assert tg.engine.encode_targets_exr(big, "zip") == want["pieces-5"]        # (a larger workspace first)
    texs, specs, compression = CASES["names"]
    t = torch.from_numpy(texs[1]).to("cuda:0")
    torch.cuda.synchronize()
    h, w = texs[1].shape[:2]
    wrapped = bp.RenderTargetTexture("wrapped", (w, h), tg.engine, t.data_ptr())
    try:
        rts = [tg.put(texs[0]), wrapped]
        chans = [(name, rts[k], comp, scale, TYPE[kind]) for name, k, comp, scale, kind in specs]
        first = tg.engine.encode_targets_exr(chans, "zip")
        assert first == want["names"]
        assert tg.engine.encode_targets_exr(chans, "zip") == first
        assert np.array_equal(t.cpu().numpy(), texs[1])
        assert tg.engine.encode_targets_exr(big, "zip") == want["pieces-5"]
    finally:
        wrapped.dispose()


def _array(bp, chans):
    arr = (bp.ExrChannel * len(chans))()
    keep = []
    for i, (name, handle, comp, scale, kind) in enumerate(chans):
        keep.append(name)
        arr[i].name, arr[i].tex, arr[i].component, arr[i].scale, arr[i].type = name, handle, comp, scale, kind
    return arr, keep


def test_capacity_and_arguments(tg):
    bp = tg.bp
    L = bp.lib()
    tex = C.ramp(6, 9, 1)
    rt = tg.put(tex)
    good = [(b"G", rt.handle, 1, 0.5, R.HALF), (b"R", rt.handle, 0, 0.5, R.FLOAT)]
    want = R.encode([("G", tex, 1, 0.5, R.HALF), ("R", tex, 0, 0.5, R.FLOAT)], R.ZIP)
    ctx, guard = tg.engine.ctx, 64
    size = ctypes.c_size_t(0)
    arr, _keep = _array(bp, good)
    for cap in (len(want) - 1, 0, 40):
        buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
        assert L.pt_targets_encode_exr(ctx, arr, 2, R.ZIP, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
        assert size.value == len(want) and bytes(buf) == b"\xA5" * (cap + guard)
    cap = len(want)
    buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
    assert L.pt_targets_encode_exr(ctx, arr, 2, R.ZIP, buf, cap, ctypes.byref(size)) == 0
    assert size.value == cap and bytes(buf)[:cap] == want and bytes(buf)[cap:] == b"\xA5" * guard

    def refused(chans, n=None, compression=R.ZIP, dst=True, sz=True, context=ctx):
        b = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
        a, _k = _array(bp, chans) if chans else (None, None)
        rc = L.pt_targets_encode_exr(context, a, len(chans) if n is None else n, compression, b if dst else None, cap,
                                     ctypes.byref(size) if sz else None)
        return rc == PT_ERR_ARG and bytes(b) == b"\xA5" * (cap + guard)

    raw = bp.RawTexture.CreateRGBATexture(np.zeros(4 * 9 * 6, np.float32), 9, 6, tg.engine)
    other_size = tg.put(C.ramp(6, 10))
    other = bp.Engine(0)
    try:
        foreign = bp.RenderTargetTexture("foreign", (9, 6), other)
        h = rt.handle
        assert refused(good, n=0) and refused(good, n=-1) and refused(None, n=1)
        assert refused([(b"c%02d" % i, h, 0, 1.0, R.HALF) for i in range(17)])
        assert refused(good, context=None)
        assert refused([(b"R", None, 0, 1.0, R.HALF)]) and refused([(b"R", raw.handle, 0, 1.0, R.HALF)])
        assert refused([(b"R", foreign.handle, 0, 1.0, R.HALF)])
        assert refused([(b"R", h, 0, 1.0, R.HALF), (b"G", other_size.handle, 0, 1.0, R.HALF)])
        assert refused([(b"R", h, 4, 1.0, R.HALF)]) and refused([(b"R", h, -1, 1.0, R.HALF)])
        assert refused([(b"R", h, 0, 1.0, 0)]) and refused([(b"R", h, 0, 1.0, 3)])
        for compression in (-1, 1, 4, 9):
            assert refused(good, compression=compression)
        for scale in (float("inf"), float("-inf"), float("nan")):
            assert refused([(b"R", h, 0, scale, R.HALF)])
        for name in (None, b"", b"x" * 32, b"a b", b"tab\t", b"\x7f", b"\xc3\xa9"):
            assert refused([(name, h, 0, 1.0, R.HALF)]), name
        assert refused([(b"R", h, 0, 1.0, R.HALF), (b"G", h, 1, 1.0, R.HALF), (b"R", h, 2, 1.0, R.FLOAT)])
        assert refused(good, dst=False) and refused(good, sz=False)
        # what is allowed at the edges: a name of 31 bytes, 0x21 and 0x7E, a negative scale, 16 channels
        ok = [(b"!" + b"~" * 30, h, 3, -1.0, R.HALF)] + [(b"c%02d" % i, h, i % 4, 1.0, R.FLOAT) for i in range(15)]
        a, _k = _array(bp, ok)
        big = (ctypes.c_uint8 * 65536)()
        assert L.pt_targets_encode_exr(ctx, a, 16, R.ZIPS, big, 65536, ctypes.byref(size)) == 0
        assert bytes(big)[:size.value] == R.encode([(n.decode(), tex, c, s, k) for n, _h, c, s, k in ok], R.ZIPS)
    finally:
        raw.dispose()
        other.dispose()


def test_a_context_of_several_parts_is_refused():
    import babylon_pt as bp
    e = bp.Engine(devices=[0, 0])
    try:
        rt = bp.RenderTargetTexture("t", (16, 16), e)
        with pytest.raises(bp.PtError) as err:
            rt.encode_exr()
        assert err.value.code == PT_ERR_UNSUPPORTED
    finally:
        e.dispose()


def _frames(encode):
    """the Cornell stream at 48 x 32, two frames, features and moments bound; `encode` observes the scene"""
    from test_gpu_denoise_variance import _VScene
    with _VScene(H.stream("cornell_256"), 48, 32, still=0) as s:
        s.e.set_counting(True)
        s.e.reset_counters()
        s.play(0, 2)
        files = encode(s) if encode else None
        beauty, nid, alb, mom = s.inputs()
        canvas = s.e.read_canvas(s.player.width, s.player.height)
        return files, beauty, nid, alb, mom, canvas, s.e.counters()


def test_rendered_frames_with_their_feature_buffers():
    """the AOV helper's ten channels right after the draws (what is deferred runs first, as a read would): the bytes
    are the reference's over the texels read back, for each compression; the same call again returns the same file
    and moves no statistic; and the beauty, the feature buffers, the canvas and the counters are bit for bit those of
    the same frames without any encode"""
    import babylon_pt as bp

    def encode(s):
        weight = float(s.alb.read()[0, 0, 3])    # the weight albedo_weight.w holds, uniform over the frame
        chans = bp.Engine.exr_aov_channels(s.beauty, s.nid, s.alb, weight)
        assert [c[0] for c in chans] == ["R", "G", "B", "albedo.R", "albedo.G", "albedo.B", "normal.X", "normal.Y",
                                         "normal.Z", "id"]
        files = {z: s.e.encode_targets_exr(chans, z) for z in ("zip", "zips", "none")}
        before = (s.e.fuse_stats(), s.e.queue_stats(), s.e.job_stats(), s.e.cont_stats())
        assert s.e.encode_targets_exr(chans, "zip") == files["zip"]
        assert (s.e.fuse_stats(), s.e.queue_stats(), s.e.job_stats(), s.e.cont_stats()) == before
        moments = s.e.encode_targets_exr([("m1", s.mom, 0, 0.5, "float"), ("m2", s.mom, 1, 0.5, "float")], "zip")
        return files, moments

    (files, moments), beauty, nid, alb, mom, canvas, counters = _frames(encode)
    weight = float(alb[0, 0, 3])
    assert weight >= 1.0 and (alb[..., 3] == weight).all() and beauty[..., :3].any() and nid[..., 3].any()
    inv = 1.0 / weight
    ref = [(n, beauty, k, inv, R.HALF) for k, n in enumerate("RGB")]
    ref += [("albedo." + n, alb, k, inv, R.HALF) for k, n in enumerate("RGB")]
    ref += [("normal." + n, nid, k, inv, R.HALF) for k, n in enumerate("XYZ")]
    ref.append(("id", nid, 3, 1.0, R.FLOAT))
    for z, number in (("zip", R.ZIP), ("zips", R.ZIPS), ("none", R.NONE)):
        assert files[z] == R.encode(ref, number), z
    assert moments == R.encode([("m1", mom, 0, 0.5, R.FLOAT), ("m2", mom, 1, 0.5, R.FLOAT)], R.ZIP)
    got, _ = R.decode(files["zip"])
    assert np.array_equal(got["id"].view(np.float32), nid[::-1, :, 3])
    _, beauty0, nid0, alb0, mom0, canvas0, counters0 = _frames(None)
    for a, b in ((beauty, beauty0), (nid, nid0), (alb, alb0), (mom, mom0)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(canvas, canvas0) and counters == counters0

"""pt_target_encode_hdr on the GPU: every comparison is bytes == tests/hdr_enc_ref.py (numpy) over the target's rows
top-down, no tolerance. The content is put into a render target with pt_write_pixels or a wrapped torch tensor, so
only the last tests render. The images are tests/hdr_enc_cases.py's, W x H the smallest at which each stage can go
wrong; each case's certificate (the token kinds present, the longest literal, a run across a byte step of the wave, a
stretch across a step of runs, more planes than waves in flight) is asserted from the reference, so a case that
stopped reaching what it is for fails too."""
import ctypes

import numpy as np
import pytest

import helpers as H
import hdr_enc_cases as C
import hdr_enc_ref as R
import pt_assets

pytestmark = pytest.mark.gpu

PT_ERR_ARG, PT_ERR_UNSUPPORTED = -1, -7
CASES = C.cases()


class Targets:
    """an engine and one render target per size, filled with pt_write_pixels"""

    def __init__(self):
        import torch
        import babylon_pt as bp
        torch.cuda.init()   # (before libpt's first device call, as in tests/test_gpu_ranks.py)
        self.bp = bp
        self.engine = bp.Engine(0)
        self.rt = {}

    def put(self, tex):
        h, w = tex.shape[:2]
        if (w, h) not in self.rt:
            self.rt[(w, h)] = self.bp.RenderTargetTexture("t%dx%d" % (w, h), (w, h), self.engine)
        self.rt[(w, h)].write(tex)
        return self.rt[(w, h)]


@pytest.fixture(scope="module")
def tg():
    t = Targets()
    yield t
    t.engine.dispose()


@pytest.fixture(scope="module")
def want():
    """the reference's file of every case, computed once"""
    return {name: R.encode(tex, scale) for name, (tex, scale) in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_bytes_are_the_references(tg, want, name):
    tex, scale = CASES[name]
    rt = tg.put(tex)
    got = rt.encode_hdr(scale)
    assert got == want[name], (name, len(got), len(want[name]))
    assert len(got) <= R.file_max(tex.shape[1], tex.shape[0])
    assert np.array_equal(rt.read(), tex, equal_nan=True)   # the target is only read


def test_cases_reach_the_kernels_loops():
    cert = {n: R.certificate(*CASES[n]) for n in ("runs", "stretches", "straddle", "size-300x5", "size-16x600",
                                                  "size-65x2", "size-129x2", "size-1x1", "size-7x3", "size-32768x1",
                                                  "size-32767x1", "size-8x2", "size-9x1")}
    for n in ("size-1x1", "size-7x3", "size-32768x1"):
        assert cert[n]["flat"]
    for n in ("size-8x2", "size-9x1", "size-32767x1"):
        assert not cert[n]["flat"]
    assert set(C.RUN_LENGTHS) <= cert["runs"]["run_lengths"]
    for n in ("runs", "stretches"):
        assert cert[n]["kinds"] == {"run", "short", "literal"}
    assert cert["stretches"]["literal"] == 128 and {1, 127, 128} <= cert["stretches"]["literal_lengths"]
    # a plane longer than one wave step, in bytes and in runs; pieces across the steps; planes at their bound
    assert cert["size-65x2"]["byte_steps"] == 2 and cert["size-65x2"]["run_steps"] == 2
    assert cert["size-32767x1"]["byte_steps"] == 512
    assert cert["size-300x5"]["run_steps"] >= 4 and cert["size-300x5"]["at_bound"] >= 2
    assert cert["size-129x2"]["at_bound"] >= 2
    assert cert["straddle"]["run_across_byte_step"] and cert["runs"]["run_across_byte_step"]
    assert cert["straddle"]["stretch_across_run_step"] and cert["size-300x5"]["stretch_across_run_step"]
    # more scanlines than waves in flight
    assert cert["size-16x600"]["plane_loop"]
    # more texels than one trip of the conversion's grid-stride loop (every 1080p and 4K target takes several)
    for n, flat in (("grid-1100x960", False), ("grid-7x150000", True)):
        c = R.certificate(*CASES[n])
        assert c["texel_loop"] and c["flat"] == flat and 2 * R.TEXELS > CASES[n][0].shape[0] * CASES[n][0].shape[1]


def test_wrapped_target_and_workspace_reuse(tg):
    """a wrapped torch tensor as the target; a smaller target after a larger one; the same target twice"""
    import torch
    bp = tg.bp
    tex, scale = CASES["size-300x5"]
    tg.put(CASES["runs"][0]).encode_hdr()          # (a larger workspace first)
    t = torch.from_numpy(tex).to("cuda:0")
    torch.cuda.synchronize()
    rt = bp.RenderTargetTexture("wrapped", (300, 5), tg.engine, t.data_ptr())
    try:
        first = tg.engine.encode_target_hdr(rt, scale)
        assert first == R.encode(tex, scale)
        assert tg.engine.encode_target_hdr(rt, scale) == first
        assert np.array_equal(t.cpu().numpy(), tex)
    finally:
        rt.dispose()


def test_capacity_and_arguments(tg):
    bp = tg.bp
    L = bp.lib()
    tex, scale = CASES["size-63x2"]
    rt = tg.put(tex)
    want = R.encode(tex, scale)
    ctx, guard = tg.engine.ctx, 64
    size = ctypes.c_size_t(0)
    call = lambda c, t, s, buf, cap, sz: L.pt_target_encode_hdr(c, t, ctypes.c_float(s), buf, cap, sz)
    for cap in (len(want) - 1, 0, 40):
        buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
        assert call(ctx, rt.handle, scale, buf, cap, ctypes.byref(size)) == PT_ERR_ARG and size.value == len(want)
        assert bytes(buf) == b"\xA5" * (cap + guard)
    buf = (ctypes.c_uint8 * (len(want) + guard))(*([0xA5] * (len(want) + guard)))
    assert call(ctx, rt.handle, scale, buf, len(want), ctypes.byref(size)) == 0
    assert size.value == len(want) and bytes(buf)[:len(want)] == want and bytes(buf)[len(want):] == b"\xA5" * guard
    cap = len(want)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(ctx, rt.handle, bad, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
    assert call(None, rt.handle, 1.0, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
    assert call(ctx, None, 1.0, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
    assert call(ctx, rt.handle, 1.0, None, cap, ctypes.byref(size)) == PT_ERR_ARG
    assert call(ctx, rt.handle, 1.0, buf, cap, None) == PT_ERR_ARG
    # not a render target; a target of another context
    raw = bp.RawTexture.CreateRGBATexture(np.zeros(4 * 63 * 2, np.float32), 63, 2, tg.engine)
    other = bp.Engine(0)
    try:
        assert call(ctx, raw.handle, 1.0, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
        foreign = bp.RenderTargetTexture("foreign", (63, 2), other)
        assert call(ctx, foreign.handle, 1.0, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
    finally:
        raw.dispose()
        other.dispose()


def test_a_context_of_several_parts_is_refused():
    import babylon_pt as bp
    e = bp.Engine(devices=[0, 0])
    try:
        rt = bp.RenderTargetTexture("t", (16, 16), e)
        with pytest.raises(bp.PtError) as err:
            rt.encode_hdr()
        assert err.value.code == PT_ERR_UNSUPPORTED
    finally:
        e.dispose()


def _cornell(engine, frames, width=96, height=64):
    import babylon_pt as bp
    meta = H.stream("cornell_256")
    player = bp.StreamPlayer(engine, meta, H.bluenoise(), None, width, height)
    engine.resize_canvas(player.width, player.height)
    for i in range(frames):
        player.play_frame(i)
    return player


def test_rendered_frames_are_observed_only():
    """the Cornell stream at 96 x 64, three frames: the draws leave a deferred screenCopy or blend, which the encoder
    runs first as tex.read() does; the file is the reference's for the accumulation at 1 / frames; the accumulation,
    the canvas, the statistics and the synchronous PNG and JPEG files are what they were before the call; and the
    file's decode uploads as an HDRI environment of that size"""
    import babylon_pt as bp
    e = bp.Engine(0)
    try:
        frames = 3
        player = _cornell(e, frames)
        acc = player.textures["pathTracingRenderTarget"]
        data = acc.encode_hdr(1.0 / frames)            # (runs what was deferred, as read would)
        tex = acc.read()
        assert tex[..., :3].any()
        assert data == R.encode(tex, 1.0 / frames)
        copy = player.textures["screenCopyRenderTarget"]
        assert copy.encode_hdr(0.5) == R.encode(copy.read(), 0.5)
        canvas = e.read_canvas(player.width, player.height)
        png, jpg = e.encode_canvas_png(), e.encode_canvas_jpeg(90)
        before = (e.fuse_stats(), e.queue_stats(), e.job_stats(), e.cont_stats())
        assert acc.encode_hdr(1.0 / frames) == data
        assert (e.fuse_stats(), e.queue_stats(), e.job_stats(), e.cont_stats()) == before
        assert np.array_equal(acc.read(), tex)
        assert np.array_equal(e.read_canvas(player.width, player.height), canvas)
        assert e.encode_canvas_png() == png and e.encode_canvas_jpeg(90) == jpg
        env = pt_assets.decode_hdr(data)
        assert env.shape == (player.height, player.width, 4)
        assert np.array_equal(env[..., :3].astype(np.float64), R.decoded(R.scanlines(tex, 1.0 / frames)))
        hdri = bp.RawTexture.CreateRGBATexture(env, player.width, player.height, e, invertY=True,
                                               samplingMode=bp.TRILINEAR, name="hdr")
        hdri.dispose()
    finally:
        e.dispose()


def test_deferred_work_is_run_first():
    """right after a frame's draws, with nothing else observed in between, the file is the reference applied to what
    read() returns afterwards"""
    import babylon_pt as bp
    e = bp.Engine(0)
    try:
        player = _cornell(e, 2)
        for name in ("screenCopyRenderTarget", "pathTracingRenderTarget"):
            player.play_frame(1)
            t = player.textures[name]
            data = t.encode_hdr()
            assert data == R.encode(t.read())
    finally:
        e.dispose()

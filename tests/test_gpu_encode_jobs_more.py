"""The PNG and HDR encode jobs on the GPU (pt_canvas_encode_png_begin, pt_target_encode_hdr_begin) beside the JPEG and
read jobs of tests/test_gpu_encode_jobs.py: a job's bytes are what the synchronous call returns at the moment of
begin, so every comparison is bytes == tests/png_enc_ref.py, tests/hdr_enc_ref.py, tests/jpeg_enc_ref.py or the
canvas's texels, no tolerance. Canvas content comes from a wrapped torch tensor, target content from
pt_write_pixels; only the last test renders."""
import ctypes

import numpy as np
import pytest

import helpers as H
import hdr_enc_cases as C
import hdr_enc_ref as R
import jpeg_enc_ref as J
import png_enc_ref as P

pytestmark = pytest.mark.gpu

PT_ERR_ARG, PT_ERR_STATE, PT_ERR_UNSUPPORTED = -1, -4, -7


def canvas_px(w, h, seed=0):
    return np.random.default_rng(w * 1009 + h * 31 + seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


class Rig:
    """an engine whose canvas is a torch tensor the test fills, and render targets filled with pt_write_pixels"""

    def __init__(self):
        import torch
        import babylon_pt as bp
        torch.cuda.init()   # (before libpt's first device call, as in tests/test_gpu_ranks.py)
        self.bp = bp
        self.engine = bp.Engine(0)
        self.tensors = []   # (a wrapped canvas stays alive until its jobs are done)

    def canvas(self, px):
        import torch
        h, w = px.shape[:2]
        t = torch.from_numpy(np.ascontiguousarray(px)).to("cuda:0")
        torch.cuda.synchronize()
        self.tensors.append(t)
        self.engine.canvas_wrap(w, h, t.data_ptr())

    def target(self, tex, name="t"):
        h, w = tex.shape[:2]
        rt = self.bp.RenderTargetTexture(name, (w, h), self.engine)
        rt.write(tex)
        return rt


@pytest.fixture
def rig():
    r = Rig()
    yield r
    r.engine.dispose()


@pytest.mark.parametrize("size", [(1, 1), (17, 9), (100, 100)], ids=lambda s: "%dx%d" % s)
def test_png_job_bytes(rig, size):
    px = canvas_px(*size)
    rig.canvas(px)
    for colour, filt in (("rgb", "adaptive"), ("rgba", "none"), ("rgba", "paeth")):
        want = P.encode(px[::-1], P.RGBA if colour == "rgba" else P.RGB, rig.bp.Engine.PNG_FILTERS[filt])
        assert rig.engine.encode_canvas_png_begin(colour, filt).result() == want
        assert rig.engine.encode_canvas_png(colour, filt) == want


@pytest.mark.parametrize("name", ["size-1x1", "size-7x3", "size-9x1", "size-129x2", "size-300x5", "size-16x600",
                                  "stretches", "specials-third"])
def test_hdr_job_bytes(rig, name):
    tex, scale = C.cases()[name]
    rt = rig.target(tex)
    want = R.encode(tex, scale)
    assert rig.engine.encode_target_hdr_begin(rt, scale).result() == want
    assert rt.encode_hdr(scale) == want


def test_the_state_as_of_begin(rig):
    """canvas A, PNG begin, canvas B on the same stream; target A, HDR begin, pt_write_pixels of B: the jobs' files
    are A's"""
    import torch
    e = rig.engine
    w, h = 24, 80
    a, b = canvas_px(w, h, 1), canvas_px(w, h, 2)
    stream = torch.cuda.Stream()
    ta, tb = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
    canvas = torch.zeros_like(ta)
    torch.cuda.synchronize()
    ha, hb = C.sized(131, 2, seed=3), C.sized(131, 2, seed=4)
    e.set_stream(stream.cuda_stream)
    e.canvas_wrap(w, h, canvas.data_ptr())
    try:
        rt = rig.target(ha)
        with torch.cuda.stream(stream):
            canvas.copy_(ta)
            j1 = e.encode_canvas_png_begin("rgba", "sub")
            canvas.copy_(tb)
            j2 = e.encode_canvas_png_begin("rgba", "sub")
            j3 = e.encode_target_hdr_begin(rt, 0.5)
            rt.write(hb)
            j4 = e.encode_target_hdr_begin(rt, 0.5)
        assert j4.result() == R.encode(hb, 0.5)
        assert j2.result() == P.encode(b[::-1], P.RGBA, P.SUB)
        assert j3.result() == R.encode(ha, 0.5)
        assert j1.result() == P.encode(a[::-1], P.RGBA, P.SUB)
    finally:
        e.set_stream(None)


def test_four_mixed_jobs_in_reverse_order(rig):
    bp, e = rig.bp, rig.engine
    px = canvas_px(24, 80, 5)
    rig.canvas(px)
    tex, scale = C.cases()["size-258x2"]
    rt = rig.target(tex)
    jobs = [e.encode_canvas_jpeg_begin(90, 0, False), e.encode_canvas_png_begin("rgb", "up"),
            e.encode_target_hdr_begin(rt, scale), e.read_canvas_begin()]
    want = [J.encode(np.ascontiguousarray(px[::-1, :, :3]), 90), P.encode(px[::-1], P.RGB, P.UP), R.encode(tex, scale),
            px.tobytes()]
    assert bp.JOBS_MAX == 4 and e.job_stats() == (4, 0, 0, 0)
    for begin in (lambda: e.encode_canvas_png_begin(), lambda: e.encode_target_hdr_begin(rt, scale)):
        with pytest.raises(bp.PtError) as err:
            begin()
        assert err.value.code == PT_ERR_STATE
    assert e.job_stats() == (4, 0, 0, 0)
    # too small a capacity at finish: the length, an untouched buffer, and the job stays valid
    L = bp.lib()
    for j, w in ((jobs[2], want[2]), (jobs[1], want[1])):
        cap, guard = len(w) - 1, 32
        buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
        size = ctypes.c_size_t(0)
        assert L.pt_job_finish(j.handle, buf, cap, ctypes.byref(size)) == PT_ERR_ARG and size.value == len(w)
        assert bytes(buf) == b"\xA5" * (cap + guard)
    for j, w in reversed(list(zip(jobs, want))):
        assert j.result() == w
    assert e.job_stats()[0] == 4 and e.job_stats()[1] == 4 and e.job_stats()[3] == 0
    # cancel gives the slot back
    j = e.encode_target_hdr_begin(rt, scale)
    k = e.encode_canvas_png_begin()
    j.cancel()
    k.cancel()
    begun, finished, slow, cancelled = e.job_stats()
    assert (begun, finished, cancelled) == (6, 4, 2) and slow <= finished
    assert e.encode_target_hdr_begin(rt, scale).result() == want[2]
    assert e.job_stats()[:2] == (7, 5)


def test_a_slot_serves_every_kind(rig):
    """slot 0 in turn: a JPEG job, a PNG job at the same canvas size, an HDR job of a target whose bound is past
    both (the slot's buffer grows), a JPEG job again; and a file past the first pinned buffer's 64 KiB takes the
    slow copy once"""
    e = rig.engine
    px = canvas_px(40, 24, 7)
    rig.canvas(px)
    rgb = np.ascontiguousarray(px[::-1, :, :3])
    assert e.encode_canvas_jpeg_begin(75, 0, False).result() == J.encode(rgb, 75)
    assert e.encode_canvas_png_begin("rgba", "none").result() == P.encode(px[::-1], P.RGBA, P.NONE)
    # the bounds that size the slot's device buffer (pt_plan.h): the JPEG stream of 40 x 24 at 4:4:4 is 3 MCU rows of
    # 5 x 3 blocks of 224 B, doubled for stuffing, + 2 each = 20,166 B; the PNG's IDATs 24 x (1 + 4 x 40) + 24 =
    # 3,888 B, below it, so a PNG job after a JPEG job at one canvas size never grows the slot; the HDR scanlines of
    # 300 x 64 are 64 x (4 + 4 x (300 + 3)) = 77,824 B, past both: that job grows it
    jpeg_bound, png_bound = 3 * (2 * 5 * 3 * 224 + 2), 24 * (1 + 4 * 40) + 24
    hdr_bound = R.file_max(300, 64) - len(R.header(300, 64))
    assert (jpeg_bound, png_bound, hdr_bound) == (20166, 3888, 77824) and png_bound < jpeg_bound < hdr_bound
    tex = C.lognormal(300, 64, seed=9)
    assert len(R.encode(tex)) - len(R.header(300, 64)) > 65536   # the scanlines are past the first pinned buffer
    rt = rig.target(tex)
    slow0 = e.job_stats()[2]
    assert e.encode_target_hdr_begin(rt, 1.0).result() == R.encode(tex)
    assert e.job_stats()[2] == slow0 + 1
    assert e.encode_target_hdr_begin(rt, 1.0).result() == R.encode(tex)
    assert e.job_stats()[2] == slow0 + 1
    assert e.encode_canvas_jpeg_begin(75, 0, False).result() == J.encode(rgb, 75)
    assert e.encode_canvas_png_begin("rgb", "adaptive").result() == P.encode(px[::-1], P.RGB, P.ADAPTIVE)


def test_refusals(rig):
    bp, e = rig.bp, rig.engine
    L = bp.lib()
    job = ctypes.c_void_p(1)
    # no canvas yet; colour and filter out of range
    assert L.pt_canvas_encode_png_begin(e.ctx, 0, 5, ctypes.byref(job)) == PT_ERR_ARG and not job.value
    rig.canvas(canvas_px(17, 9))
    for colour, filt in ((-1, 0), (2, 0), (0, -1), (0, 6)):
        job = ctypes.c_void_p(1)
        assert L.pt_canvas_encode_png_begin(e.ctx, colour, filt, ctypes.byref(job)) == PT_ERR_ARG and not job.value
    assert L.pt_canvas_encode_png_begin(e.ctx, 0, 5, None) == PT_ERR_ARG
    rt = rig.target(C.sized(9, 1))
    raw = bp.RawTexture.CreateRGBATexture(np.zeros(36, np.float32), 9, 1, e)
    for tex, scale in ((None, 1.0), (raw.handle, 1.0), (rt.handle, 0.0), (rt.handle, float("nan")), (rt.handle, float("inf"))):
        job = ctypes.c_void_p(1)
        rc = L.pt_target_encode_hdr_begin(e.ctx, tex, ctypes.c_float(scale), ctypes.byref(job))
        assert rc == PT_ERR_ARG and not job.value
    assert L.pt_target_encode_hdr_begin(e.ctx, rt.handle, ctypes.c_float(1.0), None) == PT_ERR_ARG
    assert e.job_stats() == (0, 0, 0, 0)
    parts = bp.Engine(devices=[0, 0])
    try:
        prt = bp.RenderTargetTexture("t", (16, 16), parts)
        for begin in (lambda: parts.encode_target_hdr_begin(prt), lambda: parts.encode_canvas_png_begin()):
            with pytest.raises(bp.PtError) as err:
                begin()
            assert err.value.code == PT_ERR_UNSUPPORTED
    finally:
        parts.dispose()


def test_resize_and_destroy_wait_for_the_jobs_on_a_target(rig):
    e = rig.engine
    tex = C.sized(300, 40, seed=11)
    want = R.encode(tex, 0.25)
    rt = rig.target(tex)
    j = e.encode_target_hdr_begin(rt, 0.25)
    rt.resize((64, 8))
    assert j.result() == want
    assert rt.encode_hdr() == R.encode(np.zeros((8, 64, 4), np.float32))
    rt.write(C.sized(64, 8, seed=12))
    j = e.encode_target_hdr_begin(rt, 2.0)
    rt.dispose()
    assert j.result() == R.encode(C.sized(64, 8, seed=12), 2.0)


def test_jobs_behind_rendered_frames():
    """the Cornell stream at 96 x 64: the jobs begun after frame 2 return frame 2's files although frames 3 and 4
    and a pt_write_pixels to the target are queued before finish; the HDR job enqueues what was deferred"""
    import babylon_pt as bp
    e = bp.Engine(0)
    try:
        meta = H.stream("cornell_256")
        player = bp.StreamPlayer(e, meta, H.bluenoise(), None, 96, 64)
        e.resize_canvas(96, 64)
        player.play_frame(0)
        player.play_frame(1)
        acc = player.textures["pathTracingRenderTarget"]
        png = e.encode_canvas_png_begin("rgb", "adaptive")      # (first: it runs nothing deferred)
        hdr = e.encode_target_hdr_begin(acc, 0.5)
        want_hdr, want_png = acc.encode_hdr(0.5), e.encode_canvas_png("rgb", "adaptive")
        assert want_hdr == R.encode(acc.read(), 0.5)
        player.play_frame(2)
        player.play_frame(3)
        acc.write(np.zeros((64, 96, 4), np.float32))
        assert hdr.result() == want_hdr
        assert png.result() == want_png
    finally:
        e.dispose()

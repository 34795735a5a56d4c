"""The EXR encode job on the GPU (pt_targets_encode_exr_begin) beside the JPEG, PNG, HDR and read jobs: a job's bytes
are what the synchronous call returns at the moment of begin, so every comparison is bytes == tests/exr_enc_ref.py
(or the other encoders' references), no tolerance. Target content comes from pt_write_pixels; only the last test
renders."""
import ctypes

import numpy as np
import pytest

import helpers as H
import exr_enc_cases as C
import exr_enc_ref as R
import hdr_enc_ref as HR
import jpeg_enc_ref as J
import png_enc_ref as P
from test_gpu_encode_jobs_more import Rig, canvas_px

pytestmark = pytest.mark.gpu

PT_ERR_ARG, PT_ERR_STATE, PT_ERR_UNSUPPORTED = -1, -4, -7
CASES = C.cases()
COMPRESSION = {R.NONE: "none", R.ZIPS: "zips", R.ZIP: "zip"}
TYPE = {R.HALF: "half", R.FLOAT: "float"}


@pytest.fixture
def rig():
    r = Rig()
    yield r
    r.engine.dispose()


def bound(rig, case):
    rts = [rig.target(t, "t%d" % k) for k, t in enumerate(case[0])]
    return [(name, rts[k], comp, scale, TYPE[kind]) for name, k, comp, scale, kind in case[1]], rts


def rgb(rt, scale=1.0, kind="half"):
    return [(n, rt, k, scale, kind) for k, n in enumerate("RGB")]


def rgb_ref(tex, scale=1.0, kind=R.HALF):
    return [(n, tex, k, scale, kind) for k, n in enumerate("RGB")]


@pytest.mark.parametrize("name", ["zip-1x1", "zip-3x17", "none-3x17", "piece-511", "pieces-5", "scan-5x300", "noise-zip",
                                  "mixed-zips", "names", "chan-16", "scale-third"])
def test_job_bytes(rig, name):
    case = CASES[name]
    chans, _ = bound(rig, case)
    want = R.encode(C.channels(case), case[2])
    z = COMPRESSION[case[2]]
    assert rig.engine.encode_targets_exr_begin(chans, z).result() == want
    assert rig.engine.encode_targets_exr(chans, z) == want


def test_the_state_as_of_begin(rig):
    """target A, begin, pt_write_pixels of B on the same stream, begin: the first job's file is A's"""
    import torch
    e = rig.engine
    a, b = C.ramp(40, 131, 1), C.noise(40, 131, 6)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    try:
        rt = rig.target(a)
        with torch.cuda.stream(stream):
            j1 = e.encode_targets_exr_begin(rgb(rt, 0.5), "zip")
            rt.write(b)
            j2 = e.encode_targets_exr_begin(rgb(rt, 0.5), "zip")
        assert j2.result() == R.encode(rgb_ref(b, 0.5), R.ZIP)
        assert j1.result() == R.encode(rgb_ref(a, 0.5), R.ZIP)
    finally:
        e.set_stream(None)


def test_four_mixed_jobs_in_any_order(rig):
    bp, e = rig.bp, rig.engine
    px = canvas_px(24, 80, 5)
    rig.canvas(px)
    tex = C.ramp(20, 258, 2)
    rt = rig.target(tex)
    chans, ref = rgb(rt, 0.25) + [("A", rt, 3, 1.0, "float")], rgb_ref(tex, 0.25) + [("A", tex, 3, 1.0, R.FLOAT)]
    jobs = [e.encode_canvas_jpeg_begin(90, 0, False), e.encode_targets_exr_begin(chans, "zip"),
            e.encode_target_hdr_begin(rt, 0.5), e.encode_canvas_png_begin("rgb", "up")]
    want = [J.encode(np.ascontiguousarray(px[::-1, :, :3]), 90), R.encode(ref, R.ZIP), HR.encode(tex, 0.5),
            P.encode(px[::-1], P.RGB, P.UP)]
    assert bp.JOBS_MAX == 4 and e.job_stats() == (4, 0, 0, 0)
    with pytest.raises(bp.PtError) as err:
        e.encode_targets_exr_begin(chans, "zip")
    assert err.value.code == PT_ERR_STATE and e.job_stats() == (4, 0, 0, 0)
    # too small a capacity at finish: the length, an untouched buffer, and the job stays valid
    L = bp.lib()
    cap, guard = len(want[1]) - 1, 32
    buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
    size = ctypes.c_size_t(0)
    assert L.pt_job_finish(jobs[1].handle, buf, cap, ctypes.byref(size)) == PT_ERR_ARG and size.value == len(want[1])
    assert bytes(buf) == b"\xA5" * (cap + guard)
    for k in (2, 0, 3, 1):
        assert jobs[k].result() == want[k], k
    assert e.job_stats()[:2] == (4, 4) and e.job_stats()[3] == 0
    # cancel gives the slot back
    j = e.encode_targets_exr_begin(chans, "zips")
    j.cancel()
    begun, finished, slow, cancelled = e.job_stats()
    assert (begun, finished, cancelled) == (5, 4, 1) and slow <= finished
    assert e.encode_targets_exr_begin(chans, "zips").result() == R.encode(ref, R.ZIPS)
    assert e.job_stats()[:2] == (6, 5)


def test_a_slot_grows_to_the_exr_bound(rig):
    """slot 0 in turn: a PNG job, an EXR job whose bound is past the PNG's and whose file is past the first pinned
    buffer's 64 KiB (the slow copy, once), the same again, a PNG job again"""
    e = rig.engine
    px = canvas_px(40, 24, 7)
    rig.canvas(px)
    assert e.encode_canvas_png_begin("rgba", "none").result() == P.encode(px[::-1], P.RGBA, P.NONE)
    tex = C.noise(64, 300, 9)
    ref = [("n", tex, 0, 1.0, R.FLOAT)]
    want = R.encode(ref, R.ZIP)
    assert R.file_max(ref, R.ZIP) - 277 > 24 * (1 + 4 * 40) + 24 and len(want) - 277 > 65536
    rt = rig.target(tex)
    chans = [("n", rt, 0, 1.0, "float")]
    slow0 = e.job_stats()[2]
    assert e.encode_targets_exr_begin(chans, "zip").result() == want
    assert e.job_stats()[2] == slow0 + 1
    assert e.encode_targets_exr_begin(chans, "zip").result() == want
    assert e.job_stats()[2] == slow0 + 1
    assert e.encode_canvas_png_begin("rgb", "adaptive").result() == P.encode(px[::-1], P.RGB, P.ADAPTIVE)


def test_refusals(rig):
    bp, e = rig.bp, rig.engine
    L = bp.lib()
    rt = rig.target(C.ramp(3, 9))
    raw = bp.RawTexture.CreateRGBATexture(np.zeros(4 * 27, np.float32), 9, 3, e)
    other = rig.target(C.ramp(3, 10), "other")

    def begin(chans, n=None, compression=R.ZIP, job=True):
        arr = (bp.ExrChannel * max(len(chans), 1))()
        for i, (name, handle, comp, scale, kind) in enumerate(chans):
            arr[i].name, arr[i].tex, arr[i].component, arr[i].scale, arr[i].type = name, handle, comp, scale, kind
        j = ctypes.c_void_p(1)
        rc = L.pt_targets_encode_exr_begin(e.ctx, arr, len(chans) if n is None else n, compression,
                                           ctypes.byref(j) if job else None)
        return rc, (j.value if job else None)

    h = rt.handle
    bad = [([(b"R", h, 0, 1.0, R.HALF)], dict(n=0)), ([(b"R", h, 0, 1.0, R.HALF)] * 17, {}),
           ([(b"R", None, 0, 1.0, R.HALF)], {}), ([(b"R", raw.handle, 0, 1.0, R.HALF)], {}),
           ([(b"R", h, 0, 1.0, R.HALF), (b"G", other.handle, 0, 1.0, R.HALF)], {}),
           ([(b"R", h, 4, 1.0, R.HALF)], {}), ([(b"R", h, 0, 1.0, 3)], {}), ([(b"R", h, 0, 1.0, R.HALF)], dict(compression=1)),
           ([(b"R", h, 0, float("nan"), R.HALF)], {}), ([(b"", h, 0, 1.0, R.HALF)], {}), ([(None, h, 0, 1.0, R.HALF)], {}),
           ([(b"R", h, 0, 1.0, R.HALF), (b"R", h, 1, 1.0, R.HALF)], {})]
    for chans, kw in bad:
        rc, job = begin(chans, **kw)
        assert rc == PT_ERR_ARG and not job, (chans, kw)
    assert begin([(b"R", h, 0, 1.0, R.HALF)], job=False)[0] == PT_ERR_ARG
    assert e.job_stats() == (0, 0, 0, 0)
    parts = bp.Engine(devices=[0, 0])
    try:
        prt = bp.RenderTargetTexture("t", (16, 16), parts)
        with pytest.raises(bp.PtError) as err:
            parts.encode_targets_exr_begin(rgb(prt))
        assert err.value.code == PT_ERR_UNSUPPORTED
    finally:
        parts.dispose()


def test_resize_and_destroy_wait_for_the_jobs_on_any_named_target(rig):
    e = rig.engine
    a, b = C.ramp(40, 300, 3), C.noise(40, 300, 11)
    ra, rb = rig.target(a, "a"), rig.target(b, "b")
    chans = [("x", ra, 0, 0.25, "half"), ("y", rb, 1, 1.0, "float")]
    want = R.encode([("x", a, 0, 0.25, R.HALF), ("y", b, 1, 1.0, R.FLOAT)], R.ZIP)
    j = e.encode_targets_exr_begin(chans, "zip")
    rb.resize((64, 8))                       # (the second texture the job names)
    assert j.result() == want
    rb.resize((300, 40))
    rb.write(b)
    j = e.encode_targets_exr_begin(chans, "zip")
    rb.dispose()
    assert j.result() == want
    assert ra.encode_exr(("x",), 0.25) == R.encode([("x", a, 0, 0.25, R.HALF)], R.ZIP)


def test_a_job_behind_rendered_frames():
    """the Cornell stream at 96 x 64: the job begun after frame 2 returns frame 2's file although frames 3 and 4 and a
    pt_write_pixels to the target are queued before finish; it enqueues what was deferred"""
    import babylon_pt as bp
    e = bp.Engine(0)
    try:
        meta = H.stream("cornell_256")
        player = bp.StreamPlayer(e, meta, H.bluenoise(), None, 96, 64)
        e.resize_canvas(96, 64)
        player.play_frame(0)
        player.play_frame(1)
        acc = player.textures["pathTracingRenderTarget"]
        job = e.encode_targets_exr_begin(rgb(acc, 0.5), "zip")
        want = acc.encode_exr(("R", "G", "B"), 0.5)
        assert want == R.encode(rgb_ref(acc.read(), 0.5), R.ZIP)
        player.play_frame(2)
        player.play_frame(3)
        acc.write(np.zeros((64, 96, 4), np.float32))
        assert job.result() == want
    finally:
        e.dispose()

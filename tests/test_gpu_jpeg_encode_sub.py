"""pt_canvas_encode_jpeg_sub on the GPU, 4:2:2 and 4:2:0: every comparison is bytes == tests/jpeg_enc_sub_ref.py
(which is libjpeg-turbo's output, tests/test_jpeg_encode_sub.py) over the canvas top-down, no tolerance. The canvas
content is put there with pt_canvas_wrap over a torch uint8 device tensor, so only the last tests render. Sizes are
W x H, the smallest at which each stage can go wrong, with the dummy Y blocks each must reach (CASES). The loops that
only a frame enters (more than 256 MCU rows, the largest canvas) are tests/test_gpu_jpeg_encode_scale.py's."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import jpeg_enc_sub_ref as S

pytestmark = pytest.mark.gpu

S422, S420 = 1, 2
# (subsampling, W, H, dummy Y blocks)
CASES = [
    (S420, 1, 1, 3),         # all padding
    (S420, 8, 8, 3),         # one real Y block, dummies right and below
    (S420, 16, 16, 0),       # one full MCU, no marker
    (S420, 17, 9, 2),        # odd height, a one-column MCU
    (S420, 24, 24, 7),       # even height with padded chroma rows; a bottom dummy whose DC is a dummy's; one RST
    (S420, 24, 160, 20),     # ten MCU rows: the RST index wraps
    (S420, 2056, 16, 2),     # 774 blocks in one interval, past a 256-wide scan tile
    (S422, 1, 1, 1),         # all padding
    (S422, 8, 8, 1),         # one real Y block
    (S422, 16, 8, 0),        # one full MCU, no marker
    (S422, 17, 9, 2),        # a one-column MCU, two MCU rows
    (S422, 24, 16, 2),       # dummy right, one RST
    (S422, 24, 80, 10),      # ten MCU rows: the RST index wraps
    (S422, 2056, 8, 1),      # 516 blocks in one interval
]
QUALITIES = [1, 50, 90, 100]
PT_ERR_ARG = -1


def case_id(c):
    return "%s-%dx%d" % ({S422: "422", S420: "420"}[c[0]], c[1], c[2])


def content(kind, w, h, seed=0):
    """RGBA8 canvas rows (bottom-up, as the canvas is); the alpha is random in every case"""
    rng = np.random.default_rng(w * 1009 + h * 31 + seed)
    px = np.empty((h, w, 4), np.uint8)
    if kind == "random":
        px[..., :3] = rng.integers(0, 256, (h, w, 3))
    elif kind == "flat":
        px[..., :3] = rng.integers(0, 256, 3)
    elif kind == "extremes":
        px[..., :3] = rng.integers(0, 2, (h, w, 3)) * 255
    else:
        raise ValueError(kind)
    px[..., 3] = rng.integers(0, 256, (h, w))
    return px


def reference(canvas, q, ss):
    return S.encode_stats(np.ascontiguousarray(canvas[::-1, :, :3]), q, ss)


class Canvas:
    """an engine whose canvas is a torch tensor the test fills"""

    def __init__(self):
        import torch
        import babylon_pt as bp
        torch.cuda.init()   # (before libpt's first device call, as in tests/test_gpu_ranks.py)
        self.engine = bp.Engine(0)
        self.tensor = None

    def put(self, px):
        import torch
        h, w = px.shape[:2]
        self.tensor = torch.from_numpy(np.ascontiguousarray(px)).to("cuda:0")
        torch.cuda.synchronize()
        self.engine.canvas_wrap(w, h, self.tensor.data_ptr())

    def encode(self, q, ss):
        return self.engine.encode_canvas_jpeg(q, subsampling=ss)


@pytest.fixture(scope="module")
def cv():
    c = Canvas()
    yield c
    c.engine.dispose()


@pytest.mark.parametrize("kind", ["random", "flat"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bytes_are_the_references(cv, case, kind):
    ss, w, h, dummies = case
    px = content(kind, w, h)
    cv.put(px)
    for q in QUALITIES:
        want, stats = reference(px, q, ss)
        assert stats["dummy"] == dummies, "the case must reach the dummy blocks it is for"
        assert cv.encode(q, ss) == want, (case, kind, q)
        if q == 100 and kind == "random" and w * h >= 17 * 9:   # (smaller noise may hold no 0xFF byte)
            assert stats["stuffed"] >= 1, "the noise at quality 100 must reach the byte stuffing"
    assert 100 in QUALITIES


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_extremes_at_quality_100(cv, case):
    """the largest categories and the longest blocks: what the workspace's per-block bound is for"""
    ss, w, h, dummies = case
    px = content("extremes", w, h)
    cv.put(px)
    want, stats = reference(px, 100, ss)
    assert stats["dummy"] == dummies
    assert cv.encode(100, ss) == want


@pytest.mark.parametrize("ss", [S422, S420], ids=["422", "420"])
def test_zero_runs_past_15(cv, ss):
    yy, xx = np.mgrid[0:8, 0:8]
    tile = np.rint(128 + 100 * np.cos((2 * xx + 1) * 7 * np.pi / 16) * np.cos((2 * yy + 1) * 7 * np.pi / 16))
    px = content("flat", 48, 32)
    px[..., :3] = np.tile(tile.astype(np.uint8), (4, 6))[:, :, None]
    want, stats = reference(px, 50, ss)
    assert stats["zrl"] >= 1, "the case must reach the ZRL code"
    cv.put(px)
    assert cv.encode(50, ss) == want


def test_workspace_reuse_across_samplings(cv):
    """a smaller canvas and another sampling after a larger one (no stale bit or block of the earlier call
    survives), the same call twice, and the canvas unchanged by the calls"""
    import jpeg_enc_ref as R
    big = content("random", 24, 160, seed=1)
    cv.put(big)
    assert cv.encode(100, S420) == reference(big, 100, S420)[0]
    small = content("random", 17, 9, seed=2)
    cv.put(small)
    assert cv.encode(90, 0) == R.encode(np.ascontiguousarray(small[::-1, :, :3]), 90)
    first = cv.encode(90, S422)
    assert first == reference(small, 90, S422)[0]
    assert cv.encode(90, S422) == first
    assert np.array_equal(cv.engine.read_canvas(17, 9), small)
    assert np.array_equal(cv.tensor.cpu().numpy(), small)


def test_capacity_and_arguments(cv):
    import babylon_pt as bp
    L = bp.lib()
    px = content("random", 17, 9, seed=3)
    cv.put(px)
    want = reference(px, 90, S420)[0]
    guard = 64
    cap = len(want)
    buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
    size = ctypes.c_size_t(0)
    for ss in (-1, 3):
        assert L.pt_canvas_encode_jpeg_sub(cv.engine.ctx, 90, ss, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
        assert bytes(buf) == b"\xA5" * (cap + guard) and size.value == 0
    cap = len(want) - 1
    buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
    assert L.pt_canvas_encode_jpeg_sub(cv.engine.ctx, 90, S420, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
    assert size.value == len(want) and bytes(buf)[cap:] == b"\xA5" * guard
    cap = len(want)
    buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
    assert L.pt_canvas_encode_jpeg_sub(cv.engine.ctx, 90, S420, buf, cap, ctypes.byref(size)) == 0
    assert size.value == cap and bytes(buf)[:cap] == want and bytes(buf)[cap:] == b"\xA5" * guard


def test_444_is_pt_canvas_encode_jpeg(cv):
    import babylon_pt as bp
    import jpeg_enc_ref as R
    L = bp.lib()
    px = content("random", 24, 24, seed=4)
    cv.put(px)
    got = []
    for call in (lambda *a: L.pt_canvas_encode_jpeg(cv.engine.ctx, 75, *a),
                 lambda *a: L.pt_canvas_encode_jpeg_sub(cv.engine.ctx, 75, 0, *a)):
        buf = (ctypes.c_uint8 * 65536)()
        size = ctypes.c_size_t(0)
        assert call(buf, 65536, ctypes.byref(size)) == 0
        got.append(bytes(buf)[:size.value])
    assert got[0] == got[1] == R.encode(np.ascontiguousarray(px[::-1, :, :3]), 75)


def _teapot(engine, frames=2, width=96, height=64):
    import babylon_pt as bp
    meta = H.stream("gltf_teapot_320x180")
    player = bp.StreamPlayer(engine, meta, H.bluenoise(), H.texture_payloads(meta, H.mesh(meta)), width, height)
    engine.resize_canvas(player.width, player.height)
    for i in range(frames):
        player.play_frame(i)
    data = engine.encode_canvas_jpeg(90, subsampling=S420)
    return data, engine.read_canvas(player.width, player.height)


def test_rendered_frame_one_and_two_parts():
    """the 96x64 glTF teapot of smoke(), two frames, at 4:2:0: the encoder runs behind the deferred screenCopy and
    the screenOutput, and on a context of two parts behind the gather"""
    import babylon_pt as bp
    got = []
    for devices in (None, [0, 0]):
        e = bp.Engine(0) if devices is None else bp.Engine(devices=devices)
        try:
            data, canvas = _teapot(e)
        finally:
            e.dispose()
        assert canvas[..., :3].any()
        assert data == reference(canvas, 90, S420)[0]
        got.append(data)
    assert got[0] == got[1]


@pytest.mark.skipif(not shutil.which("node"), reason="node not installed")
def test_node_route(tmp_path):
    """js/replay_encode.js with its sixth argument: two frames of the teapot stream at its recorded size, encoded
    at 4:2:0 through the shim and the addon: the reference's bytes for the canvas it read"""
    meta = H.stream("gltf_teapot_320x180")
    W, Hh = meta["width"], meta["height"]
    H.bluenoise().tofile(tmp_path / "bluenoise.u8")
    for k, v in H.texture_payloads(meta, H.mesh(meta)).items():
        v.tofile(tmp_path / (k + ".f32"))
    out = str(tmp_path / "out")
    script = os.path.join(H.ROOT, "babylon.js-pathtracing-renderer_amd", "js", "replay_encode.js")
    subprocess.run(["node", script, os.path.join(H.GOLD, "gltf_teapot_320x180.json"), str(tmp_path), out, "2", "90", "2"],
                   check=True, timeout=300)
    js = open(out + ".jpg", "rb").read()
    canvas = np.fromfile(out + ".canvas.u8", np.uint8).reshape(Hh, W, 4)
    assert js == reference(canvas, 90, S420)[0]

"""pt_canvas_encode_jpeg_opt on the GPU with optimize = 1: every comparison is bytes == tests/jpeg_enc_opt_ref.py
(which is libjpeg-turbo's optimize_coding output, tests/test_jpeg_encode_opt.py) over the canvas top-down, no
tolerance. The canvas content is put there with pt_canvas_wrap over a torch uint8 device tensor, so only the last
tests render. Sizes are W x H, at most 256 x 256 pixels but for the one-row frames whose row has more than 256 blocks;
more than 4096 MCUs (a second pass of pt_jpeg_hist's waves) and more than 256 MCU rows are
tests/test_gpu_jpeg_encode_scale.py's."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import jpeg_enc_opt_ref as O
import jpeg_enc_sub_ref as S

pytestmark = pytest.mark.gpu

S444, S422, S420 = 0, 1, 2
SIZES = [
    (1, 1),          # all padding; at 4:2:2 and 4:2:0 dummy Y blocks
    (17, 9),         # width mod 16 = 1, height mod 16 = 9: a one-column MCU, dummies right (and below at 4:2:0)
    (24, 24),        # mod 16 = 8 on both axes: a bottom dummy whose DC is a dummy's; one RST
    (29, 45),        # mod 16 = 13 on both axes: no dummy, padded rows and columns
    (40, 23),        # width mod 16 = 8, height mod 16 = 7
    (24, 160),       # ten and more MCU rows: the RST index wraps
]
# a row of more than 256 blocks, past one tile of pt_jpeg_scan_blocks: 771 (4:4:4), 516 (4:2:2), 774 (4:2:0)
WIDE = {S444: (2056, 8), S422: (2056, 8), S420: (2056, 16)}
CASES = [(ss, w, h) for ss in (S444, S422, S420) for w, h in SIZES + [WIDE[ss]]]
QUALITIES = [1, 25, 50, 75, 90, 100]
PT_ERR_ARG = -1


def case_id(c):
    return "%s-%dx%d" % ({S444: "444", S422: "422", S420: "420"}[c[0]], c[1], c[2])


def content(kind, w, h, seed=0):
    """RGBA8 canvas rows (bottom-up, as the canvas is); the alpha is random in every case"""
    rng = np.random.default_rng(w * 1009 + h * 31 + seed)
    px = np.empty((h, w, 4), np.uint8)
    if kind == "random":
        px[..., :3] = rng.integers(0, 256, (h, w, 3))
    elif kind == "flat":        # tables of a single symbol and the reserved one
        px[..., :3] = rng.integers(0, 256, 3)
    elif kind == "graded":      # every run and size, counts from one to thousands
        px[..., :3] = O.graded_noise(w, h, seed + 5)
    else:
        raise ValueError(kind)
    px[..., 3] = rng.integers(0, 256, (h, w))
    return px


def has_dummies(ss, w, h):
    """a 16-pixel MCU axis whose last MCU holds one real Y block: size mod 16 in 1..8"""
    return (ss != S444 and w % 16 in range(1, 9)) or (ss == S420 and h % 16 in range(1, 9))


def reference(canvas, q, ss):
    return O.encode_stats(np.ascontiguousarray(canvas[::-1, :, :3]), q, ss)


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

    def encode(self, q, ss, optimize=True):
        return self.engine.encode_canvas_jpeg(q, subsampling=ss, optimize=optimize)


@pytest.fixture(scope="module")
def cv():
    c = Canvas()
    yield c
    c.engine.dispose()


@pytest.mark.parametrize("kind", ["random", "flat", "graded"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bytes_are_the_references(cv, case, kind):
    ss, w, h = case
    px = content(kind, w, h)
    cv.put(px)
    for q in QUALITIES:
        want, stats = reference(px, q, ss)
        assert cv.encode(q, ss) == want, (case, kind, q)
        assert (stats["dummy"] >= 1) == has_dummies(ss, w, h), "the case must reach the dummy blocks it is for"


@pytest.mark.parametrize("ss", [S444, S420], ids=["444", "420"])
def test_long_codes_and_stuffing(cv, ss):
    """128x144 of noise of every amplitude at quality 100: codes of 13 bits and more, and 0xFF bytes to stuff"""
    px = content("graded", 128, 144, seed=1)
    cv.put(px)
    want, stats = reference(px, 100, ss)
    bits = stats["tables"][1][0]
    assert max(i + 1 for i in range(16) if bits[i]) >= 13 and stats["stuffed"] >= 1
    assert cv.encode(100, ss) == want


def test_a_lane_of_more_than_64_bits(cv):
    """The bound the Annex K tables guaranteed and optimised ones do not: a lane's ZRLs, code and value in one
    64-bit word. The frame (jpeg_enc_opt_ref.lone_coefficient_63: a block of DC and coefficient 63 alone in graded
    noise, 256 x 256, quality 95) gives ZRL a 16-bit code and that lane three of them, 70 bits in all, computed here
    from the reference's tables; its Y AC table also passes through the length-limiting loop. The full 74 bits are
    tests/test_jpeg_enc_opt_host.py's, on the packer this kernel shares with the host."""
    rgb = O.lone_coefficient_63()
    px = content("flat", 256, 256)
    px[..., :3] = rgb[::-1]
    want, stats = reference(px, 95, S444)
    print("largest lane share: %d bits; tables limited: %d" % (stats["lane_bits"], stats["limited"]))
    assert stats["lane_bits"] > 64 and stats["limited"] >= 1
    cv.put(px)
    assert cv.encode(95, S444) == want


def test_optimize_0_is_pt_canvas_encode_jpeg_sub(cv):
    import babylon_pt as bp
    L = bp.lib()
    px = content("graded", 40, 23, seed=4)
    cv.put(px)
    for ss in (S444, S422, S420):
        got = []
        for call in (lambda *a: L.pt_canvas_encode_jpeg_sub(cv.engine.ctx, 75, ss, *a),
                     lambda *a: L.pt_canvas_encode_jpeg_opt(cv.engine.ctx, 75, ss, 0, *a)):
            buf = (ctypes.c_uint8 * 65536)()
            size = ctypes.c_size_t(0)
            assert call(buf, 65536, ctypes.byref(size)) == 0
            got.append(bytes(buf)[:size.value])
        std = S.encode(np.ascontiguousarray(px[::-1, :, :3]), 75, ss)
        assert got[0] == got[1] == std == cv.encode(75, ss, optimize=False) == cv.engine.encode_canvas_jpeg(75, ss)
        assert cv.encode(75, ss) != std


def test_calls_in_a_row_resizes_and_both_modes(cv):
    """two optimised calls on different pixels of one size (a histogram left from the first would show in the
    second's tables), a smaller and a larger canvas after it, the standard call in between (its workspace has another
    row stride), the same call twice, and the canvas unchanged by the calls"""
    a, b = content("graded", 67, 36, seed=1), content("random", 67, 36, seed=2)
    cv.put(a)
    assert cv.encode(90, S420) == reference(a, 90, S420)[0]
    cv.put(b)
    assert cv.encode(90, S420) == reference(b, 90, S420)[0]
    small = content("graded", 17, 9, seed=3)
    cv.put(small)
    first = cv.encode(50, S422)
    assert first == reference(small, 50, S422)[0]
    assert cv.encode(50, S422, optimize=False) == S.encode(np.ascontiguousarray(small[::-1, :, :3]), 50, S422)
    assert cv.encode(50, S422) == first
    big = content("graded", 131, 70, seed=4)
    cv.put(big)
    assert cv.encode(75, S444) == reference(big, 75, S444)[0]
    assert np.array_equal(cv.engine.read_canvas(131, 70), big)
    assert np.array_equal(cv.tensor.cpu().numpy(), big)


def test_capacity_and_arguments(cv):
    import babylon_pt as bp
    L = bp.lib()
    px = content("graded", 17, 9, seed=3)
    cv.put(px)
    want = reference(px, 90, S420)[0]
    guard = 64
    cap = len(want)
    buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
    size = ctypes.c_size_t(0)
    for ss, opt, q in ((S420, 2, 90), (S420, -1, 90), (3, 1, 90), (-1, 1, 90), (S420, 1, 0), (S420, 1, 101)):
        assert L.pt_canvas_encode_jpeg_opt(cv.engine.ctx, q, ss, opt, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
        assert bytes(buf) == b"\xA5" * (cap + guard) and size.value == 0
    assert L.pt_canvas_encode_jpeg_opt(cv.engine.ctx, 90, S420, 1, None, cap, ctypes.byref(size)) == PT_ERR_ARG
    assert L.pt_canvas_encode_jpeg_opt(cv.engine.ctx, 90, S420, 1, buf, cap, None) == PT_ERR_ARG
    cap = len(want) - 1
    buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
    assert L.pt_canvas_encode_jpeg_opt(cv.engine.ctx, 90, S420, 1, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
    assert size.value == len(want) and bytes(buf) == b"\xA5" * (cap + guard)
    cap = len(want)
    buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
    assert L.pt_canvas_encode_jpeg_opt(cv.engine.ctx, 90, S420, 1, buf, cap, ctypes.byref(size)) == 0
    assert size.value == cap and bytes(buf)[:cap] == want and bytes(buf)[cap:] == b"\xA5" * guard
    fresh = bp.Engine(0)
    try:   # no canvas yet
        assert L.pt_canvas_encode_jpeg_opt(fresh.ctx, 90, S420, 1, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
    finally:
        fresh.dispose()


def _teapot(engine, frames=2, width=96, height=64):
    import babylon_pt as bp
    meta = H.stream("gltf_teapot_320x180")
    player = bp.StreamPlayer(engine, meta, H.bluenoise(), H.texture_payloads(meta, H.mesh(meta)), width, height)
    engine.resize_canvas(player.width, player.height)
    for i in range(frames):
        player.play_frame(i)
    data = engine.encode_canvas_jpeg(90, subsampling=S420, optimize=True)
    return data, engine.read_canvas(player.width, player.height)


def test_rendered_frame_one_and_two_parts():
    """the 96x64 glTF teapot of smoke(), two frames, at 4:2:0: the encoder runs behind the deferred screenCopy and
    the screenOutput, and on a context of two parts (both on device 0) behind the gather"""
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
    """js/replay_encode.js with its seventh argument: two frames of the teapot stream at its recorded size, encoded
    at 4:2:0 with optimised tables through the shim and the addon: the reference's bytes for the canvas it read"""
    meta = H.stream("gltf_teapot_320x180")
    W, Hh = meta["width"], meta["height"]
    H.bluenoise().tofile(tmp_path / "bluenoise.u8")
    for k, v in H.texture_payloads(meta, H.mesh(meta)).items():
        v.tofile(tmp_path / (k + ".f32"))
    out = str(tmp_path / "out")
    script = os.path.join(H.ROOT, "babylon.js-pathtracing-renderer_amd", "js", "replay_encode.js")
    subprocess.run(["node", script, os.path.join(H.GOLD, "gltf_teapot_320x180.json"), str(tmp_path), out, "2", "90", "2", "1"],
                   check=True, timeout=300)
    js = open(out + ".jpg", "rb").read()
    canvas = np.fromfile(out + ".canvas.u8", np.uint8).reshape(Hh, W, 4)
    assert js == reference(canvas, 90, S420)[0]

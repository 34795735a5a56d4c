"""pt_canvas_encode_png on the GPU: every comparison is bytes == tests/png_enc_ref.py (numpy filters and Python's zlib)
over the canvas top-down, no tolerance. The canvas content is put there with pt_canvas_wrap over a torch uint8 device
tensor, so only the last tests render. Sizes are W x H, the smallest at which each stage can go wrong; each case's
certificate (chunk count, block types, filter types chosen, the longest code) is asserted from the reference, so a
case that stopped reaching what it is for fails too."""
import ctypes
import io

import numpy as np
import pytest

import helpers as H
import png_enc_cases as C
import png_enc_ref as P

pytestmark = pytest.mark.gpu

PT_ERR_ARG = -1
FILTERS = list(range(6))


def blocks_of(stats):
    """the deflate blocks of the file, without the empty stored block of every full flush"""
    raw = b"".join(stats["payloads"])[2:-4]
    return [b for b in P.walk_blocks(raw) if not (b["type"] == "stored" and b["out"] == 0)]


def block_types(stats):
    return [b["type"] for b in blocks_of(stats)]


def decoded(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


class Canvas:
    """an engine whose canvas is a torch tensor the test fills (rows bottom-up, as the canvas is)"""

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

    def check(self, px, colour, filt):
        """the file is the reference's and decodes to the pixels; returns the reference's statistics"""
        want, stats = P.encode_stats(px[::-1], colour, filt)
        got = self.engine.encode_canvas_png(colour, filt)
        assert got == want, (px.shape, colour, filt)
        top = px[::-1] if colour == P.RGBA else px[::-1, :, :3]
        assert np.array_equal(decoded(got), top)
        return stats


@pytest.fixture(scope="module")
def cv():
    c = Canvas()
    yield c
    c.engine.dispose()


def noise(w, h, seed=0):
    return np.random.default_rng(w * 1009 + h * 31 + seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def gradient_noise(w, h, seed=0):
    """a gradient plus small noise in the colours, random alpha"""
    rng = np.random.default_rng(seed + 5)
    yy, xx = np.mgrid[0:h, 0:w]
    px = np.empty((h, w, 4), np.uint8)
    base = np.stack([xx + yy // 2, 2 * yy + xx // 3, 255 - xx - yy // 4], -1)
    px[..., :3] = (base + rng.integers(0, 4, (h, w, 3))) % 256
    px[..., 3] = rng.integers(0, 256, (h, w))
    return px


@pytest.mark.parametrize("colour", [P.RGB, P.RGBA], ids=["rgb", "rgba"])
def test_one_pixel_every_filter(cv, colour):
    px = noise(1, 1)
    cv.put(px)
    for filt in FILTERS:
        stats = cv.check(px, colour, filt)
        assert block_types(stats) == ["fixed"]


def test_noise_is_stored_and_rows_straddle_the_chunk_edge(cv):
    px = noise(100, 100)
    cv.put(px)
    for filt in (P.NONE, P.ADAPTIVE):
        stats = cv.check(px, P.RGB, filt)
        assert block_types(stats) == ["stored"] * 2
    assert P.CHUNK % 301 != 0
    assert block_types(cv.check(px, P.RGBA, P.PAETH)) == ["stored"] * 3


@pytest.mark.parametrize("h,chunks,tail", [(1020, 1, 16320), (1021, 2, 16), (2040, 2, 16320)])
def test_the_chunk_edge(cv, h, chunks, tail):
    """5 x 1020 RGB is exactly one chunk and has no trailing empty one, 5 x 1021 a chunk and 16 bytes, 5 x 2040 two"""
    px = noise(5, h)
    cv.put(px)
    stats = cv.check(px, P.RGB, P.NONE)
    assert len(stats["payloads"]) == chunks and len(stats["stream"]) - (chunks - 1) * P.CHUNK == tail
    assert len(blocks_of(stats)) == chunks


@pytest.mark.parametrize("colour,h,left", [(P.RGB, 65, 1), (P.RGBA, 155, 0), (P.RGBA, 207, 2), (P.RGBA, 104, 3)])
def test_run_remainders(cv, colour, h, left):
    """an all-zero canvas under filter None is one run: its first literal, matches of 258, and (L - 1) mod 258 left"""
    px = np.zeros((h, 1, 4), np.uint8)
    cv.put(px)
    stats = cv.check(px, colour, P.NONE)
    n = len(stats["stream"])
    assert (n - 1) % 258 == left
    block, = blocks_of(stats)
    full = (n - 1) // 258
    assert block["matches"] == full + (1 if left >= 3 else 0)
    assert block["symbols"] == 1 + block["matches"] + (left if left < 3 else 0)


def test_flat_canvas_runs_of_a_whole_chunk(cv):
    px = np.zeros((120, 100, 4), np.uint8)
    cv.put(px)
    stats = cv.check(px, P.RGB, P.NONE)
    assert block_types(stats) == ["dynamic"] * 3
    assert [b["symbols"] for b in blocks_of(stats)[:2]] == [1 + 63 + 1] * 2   # 16,319 = 63 x 258 + 65


@pytest.mark.parametrize("w", [1, 7])
def test_ties_and_the_first_row(cv, w):
    """a flat non-zero canvas under the adaptive filter. One pixel wide, the first row ties between None, Sub and Up
    (and Average and Paeth see the same zeros), the later rows between Up and Paeth at a sum of zero; wider, Sub wins
    the first row outright and the later rows tie between Up and Paeth again. The lowest type wins each tie."""
    px = np.empty((9, w, 4), np.uint8)
    px[...] = (200, 7, 130, 99)
    cv.put(px)
    for colour in (P.RGB, P.RGBA):
        stats = cv.check(px, colour, P.ADAPTIVE)
        rows = np.ascontiguousarray(px[::-1] if colour == P.RGBA else px[::-1, :, :3]).reshape(9, -1)
        bpp = 4 if colour == P.RGBA else 3
        cost = lambda k, y: int(np.abs(P.filter_row(k, rows[y], rows[y - 1] if y else np.zeros_like(rows[0]), bpp)
                                       .view(np.int8).astype(int)).sum())
        first = [cost(k, 0) for k in range(5)]
        later = [cost(k, 1) for k in range(5)]
        assert later[P.UP] == later[P.PAETH] == 0 and min(later[P.NONE], later[P.SUB], later[P.AVERAGE]) > 0
        if w == 1:
            assert first[P.NONE] == first[P.SUB] == first[P.UP] == min(first)
            assert stats["types"] == [P.NONE] + [P.UP] * 8
        else:
            assert first[P.SUB] < min(first[P.NONE], first[P.UP])
            assert stats["types"] == [P.SUB] + [P.UP] * 8


@pytest.mark.parametrize("colour", [P.RGB, P.RGBA], ids=["rgb", "rgba"])
def test_gradient_plus_noise_adaptive(cv, colour):
    px = gradient_noise(200, 150)
    cv.put(px)
    stats = cv.check(px, colour, P.ADAPTIVE)
    assert len(set(stats["types"])) >= 3, "the adaptive choice must take at least three filter types"
    assert "dynamic" in block_types(stats) and len(stats["payloads"]) == (6 if colour == P.RGB else 8)
    for filt in range(5):
        cv.check(px, colour, filt)


@pytest.mark.parametrize("w,h", [(6000, 3), (2056, 8)], ids=["row-longer-than-a-chunk", "wide-short"])
def test_long_rows(cv, w, h):
    px = gradient_noise(w, h, seed=w)
    cv.put(px)
    stats = cv.check(px, P.RGB, P.ADAPTIVE)
    assert len(stats["payloads"]) == -(-(h * (1 + 3 * w)) // P.CHUNK)
    if w == 6000:
        assert 1 + 3 * w > P.CHUNK
    cv.check(px, P.RGBA, P.PAETH)


def test_fifteen_bit_codes(cv):
    """the literal tree cut from 17 to 15 bits, and the code-length tree cut from 8 to 7: zlib's overflow repair"""
    row = C.fibonacci_row()
    px = C.row_pixels(row)
    cv.put(px)
    stats = cv.check(px, P.RGB, P.NONE)
    block, = blocks_of(stats)
    assert block["type"] == "dynamic" and block["maxlen"][0] == 15 and block["matches"] == 0
    assert C.unlimited_depth(C.literal_counts(row)) == 17
    row, _ = C.code_length_overflow_row()
    px = C.row_pixels(row)
    cv.put(px)
    block, = blocks_of(cv.check(px, P.RGB, P.NONE))
    assert block["maxlen"][2] == 7 and C.unlimited_depth(block["clcounts"]) > 7


def test_adler_past_32_bits(cv):
    """256 x 256 RGBA of 0xFF under filter None: Adler's second sum passes 2^32 many times over before the modulus"""
    px = np.full((256, 256, 4), 255, np.uint8)
    cv.put(px)
    stats = cv.check(px, P.RGBA, P.NONE)
    n = len(stats["stream"])
    assert 255 * n * (n + 1) // 2 > 1 << 40


def test_more_rows_and_chunks_than_one_pass(cv):
    """pt_png_filter's grid is 4096 blocks: 1 x 4100 gives rows a second turn; pt_png_scan takes 256 chunks a turn:
    1400 x 1000 RGB is 258 chunks"""
    px = noise(1, 4100)
    cv.put(px)
    stats = cv.check(px, P.RGB, P.ADAPTIVE)
    assert len(stats["types"]) > 4096
    yy, xx = np.mgrid[0:1000, 0:1400]
    px = np.empty((1000, 1400, 4), np.uint8)
    px[..., 0] = xx // 5
    px[..., 1] = yy // 3
    px[..., 2] = (xx + yy) // 7
    px[..., 3] = 255
    cv.put(px)
    stats = cv.check(px, P.RGB, P.SUB)
    assert len(stats["payloads"]) == 258 > 256


def test_workspace_reuse_and_observer(cv):
    """a smaller canvas after a larger one, the same canvas twice, and the canvas unchanged by the calls"""
    big = noise(100, 100, seed=1)
    cv.put(big)
    cv.check(big, P.RGBA, P.ADAPTIVE)
    small = gradient_noise(17, 9)
    cv.put(small)
    first = cv.engine.encode_canvas_png("rgba", "adaptive")
    assert first == P.encode(small[::-1], P.RGBA, P.ADAPTIVE)
    assert cv.engine.encode_canvas_png("rgba", "adaptive") == first
    assert np.array_equal(cv.engine.read_canvas(17, 9), small)
    assert np.array_equal(cv.tensor.cpu().numpy(), small)


def test_capacity_and_arguments(cv):
    import babylon_pt as bp
    L = bp.lib()
    px = gradient_noise(17, 9, seed=3)
    cv.put(px)
    want = P.encode(px[::-1], P.RGB, P.ADAPTIVE)
    guard = 64
    for cap in (len(want) - 1, 0, 40):
        buf = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
        size = ctypes.c_size_t(0)
        rc = L.pt_canvas_encode_png(cv.engine.ctx, 0, 5, buf, cap, ctypes.byref(size))
        assert rc == PT_ERR_ARG and size.value == len(want)
        assert bytes(buf) == b"\xA5" * (cap + guard)
    buf = (ctypes.c_uint8 * (len(want) + guard))(*([0xA5] * (len(want) + guard)))
    size = ctypes.c_size_t(0)
    assert L.pt_canvas_encode_png(cv.engine.ctx, 0, 5, buf, len(want), ctypes.byref(size)) == 0
    assert size.value == len(want) and bytes(buf)[:len(want)] == want and bytes(buf)[len(want):] == b"\xA5" * guard
    for colour, filt in ((-1, 0), (2, 0), (0, -1), (0, 6)):
        assert L.pt_canvas_encode_png(cv.engine.ctx, colour, filt, buf, len(want), ctypes.byref(size)) == PT_ERR_ARG
    assert L.pt_canvas_encode_png(cv.engine.ctx, 0, 5, None, len(want), ctypes.byref(size)) == PT_ERR_ARG
    assert L.pt_canvas_encode_png(cv.engine.ctx, 0, 5, buf, len(want), None) == PT_ERR_ARG
    fresh = bp.Engine(0)
    try:   # no canvas yet
        assert L.pt_canvas_encode_png(fresh.ctx, 0, 5, buf, len(want), ctypes.byref(size)) == PT_ERR_ARG
    finally:
        fresh.dispose()


def _teapot(engine, frames=2, width=96, height=64):
    import babylon_pt as bp
    meta = H.stream("gltf_teapot_320x180")
    player = bp.StreamPlayer(engine, meta, H.bluenoise(), H.texture_payloads(meta, H.mesh(meta)), width, height)
    engine.resize_canvas(player.width, player.height)
    for i in range(frames):
        player.play_frame(i)
    return player


def test_rendered_frame_is_observed_only():
    """the 96x64 glTF teapot of smoke(), two frames: the encoder runs behind the deferred screenCopy and the
    screenOutput; the file is the reference's for the canvas, decodes to read_pixels flipped, and the fuse, queue and
    job statistics and the canvas are what they were before the call"""
    import babylon_pt as bp
    e = bp.Engine(0)
    try:
        player = _teapot(e)
        data = e.encode_canvas_png("rgba", "adaptive")   # (runs what was deferred, as read_canvas would)
        canvas = e.read_canvas(player.width, player.height)
        assert canvas[..., :3].any()
        assert data == P.encode(canvas[::-1], P.RGBA, P.ADAPTIVE)
        assert np.array_equal(decoded(data), canvas[::-1])
        before = (e.fuse_stats(), e.queue_stats(), e.job_stats())
        rgb = e.encode_canvas_png()
        assert (e.fuse_stats(), e.queue_stats(), e.job_stats()) == before
        assert np.array_equal(e.read_canvas(player.width, player.height), canvas)
        assert rgb == P.encode(canvas[::-1], P.RGB, P.ADAPTIVE)
        assert np.array_equal(decoded(rgb), canvas[::-1, :, :3])
    finally:
        e.dispose()


def test_two_part_context_encodes_the_gathered_canvas():
    import babylon_pt as bp
    got = []
    for devices in (None, [0, 0]):
        e = bp.Engine(0) if devices is None else bp.Engine(devices=devices)
        try:
            player = _teapot(e)
            data = e.encode_canvas_png("rgb", "paeth")
            canvas = e.read_canvas(player.width, player.height)
        finally:
            e.dispose()
        assert data == P.encode(canvas[::-1], P.RGB, P.PAETH)
        got.append(data)
    assert got[0] == got[1]

"""The format of pt_canvas_encode_jpeg_opt with optimize = 1, pinned on the CPU: tests/jpeg_enc_opt_ref.py (the numpy
restatement the GPU tests compare bytes with) writes the file libjpeg-turbo writes, as Pillow runs it with
optimize=True and restart_marker_rows=1, at each subsampling; the file decodes to the pixels of the standard-table
file; and the table construction on counts that force libjpeg's length-limiting loop."""
import io

import numpy as np
import pytest

import jpeg_enc_opt_ref as O
import jpeg_enc_ref as R
import jpeg_enc_sub_ref as S

Image = pytest.importorskip("PIL.Image", reason="Pillow (libjpeg-turbo) is the reference here")

# W x H: 1x1; widths and heights with mod 16 in 1..8 and in 9..15 on either axis (a 4:2:2 / 4:2:0 MCU then has or has
# not dummy Y blocks at the right and the bottom); more than one MCU row; a row of several MCUs
SIZES = [(1, 1), (8, 8), (17, 9), (9, 17), (24, 24), (29, 45), (40, 23), (16, 16), (67, 36)]
QUALITIES = [1, 25, 50, 75, 90, 100]
CONTENTS = ["random", "flat", "smooth"]


def pixels(content, w, h):
    rng = np.random.default_rng(w * 1009 + h * 31 + len(content))
    if content == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "smooth":     # shading plus a little noise: few symbols, some of them rare
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 2 + yy, yy * 3, xx + yy * 2], -1) % 256
        return np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
    return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy()


def pillow_encode(rgb, quality, subsampling, optimize=True):
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=1,
                                     optimize=optimize)
    return buf.getvalue()


@pytest.fixture(scope="module")
def restart_rows():
    """Pillow passes unknown save options by; one that knows restart_marker_rows writes a DRI segment"""
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    if b"\xff\xdd" not in pillow_encode(np.zeros((16, 8, 3), np.uint8), 75, 0):
        pytest.skip("this Pillow has no restart_marker_rows")


@pytest.mark.parametrize("subsampling", [0, 1, 2], ids=["444", "422", "420"])
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_reference_writes_libjpeg_turbos_bytes(restart_rows, size, content, subsampling):
    w, h = size
    rgb = pixels(content, w, h)
    for q in QUALITIES:
        got, stats = O.encode_stats(rgb, q, subsampling)
        assert got == pillow_encode(rgb, q, subsampling), (size, content, q)
        if content == "flat":   # a table of a single symbol and the reserved one: one code of one bit
            assert [sum(bits) for bits, _ in stats["tables"]][1::2] == [1, 1]
            assert stats["tables"][1][0][0] == 1 and stats["tables"][1][1] == [0x00]


@pytest.mark.parametrize("subsampling", [0, 2], ids=["444", "420"])
def test_noisy_frame_at_high_quality_has_long_codes(restart_rows, subsampling):
    """128x144 of noise of every amplitude at quality 95 and 100: dozens of AC symbols, counts from one to
    thousands, codes of 13 bits and more"""
    rgb = O.graded_noise(128, 144, 1)
    for q in (95, 100):
        got, stats = O.encode_stats(rgb, q, subsampling)
        assert got == pillow_encode(rgb, q, subsampling)
        bits, vals = stats["tables"][1]
        assert len(vals) >= 20 and max(i + 1 for i in range(16) if bits[i]) >= 13, (len(vals), bits)


def test_length_limiting_loop_runs(restart_rows):
    """an image whose raw code lengths exceed 16, so that libjpeg's limiting loop decides the table: asserted on the
    reference, then compared with Pillow (the frame of the GPU test aimed at the 64-bit bound: a lane's share of 70
    bits); and the loop driven directly with Fibonacci-like counts (lengths up to 30), where the check is what a
    transcription must keep: the symbols all there, Kraft's sum that of a code with the reserved all-ones code
    missing"""
    rgb = O.lone_coefficient_63()
    got, stats = O.encode_stats(rgb, 95, 0)
    assert got == pillow_encode(rgb, 95, 0)
    assert stats["limited"] >= 1, "no table of this frame had a raw length past 16"
    assert max(O.code_sizes(O.gather(S.mcu_rows(rgb, 95, 0, {"dummy": 0}))[1])) > 16
    assert stats["lane_bits"] == 70 and dict(R._huff(*stats["tables"][1]))[0xF0][1] == 16
    fib = [1, 2]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    freq = [0] * 257
    for i, f in enumerate(fib):
        freq[3 * i + 1] = f
    size = O.code_sizes(freq)
    assert max(size) == 30 and size[256] == 30
    bits, vals, limited = O.gen_optimal_table(freq)
    assert limited and sum(bits) == len(fib) == len(vals) and sorted(vals) == [3 * i + 1 for i in range(30)]
    # the commonest symbols keep the shortest codes
    assert vals[0] == 3 * 29 + 1 and vals[1] == 3 * 28 + 1
    kraft = sum(n * 2 ** (16 - (i + 1)) for i, n in enumerate(bits))
    assert kraft == 2 ** 16 - 1     # complete but for one code of the longest length (16 after the limiting)
    assert bits[15] >= 1


def test_merge_takes_the_larger_index_on_a_tie():
    """four symbols of equal count and the reserved one: c1 = 256 (count 1) merges with the largest real symbol"""
    freq = [0] * 257
    for s in (3, 9, 20, 200):
        freq[s] = 5
    size = O.code_sizes(freq)
    assert [size[s] for s in (3, 9, 20, 200, 256)] == [2, 2, 2, 3, 3]
    bits, vals, limited = O.gen_optimal_table(freq)
    assert bits[:3] == [0, 3, 1] and vals == [3, 9, 20, 200] and not limited


@pytest.mark.parametrize("subsampling", [0, 1, 2], ids=["444", "422", "420"])
def test_only_the_entropy_code_changes(subsampling):
    """the optimised file decodes (libpt's decoder, which reads the tables from the file) to the pixels of the
    standard-table file, is shorter, and has the standard file's header but for the DHT segments"""
    import babylon_pt as bp
    for content, w, h in (("smooth", 67, 36), ("random", 29, 45), ("flat", 17, 9)):
        rgb = pixels(content, w, h)
        for q in (25, 90):
            opt = O.encode(rgb, q, subsampling)
            std = S.encode(rgb, q, subsampling)
            assert np.array_equal(bp.decode_jpeg(opt), bp.decode_jpeg(std))
            assert len(opt) < len(std)
            first, dri = std.index(b"\xff\xc4"), std.index(b"\xff\xdd\x00\x04")
            assert opt[:first] == std[:first] and opt[opt.index(b"\xff\xdd\x00\x04"):][:20] == std[dri:dri + 20]


def test_subsampling_0_statistics_are_the_444_blocks():
    """the histograms count what jpeg_enc_ref's emitter writes: its ZRLs, and one DC symbol per block"""
    rgb = pixels("smooth", 40, 23)
    stats = {"dummy": 0}
    rows = S.mcu_rows(rgb, 50, 0, stats)
    hist = O.gather(rows)
    assert hist[0].sum() == 5 * 3 and hist[2].sum() == 2 * 5 * 3
    assert hist[1, 0xF0] + hist[3, 0xF0] == R.encode_stats(rgb, 50)[1]["zrl"]
    assert hist[:, 256].sum() == 0

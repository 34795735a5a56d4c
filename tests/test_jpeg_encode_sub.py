"""The format of pt_canvas_encode_jpeg_sub, pinned on the CPU: tests/jpeg_enc_sub_ref.py (the numpy restatement the
GPU tests compare bytes with) writes the file libjpeg-turbo writes, as Pillow runs it with subsampling=1 (4:2:2) or
2 (4:2:0) and restart_marker_rows=1; at subsampling 0 it is tests/jpeg_enc_ref.py; and libpt's own decoder reads
the files back as libjpeg-turbo does (its h2v1 and h2v2 upsampling)."""
import io

import numpy as np
import pytest

import jpeg_enc_ref as R
import jpeg_enc_sub_ref as S

Image = pytest.importorskip("PIL.Image", reason="Pillow (libjpeg-turbo) is the reference here")

# W x H: the GPU tests' sizes of both samplings, and odd edges on either axis
SIZES = [(1, 1), (8, 8), (16, 16), (16, 8), (17, 9), (24, 24), (24, 16), (24, 160), (24, 80), (2056, 16), (2056, 8),
         (9, 9), (15, 16), (16, 15), (1, 33)]
QUALITIES = [1, 50, 90, 100]
CONTENTS = ["random", "flat", "extremes"]


def pixels(content, w, h):
    rng = np.random.default_rng(w * 1009 + h * 31 + len(content))
    if content == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "extremes":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy()


def pillow_encode(rgb, quality, subsampling):
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=1)
    return buf.getvalue()


@pytest.fixture(scope="module")
def restart_rows():
    """Pillow passes unknown save options by; one that knows restart_marker_rows writes a DRI segment"""
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    if b"\xff\xdd" not in pillow_encode(np.zeros((16, 8, 3), np.uint8), 75, 0):
        pytest.skip("this Pillow has no restart_marker_rows")


@pytest.mark.parametrize("subsampling", [1, 2], ids=["422", "420"])
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_reference_writes_libjpeg_turbos_bytes(restart_rows, size, content, subsampling):
    w, h = size
    rgb = pixels(content, w, h)
    for q in QUALITIES:
        assert S.encode(rgb, q, subsampling) == pillow_encode(rgb, q, subsampling), (size, content, q)


@pytest.mark.parametrize("size", [(1, 1), (17, 9), (24, 24), (16, 15)], ids=lambda s: "%dx%d" % s)
def test_subsampling_0_is_the_444_reference(size):
    w, h = size
    for content in CONTENTS:
        rgb = pixels(content, w, h)
        for q in QUALITIES:
            data, stats = S.encode_stats(rgb, q, 0)
            want, wstats = R.encode_stats(rgb, q)
            assert data == want and stats["dummy"] == 0
            assert {k: stats[k] for k in wstats} == wstats


@pytest.mark.parametrize("subsampling", [1, 2], ids=["422", "420"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_own_decoder_reads_the_reference_as_libjpeg_turbo_does(size, subsampling):
    import babylon_pt as bp
    w, h = size
    for content in CONTENTS:
        for q in (1, 50, 100):
            data = S.encode(pixels(content, w, h), q, subsampling)
            want = np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"), dtype=np.uint8)
            assert want.shape == (h, w, 4)
            assert np.array_equal(bp.decode_jpeg(data), want), (size, content, q)


def test_reference_counts_dummy_blocks():
    """the counts the GPU cases assert: Y blocks of an MCU outside the ceil(W / 8) x ceil(H / 8) real ones"""
    want = {(2, 1, 1): 3, (2, 8, 8): 3, (2, 16, 16): 0, (2, 17, 9): 2, (2, 24, 24): 7, (2, 24, 160): 20,
            (2, 2056, 16): 2, (1, 1, 1): 1, (1, 8, 8): 1, (1, 16, 8): 0, (1, 17, 9): 2, (1, 24, 16): 2,
            (1, 24, 80): 10, (1, 2056, 8): 1}
    for (ss, w, h), n in want.items():
        assert S.encode_stats(np.zeros((h, w, 3), np.uint8), 50, ss)[1]["dummy"] == n, (ss, w, h)

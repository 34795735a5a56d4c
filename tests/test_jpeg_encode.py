"""The format of pt_canvas_encode_jpeg, pinned on the CPU: tests/jpeg_enc_ref.py (the numpy restatement the GPU
tests compare bytes with) writes the file libjpeg-turbo writes, as Pillow runs it with subsampling=0 and
restart_marker_rows=1, and libpt's own decoder reads it back as libjpeg-turbo does."""
import io

import numpy as np
import pytest

import jpeg_enc_ref as R

Image = pytest.importorskip("PIL.Image", reason="Pillow (libjpeg-turbo) is the reference here")

SIZES = [(1, 1), (8, 8), (37, 19), (24, 16), (9, 72)]       # W x H
QUALITIES = [1, 25, 50, 75, 90, 100]
CONTENTS = ["random", "gradient", "extremes"]


def pixels(content, w, h):
    rng = np.random.default_rng(w * 1009 + h * 31 + len(content))
    if content == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "extremes":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx * 255 // max(1, w - 1), yy * 255 // max(1, h - 1), (xx + yy) * 255 // max(1, w + h - 2)],
                    -1).astype(np.uint8)


def pillow_encode(rgb, quality):
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=quality, subsampling=0, restart_marker_rows=1)
    return buf.getvalue()


@pytest.fixture(scope="module")
def restart_rows():
    """Pillow passes unknown save options by; one that knows restart_marker_rows writes a DRI segment"""
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    if b"\xff\xdd" not in pillow_encode(np.zeros((16, 8, 3), np.uint8), 75):
        pytest.skip("this Pillow has no restart_marker_rows")


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_reference_writes_libjpeg_turbos_bytes(restart_rows, size, content):
    w, h = size
    rgb = pixels(content, w, h)
    for q in QUALITIES:
        assert R.encode(rgb, q) == pillow_encode(rgb, q), (size, content, q)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_own_decoder_reads_the_reference_as_libjpeg_turbo_does(size):
    import babylon_pt as bp
    w, h = size
    for content in CONTENTS:
        for q in (1, 50, 100):
            data = R.encode(pixels(content, w, h), q)
            want = np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"), dtype=np.uint8)
            assert want.shape == (h, w, 4)
            assert np.array_equal(bp.decode_jpeg(data), want), (size, content, q)


def test_reference_reports_zrl_and_stuffing():
    """the two paths the GPU cases must reach are counted: a lone high-frequency coefficient needs ZRL codes, and
    noise at quality 100 has 0xFF bytes in its entropy-coded data"""
    yy, xx = np.mgrid[0:8, 0:8]
    tile = np.rint(128 + 100 * np.cos((2 * xx + 1) * 7 * np.pi / 16) * np.cos((2 * yy + 1) * 7 * np.pi / 16))
    grey = np.repeat(np.tile(tile.astype(np.uint8), (2, 3))[:, :, None], 3, 2)
    data, stats = R.encode_stats(grey, 50)
    assert stats["zrl"] >= 1
    data, stats = R.encode_stats(pixels("random", 37, 19), 100)
    assert stats["stuffed"] >= 1 and data.count(b"\xff\x00") >= stats["stuffed"]

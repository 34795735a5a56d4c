"""The references of tests/test_gpu_jpeg_encode_scale.py pinned on the CPU at that file's sizes and contents:
tests/jpeg_enc_sub_ref.py and tests/jpeg_enc_opt_ref.py write the file libjpeg-turbo writes, as Pillow runs it with
restart_marker_rows=1, at 257 MCU rows and at 6145 MCUs (the other CPU tests stop at 67x36). libjpeg refuses an axis
above 65500 (JPEG_MAX_DIMENSION), so the longest axis is pinned at 65500, and the references at 65535 are tied to
those: the same header but for the fields that carry the size, and a stream libpt's own decoder reads."""
import io

import numpy as np
import pytest

import jpeg_enc_opt_ref as O
import jpeg_enc_sub_ref as S
import test_gpu_jpeg_encode_scale as G

Image = pytest.importorskip("PIL.Image", reason="Pillow (libjpeg-turbo) is the reference here")

LIBJPEG_MAX = 65500
SAMPLINGS = [G.S444, G.S422, G.S420]
SS_IDS = ["444", "422", "420"]


def pillow_encode(rgb, quality, subsampling, optimize):
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=1,
                                     optimize=optimize)
    return buf.getvalue()


@pytest.fixture
def pillow(monkeypatch):
    """Pillow on libjpeg-turbo with restart_marker_rows (one that does not know the option passes it by and writes no
    DRI segment), and a write buffer that holds these files: at the default size a tall file ends in "Suspension not
    allowed here"."""
    from PIL import ImageFile, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    if b"\xff\xdd" not in pillow_encode(np.zeros((16, 8, 3), np.uint8), 75, 0, False):
        pytest.skip("this Pillow has no restart_marker_rows")
    monkeypatch.setattr(ImageFile, "MAXBLOCK", 1 << 26)


def ours(rgb, quality, subsampling, optimize):
    return O.encode_stats(rgb, quality, subsampling) if optimize else S.encode_stats(rgb, quality, subsampling)


@pytest.mark.parametrize("optimize", [False, True], ids=["std", "opt"])
@pytest.mark.parametrize("kind,q", [("random", 100), ("graded", 90)], ids=["random-q100", "graded-q90"])
@pytest.mark.parametrize("case", G.ROWS257, ids=G.case_id)
def test_257_mcu_rows_are_libjpeg_turbos(pillow, case, kind, q, optimize):
    ss, w, h = case
    rgb = G.top_down(G.content(kind, w, h))
    assert ours(rgb, q, ss, optimize)[0] == pillow_encode(rgb, q, ss, optimize)


@pytest.mark.parametrize("optimize", [False, True], ids=["std", "opt"])
@pytest.mark.parametrize("case", G.MANY, ids=G.case_id)
def test_thousands_of_mcu_rows_are_libjpeg_turbos(pillow, case, optimize):
    ss, w, h = case
    rgb = G.top_down(G.content("graded", w, h))
    assert ours(rgb, 90, ss, optimize)[0] == pillow_encode(rgb, 90, ss, optimize)


@pytest.mark.parametrize("ss", SAMPLINGS, ids=SS_IDS)
@pytest.mark.parametrize("size", [(LIBJPEG_MAX, 1), (1, LIBJPEG_MAX)], ids=lambda s: "%dx%d" % s)
def test_libjpegs_longest_axis(pillow, size, ss):
    """65500 columns or rows, the most libjpeg writes; at 4:2:0 the other axis' one pixel leaves two dummy Y blocks in
    each of the 4094 MCUs"""
    w, h = size
    rgb = G.top_down(G.content("random", w, h))
    for optimize in (False, True):
        got, stats = ours(rgb, 90, ss, optimize)
        assert got == pillow_encode(rgb, 90, ss, optimize), (size, ss, optimize)
        if ss == G.S420:
            assert stats["dummy"] == 8188


def test_libjpeg_refuses_one_more(pillow):
    """why the GPU cases at 65535 are tied to Pillow only through 65500: libjpeg itself stops there, writing and
    reading"""
    for w, h in ((LIBJPEG_MAX + 1, 1), (1, LIBJPEG_MAX + 1)):
        with pytest.raises(Exception):
            pillow_encode(np.zeros((h, w, 3), np.uint8), 90, 0, False)
    data = G.reference("random", 65535, 1, 0, 90, G.S444, False)[0]
    with pytest.raises(Exception):
        Image.open(io.BytesIO(data)).load()


def fields(head):
    """where SOF0 holds the height and the width and DRI the interval, in a header of the references"""
    sof, dri = head.index(b"\xff\xc0"), head.index(b"\xff\xdd\x00\x04")
    return sof + 5, sof + 7, dri + 4


@pytest.mark.parametrize("case", G.LIMITS, ids=G.case_id)
def test_the_formats_longest_axis_differs_from_libjpegs_in_the_size_fields(case):
    """The references at 65535, which Pillow cannot write: the header is the one at 65500 but for SOF0's height and
    width and DRI's MCUs per row, which hold the canvas's; and libpt's decoder, which libjpeg-turbo's decompression pins
    (tests/test_jpeg.py), reads the file to the canvas's shape, the optimised one to the pixels of the standard one."""
    import babylon_pt as bp
    ss, w, h, modes = case
    hs = S.SAMPLING[ss][0]
    w0, h0 = min(w, LIBJPEG_MAX), min(h, LIBJPEG_MAX)
    big, small = S.header(w, h, 90, ss), S.header(w0, h0, 90, ss)
    assert len(big) == len(small)
    at_h, at_w, at_dri = fields(big)
    assert (at_h, at_w, at_dri) == fields(small)
    size_bytes = set(range(at_h, at_h + 4)) | {at_dri, at_dri + 1}
    assert all(big[i] == small[i] for i in range(len(big)) if i not in size_bytes)
    for head, (ww, hh) in ((big, (w, h)), (small, (w0, h0))):
        assert int.from_bytes(head[at_h:at_h + 2], "big") == hh and int.from_bytes(head[at_w:at_w + 2], "big") == ww
        assert int.from_bytes(head[at_dri:at_dri + 2], "big") == -(-ww // (8 * hs))
    decoded = []
    for optimize in modes:
        data = G.reference("random", w, h, 0, 90, ss, optimize)[0]
        if optimize:    # the optimised header: the same but for the DHT segments
            first, dri = big.index(b"\xff\xc4"), big.index(b"\xff\xdd\x00\x04")
            assert data[:first] == big[:first] and data[data.index(b"\xff\xdd\x00\x04"):][:20] == big[dri:dri + 20]
        else:
            assert data[:len(big)] == big
        px = bp.decode_jpeg(data)
        assert px.shape == (h, w, 4)
        decoded.append(px)
    if len(decoded) == 2:
        assert np.array_equal(decoded[0], decoded[1])

"""pt_canvas_encode_jpeg_opt on the GPU at the scale of a frame: the loops of csrc/pt_jpeg_enc.hip that the sizes of
tests/test_gpu_jpeg_encode*.py (32 MCU rows, 1024 MCUs, 774 blocks in a row at the most) never enter. Every comparison
is bytes == tests/jpeg_enc_sub_ref.py (optimize = 0) or tests/jpeg_enc_opt_ref.py (optimize = 1) over the canvas
top-down, no tolerance; tests/test_jpeg_encode_scale.py pins both against libjpeg-turbo at these sizes. Sizes are
W x H, narrow and tall: the fewest pixels that give the MCU rows and MCUs each loop needs.

  ROWS257  257 MCU rows: pt_jpeg_scan_rows' second tile of 256 rows, one row long, and the carry into it.
  MANY     6145 MCUs (4:2:0: 6146) in 6145 (3073) MCU rows: half of the waves of pt_jpeg_hist's 1024 blocks x 4 take
           a second MCU, the others end after one; 25 (13) tiles of pt_jpeg_scan_rows, the last one partial.
  LIMITS   65535 on one axis, 1 on the other: one restart interval of 8192 MCUs (24 576 blocks: 96 tiles of
           pt_jpeg_scan_blocks, hundreds of kJpegTile tiles in pt_jpeg_count_ff and pt_jpeg_pack, which 32 blocks
           share), or 8192 MCU rows (pt_jpeg_pack's gridDim.y); and 65536, which is refused.
  and the sizes in a row on one engine, so that a small canvas is encoded in a workspace a tall one left full."""
import ctypes
import functools

import numpy as np
import pytest

import jpeg_enc_opt_ref as O
import jpeg_enc_sub_ref as S

pytestmark = pytest.mark.gpu

S444, S422, S420 = 0, 1, 2
ROWS257 = [(S444, 8, 2056), (S422, 16, 2056), (S420, 16, 4112)]
MANY = [(S444, 8, 49160), (S422, 16, 49160), (S420, 32, 49168)]
# (subsampling, W, H, the values of optimize)
LIMITS = [(S444, 65535, 1, (False, True)), (S444, 1, 65535, (False, True)),
          (S420, 65535, 1, (True,)), (S420, 1, 65535, (True,)), (S422, 65535, 1, (False,))]
# the ROWS257 files longer than 64 KiB, (subsampling, content, optimize): the first capacity of
# Engine.encode_canvas_jpeg and the least size of the stream buffer (pt_plan.h jpeg_out_room), so these take the
# second call and a stream buffer sized from the stream (4:2:2 random optimised is 63 003 B)
LONG = {(S444, "random", False), (S422, "random", False), (S420, "random", False), (S420, "random", True)}
FIRST_PASS = 1024 * 4   # the MCUs of pt_jpeg_hist's first pass: kHistBlocks blocks of kWaves waves
PT_ERR_ARG = -1


def case_id(c):
    return "%s-%dx%d" % ({S444: "444", S422: "422", S420: "420"}[c[0]], c[1], c[2])


def content(kind, w, h, seed=0):
    """RGBA8 canvas rows (bottom-up, as the canvas is); the alpha is random in every case"""
    rng = np.random.default_rng(w * 1009 + h * 31 + seed)
    px = np.empty((h, w, 4), np.uint8)
    if kind == "random":
        px[..., :3] = rng.integers(0, 256, (h, w, 3))
    elif kind == "graded":      # the amplitude rises in raster order: the last MCUs have other statistics than the first
        px[..., :3] = O.graded_noise(w, h, seed + 5)
    else:
        raise ValueError(kind)
    px[..., 3] = rng.integers(0, 256, (h, w))
    return px


def top_down(px):
    return np.ascontiguousarray(px[::-1, :, :3])


@functools.lru_cache(maxsize=None)
def reference(kind, w, h, seed, q, ss, optimize):
    """(file, stats) of content(kind, w, h, seed), once for all the tests that encode that canvas"""
    rgb = top_down(content(kind, w, h, seed))
    return O.encode_stats(rgb, q, ss) if optimize else S.encode_stats(rgb, q, ss)


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


@pytest.mark.parametrize("kind,q", [("random", 100), ("graded", 90)], ids=["random-q100", "graded-q90"])
@pytest.mark.parametrize("case", ROWS257, ids=case_id)
def test_257_mcu_rows(cv, case, kind, q):
    """a second tile of pt_jpeg_scan_rows that holds one row: a carry dropped or taken twice puts row 256, its RST
    and the EOI at the wrong offset"""
    ss, w, h = case
    assert -(-h // (8 * S.SAMPLING[ss][1])) == 257
    cv.put(content(kind, w, h))
    for optimize in (False, True):
        want, stats = reference(kind, w, h, 0, q, ss, optimize)
        print("%s %s optimize=%d: %d B, %d stuffed" % (case_id(case), kind, optimize, len(want), stats["stuffed"]))
        assert stats["stuffed"] >= 1
        assert (len(want) > 65536) == ((ss, kind, optimize) in LONG)
        assert cv.encode(q, ss, optimize) == want, (case, kind, q, optimize)


def first_pass_rows(ss, w):
    """the MCU rows that hold exactly the first FIRST_PASS MCUs of a canvas W wide"""
    mcus_x = -(-w // (8 * S.SAMPLING[ss][0]))
    assert FIRST_PASS % mcus_x == 0
    return FIRST_PASS // mcus_x


@pytest.mark.parametrize("case", MANY, ids=case_id)
def test_more_mcus_than_histogram_waves(cv, case):
    """Optimised tables of a canvas whose MCUs past the first 4096 have other statistics than those. Shown on the
    reference before the device is asked: the tables of the histogram of the first 4096 MCUs alone (a loop that ends
    after its first pass) and those of the histogram with the others counted twice (a wrong stride) are not the true
    ones, so the file would differ. Counts add, so the histogram of all MCUs is the sum of the two parts'; the tables
    built from that sum are the ones in the reference's file."""
    ss, w, h = case
    px = content("graded", w, h)
    want, stats = reference("graded", w, h, 0, 90, ss, True)
    rows = S.mcu_rows(top_down(px), 90, ss, {"dummy": 0})
    n = first_pass_rows(ss, w)
    assert n < len(rows) < 2 * n    # a second pass for some waves and no third for any
    head, tail = O.gather(rows[:n]), O.gather(rows[n:])
    full = head + tail

    def tables(hist):
        return [tuple(O.gen_optimal_table(f)[:2]) for f in hist]

    true = tables(full)
    assert true == [tuple(t) for t in stats["tables"]]
    assert any(a != b for a, b in zip(tables(head), true)), "the first 4096 MCUs alone give the true tables: another seed"
    assert any(a != b for a, b in zip(tables(full + tail), true)), "the tail counted twice gives the true tables: another seed"
    cv.put(px)
    assert cv.encode(90, ss, True) == want, case


@pytest.mark.parametrize("case", MANY, ids=case_id)
def test_thousands_of_mcu_rows_standard_tables(cv, case):
    """the same canvas with the Annex K tables: 25 (4:2:0: 13) tiles of pt_jpeg_scan_rows, the last one partial"""
    ss, w, h = case
    cv.put(content("graded", w, h))
    assert cv.encode(90, ss, False) == reference("graded", w, h, 0, 90, ss, False)[0], case


@pytest.mark.parametrize("case", LIMITS, ids=case_id)
def test_largest_canvas_on_either_axis(cv, case):
    """65535 columns are one restart interval of 8192 (4:2:2, 4:2:0: 4096) MCUs, 65535 rows 8192 (4096) intervals of
    one MCU; at 4:2:0 the other axis' single pixel leaves half of every MCU's Y blocks dummies"""
    ss, w, h, modes = case
    cv.put(content("random", w, h))
    for optimize in modes:
        want, stats = reference("random", w, h, 0, 90, ss, optimize)
        if ss == S420:
            assert stats["dummy"] == 8192
        assert cv.encode(90, ss, optimize) == want, (case, optimize)


@pytest.mark.parametrize("size", [(65536, 1), (1, 65536)], ids=lambda s: "%dx%d" % s)
def test_one_past_the_limit_is_refused(cv, size):
    """SOF0 has 16 bits for each axis: PT_ERR_ARG, nothing written"""
    import babylon_pt as bp
    L = bp.lib()
    w, h = size
    cv.put(content("random", w, h))
    cap, guard = 1 << 20, 64
    buf = (ctypes.c_uint8 * (cap + guard))()
    ctypes.memset(buf, 0xA5, cap + guard)
    size = ctypes.c_size_t(0)
    for ss, opt in ((S444, 0), (S444, 1), (S422, 0), (S420, 1)):
        assert L.pt_canvas_encode_jpeg_opt(cv.engine.ctx, 90, ss, opt, buf, cap, ctypes.byref(size)) == PT_ERR_ARG
        assert bytes(buf) == b"\xA5" * (cap + guard) and size.value == 0


def test_calls_in_a_row_at_scale():
    """One engine from its first call on: a canvas of 6145 MCU rows, a 17x9 one in the workspace that one left
    (row offsets, row lengths, tile offsets, histograms and a stream beyond what the small call rewrites), a wider
    tall one of other pixels at another sampling, and 257 rows with the standard tables; no call changes the canvas"""
    c = Canvas()
    try:
        steps = [("graded", 8, 49160, 0, 90, S444, (True,)),
                 ("random", 17, 9, 3, 90, S420, (True, False)),
                 ("random", 16, 49160, 7, 90, S422, (True,)),
                 ("random", 8, 2056, 0, 100, S444, (False,))]
        for kind, w, h, seed, q, ss, modes in steps:
            px = content(kind, w, h, seed)
            c.put(px)
            for optimize in modes:
                assert c.encode(q, ss, optimize) == reference(kind, w, h, seed, q, ss, optimize)[0], (w, h, optimize)
            assert np.array_equal(c.tensor.cpu().numpy(), px)
    finally:
        c.engine.dispose()

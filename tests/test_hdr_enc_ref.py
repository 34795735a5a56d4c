"""The definition of pt_target_encode_hdr's file checks itself (tests/hdr_enc_ref.py): the rule form of the plane
coder equals the sequential form of Radiance's scanline writer, every file decodes through pt_assets.decode_hdr to
byte x 2^(E - 136), the decoded values lie at or below the scaled input and within max x 2^-7 of it, no coded plane
exceeds W + ceil(W / 128), the special texels give the stated bytes, and the shared cases reach what they are for."""
import numpy as np
import pytest

import hdr_enc_cases as C
import hdr_enc_ref as R
import pt_assets

CASES = C.cases()


def test_rule_form_is_the_sequential_form_on_random_planes():
    rng = np.random.default_rng(11)
    for i in range(3000):
        w = int(rng.integers(1, 700))
        kind = i % 4
        if kind == 0:
            p = rng.integers(0, 256, w, dtype=np.uint8)
        elif kind == 1:
            p = rng.integers(0, 2, w, dtype=np.uint8)
        elif kind == 2:   # runs of geometric lengths
            p = np.repeat(rng.integers(0, 4, w, dtype=np.uint8), rng.geometric(0.05, w))[:w]
        else:
            p = C.mixed_row(w, rng)
        a, b = R.code_plane(p), R.code_plane_sequential(p)
        assert a == b, (i, w)
        assert len(a) <= R.plane_max(w)


@pytest.mark.parametrize("L", C.RUN_LENGTHS)
def test_rule_form_is_the_sequential_form_at_the_run_lengths(L):
    for before in (0, 1, 2, 3, 5, 127, 128, 129):
        for after in (0, 1, 2, 3, 5, 128):
            p = C.plane(before + L + after, C.literal(before), L, C.literal(after, 9))
            assert R.code_plane(p) == R.code_plane_sequential(p), (L, before, after)


def test_tokens_at_the_run_lengths():
    tok = lambda p: [(k, n) for k, _, n in R.tokens(p)]
    run = lambda n: np.full(n, 9, np.uint8)
    assert tok(run(3)) == [("short", 3)]
    assert tok(run(4)) == [("run", 4)]
    assert tok(run(127)) == [("run", 127)]
    assert tok(run(128)) == [("run", 127), ("literal", 1)]
    assert tok(run(130)) == [("run", 127), ("short", 3)]
    assert tok(run(131)) == [("run", 127), ("run", 4)]
    assert tok(run(258)) == [("run", 127), ("run", 127), ("run", 4)]
    assert tok(run(381)) == [("run", 127)] * 3
    assert tok(C.literal(257)) == [("literal", 128), ("literal", 128), ("literal", 1)]
    assert tok(np.concatenate((run(128), np.full(2, 8, np.uint8)))) == [("run", 127), ("literal", 3)]
    assert R.code_plane(np.array([5, 5, 7], np.uint8)) == bytes([3, 5, 5, 7])
    assert R.code_plane(np.array([5, 5], np.uint8)) == bytes([130, 5])


def test_special_texels():
    cap, big = float(R.CAP), float(np.finfo(np.float32).max)
    one = lambda v, s=1.0: tuple(int(x) for x in R.rgbe(np.array([v, v, v], np.float32), s))
    for v in (np.nan, -1.0, -0.0, 1e-33):
        assert one(v) == (0, 0, 0, 0), v
    assert one(np.float32(1e-32)) == (207, 207, 207, 22)     # 1e-32 = 0.8113 x 2^-106, and 0.8113 x 256 = 207.7
    assert one(0.5) == (128, 128, 128, 128)
    assert one(1.0) == (128, 128, 128, 129)
    for v in (np.inf, cap, big):
        assert one(v) == (255, 255, 255, 255), v
    # beside an ordinary component the special one is 0 (or the cap), and the others keep their bytes
    assert tuple(R.rgbe(np.array([np.nan, 0.75, -2.0], np.float32), 1.0)) == (0, 192, 0, 128)
    assert tuple(R.rgbe(np.array([np.inf, 1.0, 1.0], np.float32), 1.0)) == (255, 0, 0, 255)
    assert tuple(R.rgbe(np.array([1.0, 0.5, 0.25], np.float32), 0.5)) == (128, 64, 32, 128)
    # the page's own decoders
    assert float(R.decoded(np.array([255, 255, 255, 255], np.uint8))[0]) == cap


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_decodes_and_holds_the_bounds(name):
    tex, scale = CASES[name]
    h, w = tex.shape[:2]
    data = R.encode(tex, scale)
    assert data.startswith(R.header(w, h))
    assert len(data) <= R.file_max(w, h)
    q = R.scanlines(tex, scale)
    # the project's decoder returns byte x 2^(E - 136), rows in file order
    got = pt_assets.decode_hdr(data)
    assert got.shape == (h, w, 4)
    assert np.array_equal(got[..., :3].astype(np.float64), R.decoded(q))
    # at or below the scaled input and within max x 2^-7 of it, where the input is finite and in [1e-32, 2^126)
    with np.errstate(all="ignore"):
        v = (tex[::-1, :, :3] * np.float32(scale)).astype(np.float64)
    c = np.where(v > 0, v, 0.0)
    m = c.max(axis=-1)
    ok = np.isfinite(v).all(axis=-1) & (m >= float(R.TINY)) & (m < 2.0 ** 126)
    d = R.decoded(q)
    assert np.all(d[ok] <= c[ok])
    assert np.all(c[ok] - d[ok] <= (m[ok] * 2.0 ** -7)[:, None])
    if not R.flat_width(w):
        for y in range(h):
            for k in range(4):
                p = q[y, :, k]
                coded = R.code_plane(p)
                assert len(coded) <= R.plane_max(w)
                if h * w <= 40000:
                    assert coded == R.code_plane_sequential(p)


def test_cases_reach_what_they_are_for():
    cert = {n: R.certificate(*CASES[n]) for n in ("runs", "stretches", "straddle", "size-300x5", "size-16x600",
                                                  "size-129x2", "size-7x3", "size-32768x1", "size-32767x1", "size-8x2")}
    assert cert["size-7x3"]["flat"] and cert["size-32768x1"]["flat"] and not cert["size-8x2"]["flat"]
    assert not cert["size-32767x1"]["flat"] and cert["size-32767x1"]["byte_steps"] == 512
    # every run length as a maximal run, and all three token kinds
    assert set(C.RUN_LENGTHS) <= cert["runs"]["run_lengths"]
    assert cert["runs"]["kinds"] == {"run", "short", "literal"} and cert["runs"]["run"] == 127
    assert cert["stretches"]["kinds"] == {"run", "short", "literal"} and cert["stretches"]["literal"] == 128
    assert {127, 128, 1} <= cert["stretches"]["literal_lengths"]
    # noise rows: planes at their bound, more runs than one step holds, stretches across run steps
    assert cert["size-300x5"]["at_bound"] >= 2 and cert["size-300x5"]["run_steps"] >= 2
    assert cert["size-129x2"]["at_bound"] >= 2 and cert["size-129x2"]["byte_steps"] == 3
    assert cert["size-300x5"]["stretch_across_run_step"] and cert["straddle"]["stretch_across_run_step"]
    assert cert["straddle"]["run_across_byte_step"] and cert["runs"]["run_across_byte_step"]
    # more planes than waves in flight
    assert cert["size-16x600"]["plane_loop"] and not cert["size-300x5"]["plane_loop"]
    # more texels than one trip of the conversion's grid, coded and flat; no other case has
    grid = {n: R.certificate(*CASES[n]) for n in ("grid-1100x960", "grid-7x150000")}
    assert grid["grid-1100x960"]["texel_loop"] and not grid["grid-1100x960"]["flat"]
    assert grid["grid-1100x960"]["kinds"] == {"run", "short", "literal"}
    assert grid["grid-7x150000"]["texel_loop"] and grid["grid-7x150000"]["flat"]
    assert not any(R.certificate(*CASES[n])["texel_loop"] for n in ("runs", "size-32768x1", "size-32767x1"))

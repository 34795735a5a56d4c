"""The bilinear samplers (tex_bilinear / tex_bilinear_f in oracle/ptoracle.c, which texBilinear / texBilinearF
in csrc/pt_device.h restate line for line) against the specification's texture() at level 0, LINEAR, REPEAT
(tests/tex_ref.py), bit for bit, texel index for texel index; and the cases of tests/texture_cases.py certified
on the oracle's tap log: each one really reaches the wrap seams, the UV ranges and the non-finite coordinates
it is named for, on every map it samples, and its maps decide a good part of the frame.

CPU only; tests/test_gpu_texture_cases.py draws the same cases on the device.
"""
import numpy as np
import pytest

import helpers as H
import ptoracle as po
import tex_ref as R
import texture_cases as C

# ------------------------------------------------------------------------------------------ the probe

PROBE_SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (37, 29), (255, 257), (2048, 1024))    # W x H
PERIODS = (-3.0, -1.0, 1.0, 1000.0)
SPECIALS = (0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 2.0 ** 24, -2.0 ** 24, 3e38, -3e38, np.inf, -np.inf, np.nan)


def _probe_map(kind, w, h):
    """Seeded texels with 0 and 255 (0.0 and 1.0) among them, components in [0, 1] for RGBA32F too."""
    rng = np.random.default_rng([3, kind, w, h])
    if kind == 0:
        m = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        m[0, 0], m[-1, -1] = (0, 255, 0, 255), (255, 0, 255, 0)
    else:
        m = rng.random((h, w, 4), dtype=np.float32)
        m[0, 0], m[-1, -1] = (0.0, 1.0, 0.0, 1.0), (1.0, 0.0, 1.0, 0.0)
    assert m.min() == 0 and m.max() == (255 if kind == 0 else 1.0)
    return m


def _neighbours(x):
    x = np.asarray(x, np.float32)
    return np.concatenate([x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))])


def _axis_values(n):
    """Every texel edge k / n and centre (k + 1/2) / n of an axis of n texels, each with its float32 neighbours
    below and above; the same shifted by whole periods, again with the neighbours of the shifted value; and the
    special values."""
    k = np.arange(n + 1)
    base = np.concatenate([k / n, (k[:-1] + 0.5) / n]).astype(np.float32)
    vals = [_neighbours(base)]
    for p in PERIODS:
        vals.append(_neighbours(base + np.float32(p)))
    vals.append(np.array(SPECIALS, np.float32))
    return np.concatenate(vals)


def _probe_uv(w, h):
    """Pairs: every u of the u axis with a seeded v of the v axis and the other way round, the specials crossed
    with one another, and 512 seeded pairs over [-4, 4)."""
    rng = np.random.default_rng([4, w, h])
    us, vs = _axis_values(w), _axis_values(h)
    sp = np.array(SPECIALS, np.float32)
    u = np.concatenate([us, rng.choice(us, vs.size), np.repeat(sp, sp.size), rng.random(512, dtype=np.float32) * 8 - 4])
    v = np.concatenate([rng.choice(vs, us.size), vs, np.tile(sp, sp.size), rng.random(512, dtype=np.float32) * 8 - 4])
    return u.astype(np.float32), v.astype(np.float32)


def _same_bits(a, b):
    """Bit equality, a NaN matching a NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("kind", [0, 1], ids=["rgba8", "rgba32f"])
@pytest.mark.parametrize("size", PROBE_SIZES, ids=["%dx%d" % s for s in PROBE_SIZES])
def test_probe_is_the_specification_bit_for_bit(size, kind):
    """The oracle's sampler returns tex_ref.sample's bits (NaN for NaN) and reads tex_ref.taps's four texels,
    at every texel edge and centre of both axes with their float32 neighbours, whole periods away, and at +-0,
    denormals, +-2^24, +-3e38, +-inf and NaN; tex_ref.sample lies within the derived bound of the float64
    evaluation of the specification's sum."""
    w, h = size
    tex = _probe_map(kind, w, h)
    u, v = _probe_uv(w, h)
    with po.TapLog(u.size) as log:
        got = po.tex_probe(tex, u, v)
    want = R.sample(tex, u, v)
    ok = _same_bits(got, want).all(-1)
    assert ok.all(), "%d of %d coordinates differ, first (u, v) = (%r, %r): %s / %s" % (
        (~ok).sum(), ok.size, u[~ok][0], v[~ok][0], got[~ok][0], want[~ok][0])
    assert log.dropped == 0 and log.rows.size == u.size and (log.rows["map"] == po.TAP_MAPS.index("probe")).all()
    assert (log.rows["bounce"] == -1).all()
    assert _same_bits(log.rows["u"], u).all() and _same_bits(log.rows["v"], v).all()
    for name, idx in zip(("x0", "y0", "x1", "y1"), R.taps(tex, u, v)):
        bad = log.rows[name] != idx
        assert not bad.any(), "%s differs at (u, v) = (%r, %r): %d / %d" % (name, u[bad][0], v[bad][0], log.rows[name][bad][0], idx[bad][0])
    # the non-finite pin was met, and finite coordinates far from 0 were
    with np.errstate(all="ignore"):
        nonfinite = ~np.isfinite(u * np.float32(w))
    assert nonfinite.any() and (log.rows["x0"][nonfinite] == 0).all() and (log.rows["x1"][nonfinite] == 1 % w).all()
    assert np.isnan(got[nonfinite]).all()
    # within the derived bound of the float64 evaluation, wherever that is finite
    ref64 = R.sample64(tex, u, v)
    fin = np.isfinite(ref64).all(-1)
    assert fin.sum() > u.size // 2 and np.isfinite(want[fin]).all()
    err = np.abs(want[fin].astype(np.float64) - ref64[fin]).max()
    assert err <= (R.BOUND_RGBA8 if kind == 0 else R.BOUND_RGBA32F), err


def test_tap_log_counts_what_does_not_fit_and_wants_one_thread():
    tex = _probe_map(0, 3, 5)
    u = np.linspace(-1, 2, 10, dtype=np.float32)
    with po.TapLog(4) as log:
        po.tex_probe(tex, u, u)
    assert log.rows.size == 4 and log.dropped == 6
    after = po.tex_probe(tex, u, u)                   # unbound again: nothing is written
    assert log.rows.size == 4 and np.array_equal(after, R.sample(tex, u, u))
    c = C.case("sizes", C.STREAMS[0], C.SMALL)
    sc = po.Scene(c["meta"]["scene"], 33, 17, H.bluenoise(), c["mesh"]["bvh"], c["mesh"]["tri"], None, c["steps"][0])
    u0 = H.with_resolution(H.path_call(c["meta"]["frames"][0])["uniforms"], 33, 17)
    with po.TapLog(16):
        with pytest.raises(RuntimeError, match="-4"):
            sc.path_trace(u0, np.zeros((17, 33, 4), np.float32), nthreads=0)


# ------------------------------------------------------------------------------------------ reach

_TAPPED = {}


def _tapped(name, stream, size=C.SIZE):
    """The case on the oracle with the tap log bound (one thread), once; its pixels are the threaded run's."""
    key = (name, stream, size)
    if key not in _TAPPED:
        run = C.oracle_run(C.case(name, stream, size), taps=True)
        ref = C.reference(name, stream, size)
        assert run["dropped"] == 0, "the tap log was truncated: %d rows dropped" % run["dropped"]
        assert all(_same_bits(a, b).all() for a, b in zip(run["acc"], ref["acc"])) and run["cnt"] == ref["cnt"]
        _TAPPED[key] = run
    return _TAPPED[key]


def _sampled_kinds(c):
    """The maps a case binds and samples: its flag is set (the albedo's governs the metallic and emissive
    maps too: they are PBR_MATERIAL's) and a step binds it."""
    fl = C.flags_of(c)
    on = {"albedo": fl["albedo"], "bump": fl["bump"], "metallic": fl["albedo"] and fl["metallic"],
          "emissive": fl["albedo"] and fl["emissive"]}
    return [k for k in C.KINDS if on[k] and any(s[k] is not None for s in c["steps"])]


def _rows(run, kind):
    return run["taps"][run["taps"]["map"] == po.TAP_MAPS.index(kind)]


def _seams(rows, what):
    """Seam taps in both axes: the second texel wraps to 0 (x1 <= x0; on a one-texel axis every tap does)."""
    assert rows.size > 0, "%s: no taps" % what
    assert (rows["x1"] <= rows["x0"]).any(), "%s: no tap across the u seam" % what
    assert (rows["y1"] <= rows["y0"]).any(), "%s: no tap across the v seam" % what
    assert (rows["x1"] > rows["x0"]).any() or rows["x0"].max() == 0, "%s: u never inside" % what
    assert (rows["y1"] > rows["y0"]).any() or rows["y0"].max() == 0, "%s: v never inside" % what


_RGBA8 = [(n, s) for n in C.RGBA8_CASES for s in C.STREAMS]


@pytest.mark.parametrize("name,stream", _RGBA8, ids=["%s-%s" % (n, s.split("_")[0]) for n, s in _RGBA8])
def test_rgba8_case_reaches_what_it_is_named_for(name, stream):
    c = C.case(name, stream)
    run = _tapped(name, stream)
    sampled = _sampled_kinds(c)
    total = 0
    for kind in C.KINDS:
        rows = _rows(run, kind)
        total += rows.size
        what = "%s %s %s" % (name, stream, kind)
        if kind not in sampled:
            assert rows.size == 0, "%s: a map that is off or unbound was read" % what
            continue
        _seams(rows, what)
        u, v = rows["u"], rows["v"]
        if name in C.OUTSIDE_UNIT:
            for label, hit in (("u < 0", u < 0), ("u >= 1", u >= 1), ("v < 0", v < 0), ("v >= 1", v >= 1)):
                assert hit.any(), "%s: no tap with %s" % (what, label)
        if name in C.COMPACTED:   # some of them at the bounces late-bounce compaction hands to pt_cont (PT_CONT_BOUNCE = 2)
            assert (rows["bounce"] >= 2).any(), "%s: no tap at a late bounce" % what
        assert rows["bounce"].min() == 0 and rows["bounce"].max() <= 5, what
        if name == "far":
            assert (np.abs(u) >= 2.0 ** 24).any() and (np.abs(v) >= 2.0 ** 24).any(), what
            assert ((np.abs(u) > 1000) & (np.abs(u) < 1003)).any() and ((np.abs(v) > 1000) & (np.abs(v) < 1003)).any(), what
        if name == "stray":
            w, h = C.SIZES[kind]
            with np.errstate(all="ignore"):
                bad_u, bad_v = ~np.isfinite(u * np.float32(w)), ~np.isfinite(v * np.float32(h))
            assert bad_u.any() and bad_v.any(), "%s: no tap at a non-finite coordinate" % what
            assert (rows["x0"][bad_u] == 0).all() and (rows["y0"][bad_v] == 0).all(), "%s: the pin to texel 0" % what
            assert np.isnan(u).any() and np.isinf(u).any() and np.isnan(v).any() and np.isinf(v).any(), what
        if name == "one_texel":
            assert not rows["x0"].any() and not rows["x1"].any() and not rows["y0"].any() and not rows["y1"].any()
    assert (total > 0) == bool(sampled)
    assert run["cnt"]["rgba8_taps"] >= 4 * total      # (blue noise, and lookups of unbound samplers, count too)


@pytest.mark.parametrize("name,stream", [(n, s) for n in C.CARD_CASES for s in C.STREAMS if n != "flags_none"],
                         ids=lambda x: x.split("_")[0] if x in C.STREAMS else x)
def test_card_case_maps_decide_the_frame(name, stream):
    """The bytewise complement of the maps changes at least 40 % of the pixels of the three-frame render."""
    c = C.case(name, stream)
    ref, swap = C.reference(name, stream), C.oracle_run(C.swapped(c))
    changed = C.pixels_changed(ref["acc"][-1], swap["acc"][-1])
    assert changed >= 0.40, "%s %s: %.3f" % (name, stream, changed)


def test_sizes_at_33x17_reaches_the_seams_too():
    run = _tapped("sizes", C.STREAMS[1], C.SMALL)
    for kind in C.KINDS:
        _seams(_rows(run, kind), "sizes 33x17 %s" % kind)
    swap = C.oracle_run(C.swapped(C.case("sizes", C.STREAMS[1], C.SMALL)))
    assert C.pixels_changed(run["acc"][-1], swap["acc"][-1]) >= 0.40


@pytest.mark.parametrize("name", C.ENV_CASES)
def test_environment_case_reaches_the_seams(name):
    stream = C.STREAMS[1]
    c = C.case(name, stream)
    run = _tapped(name, stream)
    rows = _rows(run, "hdr")
    _seams(rows, name)
    h, w = c["hdr"].shape[:2]
    if h <= 5 and name != "env_seam":   # the small environments are read in every row and column
        assert set(rows["x0"]) == set(range(w)) and set(rows["y0"]) == set(range(h))
    if w == 1:
        assert (rows["x1"] <= rows["x0"]).all()
    if h == 1:
        assert (rows["y1"] <= rows["y0"]).all()
    assert run["cnt"]["hdr_taps"] == 4 * rows.size
    if name == "env_seam":   # every path is a primary ray into the environment: one lookup per pixel, at both poles
        assert rows.size == run["cnt"]["paths"]
        assert (rows["v"] < 0.5 / h).any() and (rows["v"] > 1 - 0.5 / h).any()
    swap = C.oracle_run(C.swapped(c))
    changed = C.pixels_changed(run["acc"][-1], swap["acc"][-1])
    assert changed >= 0.40, "%s: %.3f" % (name, changed)


# ------------------------------------------------------------------------------------------ flags and flip

@pytest.mark.parametrize("stream", C.STREAMS)
def test_flags_equalities_on_the_oracle(stream):
    """No flag set with all four maps bound is, bit for bit, the render with no map bound, and reads no map;
    every flag set with the emissive and metallic samplers unbound reads zeros there: the pixels of the
    (1, 1, 0, 0) render."""
    none = C.reference("flags_none", stream)
    bare = C.oracle_run(C.unbound(C.case("flags_none", stream)))
    unb, two = C.reference("flags_unbound", stream), C.reference("flags_1100", stream)
    for i in range(C.FRAMES):
        assert _same_bits(none["acc"][i], bare["acc"][i]).all() and np.array_equal(none["can"][i], bare["can"][i])
        assert _same_bits(unb["acc"][i], two["acc"][i]).all() and np.array_equal(unb["can"][i], two["can"][i])
    assert none["cnt"] == bare["cnt"]
    assert unb["cnt"]["rgba8_taps"] > two["cnt"]["rgba8_taps"]      # the lookups are made, and counted
    # and the flags do something: every subset renders other pixels than the full set
    full = C.reference("sizes", stream)
    for f in C.FLAG_SUBSETS:
        assert C.pixels_changed(full["acc"][-1], C.reference("flags_%d%d%d%d" % f, stream)["acc"][-1]) > 0.05, f


@pytest.mark.parametrize("stream", C.STREAMS)
def test_flip_case_is_the_row_reversed_sizes_case(stream):
    """What the flip case hands the oracle is the sizes case's maps with their rows reversed - odd heights and a
    one-row map among them - and the reversal shows in the frame."""
    flip, sizes = C.case("flip", stream), C.case("sizes", stream)
    assert flip["invert_y"] and not sizes["invert_y"]
    assert sorted(C.SIZES[k][1] for k in C.KINDS) == [1, 3, 5, 29]
    for k in C.KINDS:
        assert np.array_equal(flip["steps"][0][k][::-1], sizes["steps"][0][k])
    assert C.pixels_changed(C.reference("flip", stream)["acc"][-1], C.reference("sizes", stream)["acc"][-1]) > 0.40


def test_rebind_changes_every_size():
    c = C.case("rebind", C.STREAMS[0])
    a, b, last = c["steps"]
    for k in C.KINDS:
        assert a[k].shape != b[k].shape and a[k].shape[0] != b[k].shape[0] and a[k].shape[1] != b[k].shape[1]
    assert last["emissive"] is None and C.flags_of(c)["emissive"] == 1

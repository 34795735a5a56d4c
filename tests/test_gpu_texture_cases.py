"""The texture-sampling cases of tests/texture_cases.py on the device: texBilinear / texBilinearF (csrc/pt_device.h)
under meshHit, shadeStep and envColor (csrc/pt_program.h) on random maps of odd and unequal sizes, one-texel
axes, repeating, far and non-finite UVs, `uses_*` flags against bound and unbound samplers, flipped uploads,
samplers re-bound between draws, and environments of a few texels - on a card that fills most of the frame.
tests/test_texture_cases.py certifies on the CPU oracle that every case reaches the seams and ranges it names,
and pins the oracle's sampler to the specification (tests/tex_ref.py).

Every case is drawn on the timed kernels - the ones the product and the bench run - and compares, with the oracle's
run of the same arrays, the accumulation after each frame as uint32 and the canvas bytes after each frame; in
one-part contexts it is then drawn once more on the counting variants, and that draw's pixels and its whole
counter dictionary, rgba8_taps and hdr_taps in it, are compared too. `stray` alone matches a NaN channel with a NaN channel whatever its payload, and leaves the
canvas out. 96 x 64 (one case 33 x 17), three frames.

Run on an MI355X: python -m pytest tests/test_gpu_texture_cases.py -m gpu
"""
import numpy as np
import pytest

import helpers as H
import texture_cases as C
from test_gpu_parity import BACKENDS

pytestmark = pytest.mark.gpu


def _same(a, b, nan_matches_nan=False):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype != np.float32:
        return a == b
    same = a.view(np.uint32) == b.view(np.uint32)
    return same | (np.isnan(a) & np.isnan(b)) if nan_matches_nan else same


def _report(same):
    pix = ~same.reshape(same.shape[0], same.shape[1], -1).all(-1)
    ys, xs = np.nonzero(pix)
    return "mismatching pixels %d / %d, first (x,y)=%s" % (pix.sum(), pix.size, (int(xs[0]), int(ys[0])) if len(xs) else None)


class _Scene:
    """A case's textures on an engine; draw() renders its frames from a zero history, binding each frame's
    maps first. counting=False draws with the timed kernels, counting=True with the counting variants (other
    instantiations: no any-hit walk, no dead shadow segments, no fused output pass), which fill the counters."""

    def __init__(self, engine, case):
        import babylon_pt as bp
        self.engine, self.case = engine, case
        self.w, self.h = case["size"]
        meta = case["meta"]
        payload = H.texture_payloads(meta, case["mesh"])
        if case["hdr"] is not None:
            payload["hdr"] = case["hdr"]
        self.player = bp.StreamPlayer(engine, meta, H.bluenoise(), payload, self.w, self.h)
        self.raw = list(meta["textures"])
        self.maps = {}

    def _texture(self, kind, m, invert_y):
        """The map as the engine holds it, uploaded once: invert_y hands over the rows reversed and lets the
        upload turn them back."""
        import babylon_pt as bp
        key = (id(m), invert_y)
        if key not in self.maps:
            self.maps[key] = bp.Texture(self.engine, m[::-1] if invert_y else m, invertY=invert_y, name=kind)
        return self.maps[key]

    def draw(self, schedule="megakernel", layout="pairs", steps=None, invert_y=None, counting=False):
        e, player = self.engine, self.player
        steps = self.case["steps"] if steps is None else steps
        invert_y = self.case["invert_y"] if invert_y is None else invert_y
        e.resize_canvas(self.w, self.h)
        zero = np.zeros((self.h, self.w, 4), np.float32)
        for name in ("pathTracingRenderTarget", "screenCopyRenderTarget"):
            player.textures[name].write(zero)
        one_part = e.parts == 1      # (a multi-part context keeps the default schedule and layout)
        if one_part:
            e.set_backend(schedule)
            e.set_bvh_layout(layout)
        if counting:
            e.set_counting(True)
            e.reset_counters()
        got = {"acc": [], "can": []}
        try:
            for i in range(C.FRAMES):
                for kind, sampler in H.PBR_SAMPLERS.items():
                    m = steps[i][kind]
                    if m is None:
                        player.textures.pop(sampler, None)
                    else:
                        player.textures[sampler] = self._texture(kind, m, invert_y)
                player.play_frame(i)
                e.sync()
                got["acc"].append(player.textures["pathTracingRenderTarget"].read())
                got["can"].append(e.read_canvas(self.w, self.h))
            got["used"] = e.bvh_layout_used()
            got["cnt"] = e.counters() if counting else None
        finally:
            if counting:
                e.set_counting(False)
            if one_part:
                e.set_backend("megakernel")
                e.set_bvh_layout("pairs")
        return got

    def dispose(self):
        for t in list(self.maps.values()) + [self.player.textures[raw] for raw in self.raw]:
            t.dispose()
        self.maps = {}


@pytest.fixture(scope="module")
def scenes(engine):
    """The cases' scenes on the session's engine, each built once and kept until the module is done."""
    built = {}

    def get(name, stream, size=C.SIZE):
        key = (name, stream, size)
        if key not in built:
            built[key] = _Scene(engine, C.case(name, stream, size))
        return built[key]

    yield get
    for s in built.values():
        s.dispose()


@pytest.fixture(scope="module")
def two_parts():
    import babylon_pt as bp
    e = bp.Engine(devices=[0, 0])
    yield e
    e.dispose()


def _compare(what, got, ref, layout=None, nan_matches_nan=False, canvas=True):
    if layout is not None:
        assert got["used"] == layout, "%s: walked %s" % (what, got["used"])
    for i in range(C.FRAMES):
        same = _same(ref["acc"][i], got["acc"][i], nan_matches_nan)
        assert same.all(), "%s frame %d accumulation: %s" % (what, i, _report(same))
        if canvas:
            same = _same(ref["can"][i], got["can"][i])
            assert same.all(), "%s frame %d canvas: %s" % (what, i, _report(same))
    if got.get("cnt") is not None:
        assert got["cnt"] == ref["cnt"], "%s counters: %s / %s" % (what, got["cnt"], ref["cnt"])


def _check(scenes, name, stream, schedule="megakernel", layout="pairs", size=C.SIZE):
    """The case drawn twice: on the timed kernels (what the product and the bench run: any-hit walks, dead shadow
    segments, the fused history blend / screenCopy / screenOutput pass), then on the counting variants for the
    counters; accumulation and canvas are compared both times."""
    ref = C.reference(name, stream, size)
    stray = name == "stray"
    scene = scenes(name, stream, size)
    what = "%s %s %s-%s" % (name, stream, schedule, layout)
    got = scene.draw(schedule, layout)
    _compare(what + ", timed kernels", got, ref, layout, nan_matches_nan=stray, canvas=not stray)
    counted = scene.draw(schedule, layout, counting=True)
    assert counted["cnt"] is not None
    _compare(what + ", counting kernels", counted, ref, layout, nan_matches_nan=stray, canvas=not stray)
    return ref, got


_RGBA8 = [(n, s) for n in C.RGBA8_CASES for s in C.STREAMS]
_IDS = ["%s-%s" % (n, s.split("_")[0]) for n, s in _RGBA8]


@pytest.mark.parametrize("name,stream", _RGBA8, ids=_IDS)
def test_rgba8_case_bitexact(scenes, name, stream):
    """Every RGBA8 case on the megakernel with the pairs layout; the extra draws below are on the timed kernels."""
    ref, got = _check(scenes, name, stream)
    scene = scenes(name, stream)
    if name == "stray" and stream.startswith("hdri"):
        nan = np.isnan(ref["acc"][-1]).any(-1).mean()
        assert nan > 0.001, "the oracle's stray frame holds no NaN pixels (%.4f)" % nan
    if name == "flags_none":   # all four maps bound and no flag set: the draw with no map bound, bit for bit
        bare = scene.draw(steps=C.unbound(scene.case)["steps"])
        _compare("flags_none, unbound", bare, got)
        _compare("flags_none, unbound", scene.draw(steps=C.unbound(scene.case)["steps"], counting=True), ref)
    if name == "flip":         # invertY=True of the reversed rows (drawn above) is invertY=False of the rows themselves
        plain = scene.draw(invert_y=False)
        _compare("flip, invertY=False", plain, got)
        _compare("flip, invertY=False", plain, ref, "pairs")
    if name == "rebind":       # and the frames drawn again with the first maps bound again
        again = scene.draw()
        _compare("rebind, second pass", again, ref, "pairs")


@pytest.mark.parametrize("name", C.ENV_CASES)
def test_environment_case_bitexact(scenes, name):
    """Environments of 1 x 1, 1 x 4, 5 x 1, 7 x 5 and 64 x 32 texels (invertY as recorded: odd heights flip), and
    the 7 x 5 one seen across its u seam and both poles."""
    ref, _ = _check(scenes, name, C.STREAMS[1])
    assert ref["cnt"]["hdr_taps"] > 0


_EVERY = [(n, s) for n in ("sizes", "repeat8", "repeat_sizes", "stray") for s in C.STREAMS] + [("env_7x5", C.STREAMS[1])]


@pytest.mark.parametrize("backend", BACKENDS, ids=["-".join(b) for b in BACKENDS])
@pytest.mark.parametrize("name,stream", _EVERY, ids=["%s-%s" % (n, s.split("_")[0]) for n, s in _EVERY])
def test_case_on_every_schedule_and_layout(scenes, name, stream, backend):
    _check(scenes, name, stream, backend[0], backend[1])


@pytest.mark.parametrize("stream", C.STREAMS)
def test_sizes_at_33x17_bitexact(scenes, stream):
    """An odd frame narrower than a wave's row of tiles; the counters include the quad helpers beyond the odd
    edges, which the oracle shades and counts too."""
    _check(scenes, "sizes", stream, size=C.SMALL)


@pytest.mark.parametrize("name,stream", [("sizes", C.STREAMS[0]), ("sizes", C.STREAMS[1]), ("env_1x4", C.STREAMS[1])])
def test_case_in_a_two_part_context(two_parts, name, stream):
    """Two parts on device 0: every part uploads its own copies of the maps and of the environment. (Timed
    kernels only: no other test reads counters from a multi-part context.)"""
    scene = _Scene(two_parts, C.case(name, stream))
    try:
        got = scene.draw()
    finally:
        scene.dispose()
    _compare("%s %s, two parts" % (name, stream), got, C.reference(name, stream))


@pytest.mark.parametrize("stream", C.STREAMS)
@pytest.mark.parametrize("name", ["sizes", "repeat8", "repeat_sizes"])
def test_case_through_late_bounce_compaction(monkeypatch, name, stream):
    """The later bounces' shading in pt_cont (PT_CONT=1, a fresh engine, seven draws with no sync between them:
    tests/test_gpu_compaction.py's scaffold), and records really went through it. tests/test_texture_cases.py
    certifies from the tap log that these cases read every map at bounces >= 2, the ones pt_cont takes over."""
    import test_gpu_compaction as GC
    c = C.case(name, stream)
    w, h = c["size"]
    rep, _ = GC._run(monkeypatch, "texture-%s-%s" % (name, stream), c["meta"], w, h, mesh=c["mesh"], maps=c["steps"][0])
    assert rep["layout"] == "pairs"
    GC._assert_compacted(rep, w, h)

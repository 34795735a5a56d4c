"""The render loop's fused pass (PT_FUSE_BLEND; csrc/pt_plan.h MainPlan, pt_output_f1): a megakernel
draw's history blend waits for the loop's screenCopy and screenOutput and runs folded into the output pass, which
reads the history from one of the loop's two textures, writes the accumulation to the other and leaves the first
one stale until something has to see it.

Every case is a script of draws and reads played on the GPU and on a two-buffer model that runs the oracle's
path tracing, blend, copy and screenOutput eagerly; every read is compared bit for bit. pt_fuse_stats then shows
that the fused pass really ran (or, for the cases where it must stay off, that it did not) and how many screenCopy
kernels the reads forced.

Script letters: T path tracing (the next frame's uniforms) | C screenCopy | O screenOutput into the canvas |
F screenOutput into an RGBA32F target | a / b / c read the accumulation target / the copy target / the canvas |
f read the RGBA32F target | R resize both targets (and the canvas) to the case's second size | A / B destroy the
accumulation target / the copy target and put a new, zeroed one in its place.

Run on an MI355X: python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest
import torch   # loaded before libpt.so, as in tests/test_gpu_denoise.py: the caller-memory case needs both on one HIP runtime

import helpers as H

pytestmark = pytest.mark.gpu

ACC, COPY = "pathTracingRenderTarget", "screenCopyRenderTarget"
LOOP = "TCO"


def _bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def _frames(meta, n, moving=()):
    """n frames of the loop from a cleared history: uFrameCounter 1 (the history rule of frame 1), 2, ...; the
    camera moves on the frames in `moving` (history and sample halved, the sample counter back at 1)."""
    import babylon_pt as bp
    base = meta["frames"][0]
    frames, sample = [], 0
    for k in range(n):
        mv = k in moving
        sample = 1 if mv else sample + 1
        calls = []
        for c in base:
            u = dict(c["uniforms"])
            if c["shader"] == "pathTracingFragmentShader":
                u["uFrameCounter"] = ["f", [float(k + 1)]]
                u["uSampleCounter"] = ["f", [float(sample)]]
                u["uCameraIsMoving"] = ["i", [1 if mv else 0]]
                u["uRandomVec2"] = ["f", bp.splitmix64_uniforms(4242 * 1000003 + k, 2)]
            if "uOneOverSampleCounter" in u:
                u["uOneOverSampleCounter"] = ["f", [1.0 / sample]]
            calls.append(dict(c, uniforms=u))
        frames.append(calls)
    return frames


class _Model:
    """The loop's two textures and the canvas with every pass performed at once, by the oracle."""

    def __init__(self, meta, w, h, mesh=None):
        self.meta, self.mesh = meta, mesh
        self.resize(w, h)
        self.can = self.f32 = None

    def resize(self, w, h):
        self.w, self.h = w, h
        self.scene = H.oracle_scene(self.meta, w, h, self.mesh)
        self.a = np.zeros((h, w, 4), np.float32)
        self.b = np.zeros((h, w, 4), np.float32)

    def trace(self, calls):
        self.a, _ = self.scene.path_trace(H.with_resolution(H.path_call(calls)["uniforms"], self.w, self.h), self.b.copy())

    def output(self, calls, f32=False):
        import ptoracle as po
        ou = H.output_call(calls)["uniforms"]
        inv, exp = ou["uOneOverSampleCounter"][1][0], ou.get("uToneMappingExposure", ["f", [0.0]])[1][0]
        if f32:
            self.f32 = po.screen_output_f32(self.a, inv, exp)
        else:
            self.can = po.screen_output(self.a, inv, exp)


def _payload(meta, mesh=None):
    if meta["scene"] not in ("gltf", "hdri", "skymesh"):
        return None
    return H.texture_payloads(meta, mesh if mesh is not None else H.mesh(meta))


def _play(e, meta, script, w, h, frames, mesh=None, canvas=None, second=None, rt_ptrs=None, read_rt=None, payload=None):
    """Plays `script` on engine `e` and on the model; returns pt_fuse_stats' two counts, as this script moved them,
    at every 's' in the script and at its end. `canvas`: a canvas of another size than the frame (the model's canvas
    is then cropped to it). `read_rt`: how to read a render target (default: through the API)."""
    import babylon_pt as bp
    model = _Model(meta, w, h, mesh)
    player = bp.StreamPlayer(e, meta, H.bluenoise(), payload if payload is not None else _payload(meta, mesh), w, h,
                             rt_ptrs=rt_ptrs)
    cw, ch = canvas or (w, h)
    e.resize_canvas(cw, ch)
    read_rt = read_rt or (lambda name: player.textures[name].read())
    f0 = e.fuse_stats()
    marks = []

    def stats():
        f = e.fuse_stats()
        return f[0] - f0[0], f[1] - f0[1]

    try:
        return _steps(e, meta, script, frames, model, player, cw, ch, second, read_rt, stats, marks)
    finally:   # (the player's textures go with the case; what was deferred for them runs first)
        for t in player.textures.values():
            t.dispose()


def _steps(e, meta, script, frames, model, player, cw, ch, second, read_rt, stats, marks):
    import babylon_pt as bp
    k, calls = -1, None
    for pos, op in enumerate(script):
        where = "%r step %d (%s), frame %d" % (script, pos, op, k)
        if op == "T":
            k += 1
            calls = frames[k]
            player.play_call(H.path_call(calls))
            model.trace(calls)
        elif op == "C":
            player.play_call(calls[1])
            model.b = model.a.copy()
        elif op == "O":
            player.play_call(H.output_call(calls))
            model.output(calls)
        elif op == "F":
            if "outputF32" not in player.textures:
                player.textures["outputF32"] = bp.RenderTargetTexture("outputF32", (model.w, model.h), e)
            player.play_call(dict(H.output_call(calls), target="outputF32"))
            model.output(calls, f32=True)
        elif op == "a":
            assert _bits_equal(model.a, read_rt(ACC)), "accumulation target at " + where
        elif op == "b":
            assert _bits_equal(model.b, read_rt(COPY)), "copy target at " + where
        elif op == "c":
            assert _bits_equal(model.can[:ch, :cw], e.read_canvas(cw, ch)), "canvas at " + where
        elif op == "f":
            assert _bits_equal(model.f32, player.textures["outputF32"].read()), "RGBA32F output at " + where
        elif op == "R":
            w2, h2 = second
            for name in (ACC, COPY):
                player.textures[name].resize((w2, h2))
            e.resize_canvas(w2, h2)
            cw, ch = w2, h2
            player.width, player.height = w2, h2
            vlen = bp.path_uniform(meta["frames"][0], "uVLen")
            player.override = {"uResolution": ["f", [float(w2), float(h2)]], "uULen": ["f", [vlen * (w2 / h2)]]}
            model.resize(w2, h2)
        elif op in "AB":
            name = ACC if op == "A" else COPY
            player.textures[name].dispose()
            player.textures[name] = bp.RenderTargetTexture(name, (model.w, model.h), e)
            if op == "A":
                model.a = np.zeros_like(model.a)
            else:
                model.b = np.zeros_like(model.b)
        elif op == "s":
            marks.append(stats())
        else:
            raise ValueError(op)
    marks.append(stats())
    return marks


@pytest.fixture(scope="module")
def teapot():
    meta = H.stream("gltf_teapot_320x180")
    return meta, _frames(meta, 6, moving=(3, 4)), _payload(meta)


@pytest.fixture(scope="module")
def eng():
    """One engine with the default knobs for the cases that need nothing else."""
    import babylon_pt as bp
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("PT_")}
    e = bp.Engine(0)
    os.environ.update(saved)
    yield e
    e.dispose()


@pytest.fixture
def fresh(monkeypatch):
    """fresh(env, devices) -> an engine of its own, created under exactly the PT_* variables in `env`."""
    import babylon_pt as bp
    made = []

    def make(env=None, devices=None):
        for k in list(os.environ):
            if k.startswith("PT_"):
                monkeypatch.delenv(k)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        made.append(bp.Engine(0) if devices is None else bp.Engine(devices=devices))
        return made[-1]
    yield make
    for e in made:
        e.dispose()


# ------------------------------------------------------------------ the loop, every frame observed

@pytest.mark.parametrize("w,h", [(96, 64), (33, 17), (48, 40)])
def test_six_frames_every_texture_after_every_frame(eng, teapot, w, h):
    """Frame 1's history rule, two still frames, two moving-camera frames, a still one; 33x17: partial tiles on
    both axes, the halo at the texture's edges; 48x40: several tiles and bands. After every frame the canvas and
    both textures are read: every frame fused, and each frame's reads brought its one stale texture up to date."""
    meta, frames, payload = teapot
    (fused, stale), = _play(eng, meta, (LOOP + "cab") * 6, w, h, frames, payload=payload)
    assert (fused, stale) == (6, 6)


def test_steady_loop_never_copies(eng, teapot):
    """No read between the frames: six fused passes and no screenCopy kernel; the reads at the end run one."""
    meta, frames, payload = teapot
    loop, end = _play(eng, meta, LOOP * 6 + "s" + "cba", 96, 64, frames, payload=payload)
    assert loop == (6, 0)
    assert end == (6, 1)


# ------------------------------------------------------------------ interleavings

@pytest.mark.parametrize("script,want", [
    # (fused passes, screenCopy kernels run alone), worked out by hand from the rules in pt_plan.h:
    # a read of either texture after the trace: the frame takes pt_blend, which overwrites the stale target, and
    # its copy rides along with the output; the one copy is the last frame's stale texture, for the reads at the end
    (LOOP * 2 + "TaCOcab" + LOOP + "cab", (3, 1)),
    (LOOP * 2 + "TbCOcab" + LOOP + "cab", (3, 1)),
    (LOOP * 2 + "TbaCOcab", (2, 0)),
    # ... after the copy: pt_blend and that copy alone, then the last frame's
    (LOOP * 2 + "TCaOcab" + LOOP + "cab", (3, 2)),
    (LOOP * 2 + "TCbOcab" + LOOP + "cab", (3, 2)),
    # ... after the output: the stale texture's copy, once per frame that is read
    (LOOP * 3 + "a" + LOOP + "b" + LOOP + "cab", (5, 3)),
    # two traces in a row: the first one's pt_blend needs its stale previousBuffer copied first (the second trace
    # reads it too: its frame's copy never came)
    (LOOP + "TTCOcab" + LOOP + "cab", (3, 3)),
    ("TTCOcab", (1, 1)),
    # screenOutput into a float render target takes the blend along too; a second output of the frame is plain,
    # and the copy rides along with it
    (LOOP + "TCFfab" + "TCFOfcab", (3, 1)),
])
def test_interleavings(eng, teapot, script, want):
    meta, frames, payload = teapot
    (got,) = _play(eng, meta, script, 96, 64, frames, payload=payload)
    assert got == want


def test_canvas_of_another_size_does_not_fuse(eng, teapot):
    """The output pass covers other pixels than the blend: pt_blend, and the copy alone (no fused pass, no stale
    texture, so no screenCopy kernel counted as forced by a read... but each frame's own)."""
    meta, frames, payload = teapot
    (got,) = _play(eng, meta, LOOP * 3 + "cab", 96, 64, frames, payload=payload, canvas=(48, 32))
    assert got == (0, 3)


def test_resize_mid_stream(eng, teapot):
    """Both targets resized with a stale texture pending: the loop goes on from a zero history at 48x40."""
    meta, frames, payload = teapot
    (got,) = _play(eng, meta, LOOP * 2 + "R" + LOOP * 2 + "cab", 96, 64, frames, payload=payload, second=(48, 40))
    assert got == (4, 2)


@pytest.mark.parametrize("script,want", [
    (LOOP * 2 + "Ba" + LOOP * 2 + "cab", (4, 2)),   # after two frames the copy target is the fresh one: its copy runs first
    (LOOP + "Ba" + LOOP * 2 + "cab", (3, 2)),       # after one, the stale one
    (LOOP * 2 + "Ab" + LOOP * 2 + "cab", (4, 2)),
    (LOOP + "Ab" + LOOP * 2 + "cab", (3, 2)),
])
def test_destroying_either_texture(eng, teapot, script, want):
    meta, frames, payload = teapot
    (got,) = _play(eng, meta, script, 96, 64, frames, payload=payload)
    assert got == want


def test_knob_off_is_the_two_passes(fresh, teapot):
    meta, frames, payload = teapot
    e = fresh({"PT_FUSE_BLEND": "0"})
    (got,) = _play(e, meta, (LOOP + "cab") * 6, 96, 64, frames, payload=payload)
    assert got == (0, 0)   # (each frame's copy rode along with its output, as ever)


# ------------------------------------------------------------------ where it must stay off

def test_four_wave_workgroups_keep_the_two_passes(fresh, teapot):
    """PT_MAIN_WAVES=0: the main stream's passes as 256-thread workgroups; the fused pass has no such form."""
    meta, frames, payload = teapot
    e = fresh({"PT_MAIN_WAVES": "0"})
    (got,) = _play(e, meta, (LOOP + "cab") * 3, 96, 64, frames, payload=payload)
    assert got == (0, 0)


@pytest.mark.parametrize("w,h,fused", [(2048, 1024, 2), (2048, 1025, 0)])
def test_the_threshold_of_8192_tiles(eng, teapot, w, h, fused):
    """128 x 64 tiles: the largest frame the fused pass takes; one more row of tiles: the two passes (256-thread
    workgroups, where the fused pass lost)."""
    meta, frames, payload = teapot
    (got,) = _play(eng, meta, LOOP * 2 + "cab", w, h, frames, payload=payload)
    assert got == (fused, 1 if fused else 0)


def test_caller_provided_memory_is_always_current(eng, teapot):
    """Render targets over the caller's memory: read straight from that memory after a sync, never fused."""
    meta, frames, payload = teapot
    w, h = 96, 64
    mem = {n: torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for n in (ACC, COPY)}

    torch.cuda.synchronize()

    def read(name):
        eng.sync()
        return mem[name].cpu().numpy()

    (got,) = _play(eng, meta, (LOOP + "ab") * 3 + "c", w, h, frames, payload=payload,
                   rt_ptrs={n: t.data_ptr() for n, t in mem.items()}, read_rt=read)
    assert got == (0, 0)


def test_two_parts_on_one_device(fresh, teapot):
    meta, frames, payload = teapot
    e = fresh(devices=[0, 0])
    (got,) = _play(e, meta, (LOOP + "cab") * 3, 96, 64, frames, payload=payload)
    assert got[0] == 0


def test_row_partition_with_output_partition(eng, teapot):
    """Two partitions traced into the same targets on one context, the output band by band: the parent's passes."""
    import babylon_pt as bp
    meta, frames, payload = teapot
    w, h = 96, 64
    model = _Model(meta, w, h)
    player = bp.StreamPlayer(eng, meta, H.bluenoise(), payload, w, h)
    eng.resize_canvas(w, h)
    fused0 = eng.fuse_stats()[0]
    try:
        for calls in frames[:3]:
            for p in range(2):
                eng.set_row_partition(2, p)
                player.play_call(calls[0])
            eng.set_row_partition(1, 0)
            player.play_call(calls[1])
            eng.set_output_partition(True)
            for p in range(2):
                eng.set_row_partition(2, p)
                player.play_call(calls[2])
            eng.set_output_partition(False)
            eng.set_row_partition(1, 0)
            model.trace(calls)
            model.b = model.a.copy()
            model.output(calls)
            assert _bits_equal(model.can, eng.read_canvas(w, h))
            assert _bits_equal(model.a, player.textures[ACC].read())
            assert _bits_equal(model.b, player.textures[COPY].read())
    finally:
        eng.set_output_partition(False)
        eng.set_row_partition(1, 0)
    assert eng.fuse_stats()[0] == fused0
    for t in player.textures.values():
        t.dispose()


# ------------------------------------------------------------------ compaction and the buffer sets' counters

def test_compacting_schedule_twelve_frames(fresh):
    """The flagship's schedule (three frames in flight, no lag, compaction on, the record sort) at 256x144 with
    every wave handing its paths on (PT_CONT_LANES=64), twelve frames: every buffer set is reused, and the fused
    pass has taken over the record counter's reset and total from pt_blend."""
    meta = H.stream("gltf_bunny_1080p")
    mesh = H.synthetic_dragon(64, 64)
    frames = _frames(meta, 12)
    e = fresh({"PT_CONT": "1", "PT_OVERLAP_LAG": "0", "PT_CONT_LANES": "64"})
    (got,) = _play(e, meta, LOOP * 12 + "cab", 256, 144, frames, mesh=mesh)
    assert got == (12, 1)
    stored, launched = e.cont_stats()
    qs = e.queue_stats()
    assert qs["late_bounce_compaction"] == "on" and qs["frames_in_flight"] == 3, qs
    assert launched == 12 and 0 < stored <= 256 * 144 * 12, (stored, launched)

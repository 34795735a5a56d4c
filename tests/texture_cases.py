"""The texture-sampling cases (test infrastructure, host only): small random maps of odd and unequal sizes,
one-texel axes, UVs that repeat, lie far from 0 or are not finite, `uses_*` flags against bound and unbound
samplers, flipped uploads, re-bound samplers, and small environments - drawn over the helmet streams on a
card that fills most of the frame. tests/test_texture_cases.py certifies on the CPU oracle, from its tap log,
that every case reaches the seams and the UV ranges it is named for; tests/test_gpu_texture_cases.py draws the
same cases on the device.

A case is a dict:
    name, stream, size (W, H)
    meta     the recorded stream, cut to FRAMES frames, with the case's uniforms edited in
    mesh     {"bvh", "tri"}: the card or the helmet with its UV columns edited
    steps    one dict per frame: {kind: (h, w, 4) uint8 map, or None for an unbound sampler}, in the row
             order the oracle reads (row 0 is v = 0)
    invert_y the engine uploads `steps`' maps reversed in their rows with invertY=True (the same texels)
    hdr      None (the stream's synthetic environment) or the (h, w, 4) float32 payload as the setup script
             uploads it (invertY as the stream records it)
"""
import contextlib

import numpy as np

import helpers as H
import tree_shapes as T

FRAMES = 3
SIZE = (96, 64)
SMALL = (33, 17)
STREAMS = ("gltf_helmet_320x180", "hdri_helmet_320x180")
KINDS = ("albedo", "bump", "metallic", "emissive")
FLAG = {"albedo": "uModelUsesAlbedoTexture", "bump": "uModelUsesBumpTexture",
        "metallic": "uModelUsesMetallicTexture", "emissive": "uModelUsesEmissiveTexture"}
# W x H
SIZES = {"albedo": (37, 29), "bump": (64, 1), "metallic": (1, 5), "emissive": (3, 3)}
OTHER_SIZES = {"albedo": (5, 12), "bump": (3, 7), "metallic": (16, 9), "emissive": (2, 31)}
EIGHT = {k: (8, 8) for k in KINDS}
ONE = {k: (1, 1) for k in KINDS}


# ------------------------------------------------------------------------------------------ maps

def random_map(kind, w, h, seed):
    """Seeded random bytes, (h, w, 4). CalculateRadiance reads the emissive and the metallic-roughness maps
    through thresholds (a first-bounce texel brighter than 0.01 after pow 2.2 - a byte above 31 - ends the path
    with the emission; .g and .b above it choose clear coat and metal), so all-random bytes would end every
    path at the emissive tap and never read the metallic map. A seeded half of the emissive texels is
    therefore dim (bytes 0 .. 31: the path goes on, the metallic map is read), and a seeded third each of the
    metallic texels is diffuse (.g, .b dim), clear coat (.b dim) and metal."""
    rng = np.random.default_rng([seed, w, h, KINDS.index(kind)])
    m = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    dim = rng.integers(0, 32, (h, w, 4), dtype=np.uint8)
    if kind == "emissive":
        pick = rng.permutation(w * h).reshape(h, w) % 2 == 0
        m[pick, :3] = dim[pick, :3]
    if kind == "metallic":
        zone = rng.permutation(w * h).reshape(h, w) % 3
        m[zone == 0, 1:3] = dim[zone == 0, 1:3]
        m[zone == 1, 2] = dim[zone == 1, 2]
    return m


def random_maps(sizes, seed=11):
    return {k: random_map(k, sizes[k][0], sizes[k][1], seed) for k in KINDS}


def complement(maps):
    """Every byte of every map (or of an environment's floats) inverted."""
    if isinstance(maps, dict):
        return {k: (None if m is None else complement(m)) for k, m in maps.items()}
    m = np.ascontiguousarray(maps)
    return (~m.view(np.uint8)).view(m.dtype)


def random_env(w, h, seed=5):
    """Seeded random floats in [1/16, 4), alpha 1, in upload order (h, w, 4)."""
    rng = np.random.default_rng([seed, w, h])
    e = (0.0625 + rng.random((h, w, 4)) * 3.9375).astype(np.float32)
    e[..., 3] = 1.0
    return e


# ------------------------------------------------------------------------------------------ streams

def _path_uniforms(meta):
    return H.path_call(meta["frames"][0])["uniforms"]


def edited(meta, **uniforms):
    """The stream's first FRAMES frames with path-tracing uniforms replaced: name=[kind, values]."""
    frames = []
    for f in meta["frames"][:FRAMES]:
        fr = []
        for c in f:
            if c["shader"] == "pathTracingFragmentShader":
                c = dict(c, uniforms=dict(c["uniforms"], **uniforms))
            fr.append(c)
        frames.append(fr)
    return dict(meta, frames=frames)


def with_flags(meta, flags):
    return edited(meta, **{FLAG[k]: ["i", [int(f)]] for k, f in zip(KINDS, flags)})


# ------------------------------------------------------------------------------------------ the card

GRID = (4, 3)          # cells across, cells up: every cell two triangles with UVs of its own
CARD_FILL = 0.9        # of the view's half extents
# The card cases' camera: the streams' own, moved into the mouth of the room (its walls lie 50 about the origin),
# and the card 55 in front of it, between the side walls at either frame size and above the two spheres. It
# faces the camera and, in the glTF scene, the quad light on the ceiling, so its diffuse texels are lit, not
# black; the HDRI scene's sun is turned to shine in through the mouth of the room for the same reason (the
# recorded one lies in the card's plane).
CARD_CAMERA = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -45.0, 1.0]
CARD_DISTANCE = 55.0
CARD_SUN = [0.35, 0.5, -0.7921489759887339]


def card(meta, size, cell_uv):
    """A camera-facing card of GRID cells in the stream's first camera at `size`, CARD_FILL of the view each
    way (about 0.8 of the pixels), as triangle records in the model's space with a balanced tree.
    cell_uv(i, j) -> (u0, u1, v0, v1): the cell's UVs run linearly from (u0, v0) at its lower left corner to
    (u1, v1) at its upper right one."""
    u = _path_uniforms(meta)
    w, h = size
    cam = np.array(u["uCameraMatrix"][1], np.float64)
    right, up, fwd, pos = cam[0:3], cam[4:7], cam[8:11], cam[12:15]
    vlen = u["uVLen"][1][0]
    ulen = vlen * (w / h)
    inv = np.array(u["uGLTF_Model_InvMatrix"][1], np.float64).reshape(4, 4).T     # world -> model
    hx, hy = CARD_FILL * ulen * CARD_DISTANCE, CARD_FILL * vlen * CARD_DISTANCE
    centre = pos + fwd * CARD_DISTANCE

    def to_model(p):
        return (inv @ np.append(p, 1.0))[:3]

    nrm = inv[:3, :3] @ (-fwd)
    gx, gy = GRID
    tris = []
    for j in range(gy):
        for i in range(gx):
            u0, u1, v0, v1 = cell_uv(i, j)
            x0, x1 = -hx + 2 * hx * i / gx, -hx + 2 * hx * (i + 1) / gx
            y0, y1 = -hy + 2 * hy * j / gy, -hy + 2 * hy * (j + 1) / gy
            corner = {(a, b): (to_model(centre + right * x + up * y), (uu, vv))
                      for a, x, uu in ((0, x0, u0), (1, x1, u1)) for b, y, vv in ((0, y0, v0), (1, y1, v1))}
            for tri in (((0, 0), (1, 0), (1, 1)), ((0, 0), (1, 1), (0, 1))):
                p = np.stack([corner[c][0] for c in tri])
                if np.dot(np.cross(p[1] - p[0], p[2] - p[0]), nrm) < 0:    # front face towards the camera
                    tri = tri[::-1]
                rec = np.zeros(32, np.float32)
                rec[0:9] = np.concatenate([corner[c][0] for c in tri])
                rec[9:18] = np.tile(nrm, 3)
                rec[18:24] = np.concatenate([corner[c][1] for c in tri])
                tris.append(rec)
    return T.shaped_tree(np.stack(tris), T.balanced)


def linear_uv(lo, hi):
    """UVs linear over [lo, hi] across the whole card, both axes."""
    gx, gy = GRID
    span = hi - lo
    return lambda i, j: (lo + span * i / gx, lo + span * (i + 1) / gx, lo + span * j / gy, lo + span * (j + 1) / gy)


FAR_BASES = (1000.25, -1000.25, 16777216.0, -16777216.0)


def far_uv(i, j):
    """Every cell near one of FAR_BASES in u and another in v: 1.75 periods wide near +-1000.25 (the seams are
    crossed), 64 wide at +-2^24, where float32 holds whole numbers only, u * w - 0.5 has no fraction left and
    fmodf is exact on the large argument."""
    def span(base):
        return (base, base + (1.75 if abs(base) < 2000 else 64.0 if base > 0 else -64.0))
    bu, bv = FAR_BASES[i % 4], FAR_BASES[(i + j + 1) % 4]
    return span(bu) + span(bv)


# ------------------------------------------------------------------------------------------ the helmet

STRAY_VALUES = (np.nan, np.inf, -np.inf, 3e38, -3e38, -0.0, 1e-45)
STRAY_EVERY = 29
# the stray case's camera: the streams' own, moved up to the helmet, which then covers a third of a 96 x 64 frame
STRAY_CAMERA = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -40.0, 1.0]


def helmet():
    return H.mesh("helmet")


def stray_helmet():
    """The helmet with one UV component of every 29th triangle replaced: the values and the six components
    in turn (7 and 6 are coprime, so every value meets every component)."""
    m = helmet()
    tri = m["tri"].copy()
    for n, t in enumerate(range(0, tri.shape[0], STRAY_EVERY)):
        tri[t, 18 + n % 6] = np.float32(STRAY_VALUES[n % len(STRAY_VALUES)])
    return {"bvh": m["bvh"], "tri": tri}


# a camera at the recorded place that looks back along -z, with a view wide enough for both poles: primary rays
# leave the room, cross the environment's u seam (the -z meridian) and come within a few degrees of +-y
SEAM_CAMERA = [-1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, -200.0, 1.0]
SEAM_VLEN = 8.0


# ------------------------------------------------------------------------------------------ the cases

FLAG_SUBSETS = ((1, 0, 0, 0), (1, 1, 0, 0), (1, 0, 1, 0), (1, 0, 0, 1), (0, 1, 0, 0))
ENV_SIZES = ((1, 1), (1, 4), (5, 1), (7, 5), (64, 32))

RGBA8_CASES = ("sizes", "one_texel", "repeat8", "repeat_sizes", "far", "stray", "flip", "rebind", "flags_none",
               "flags_unbound") + tuple("flags_%d%d%d%d" % f for f in FLAG_SUBSETS)
ENV_CASES = tuple("env_%dx%d" % s for s in ENV_SIZES) + ("env_seam",)
# the cases drawn on a card (the coverage bound applies), and the UV ranges a case is named for
CARD_CASES = tuple(c for c in RGBA8_CASES if c != "stray")
OUTSIDE_UNIT = ("repeat8", "repeat_sizes", "far", "stray")
# the cases the GPU file also draws with late-bounce compaction forced: their maps are read at bounces >= 2 too
COMPACTED = ("sizes", "repeat8", "repeat_sizes")

_CASES = {}


def _steps(maps):
    return [maps] * FRAMES


def _build(name, stream, size):
    meta = edited(H.stream(stream))
    case = {"name": name, "stream": stream, "size": size, "invert_y": False, "hdr": None}
    sizes_maps = random_maps(SIZES)
    if name in ENV_CASES:
        assert stream == "hdri_helmet_320x180"
        w, h = (7, 5) if name == "env_seam" else tuple(int(x) for x in name[4:].split("x"))
        if name == "env_seam":
            meta = edited(meta, uCameraMatrix=["f", list(SEAM_CAMERA)], uVLen=["f", [SEAM_VLEN]])
        meta = dict(meta, hdr=dict(meta["hdr"], width=w, height=h, generator="random_env", sha256=None))
        return dict(case, meta=meta, mesh=helmet(), hdr=random_env(w, h), steps=_steps(H.synthetic_pbr_maps(16)))
    if name == "stray":
        meta = edited(meta, uCameraMatrix=["f", list(STRAY_CAMERA)])
        return dict(case, meta=meta, mesh=stray_helmet(), steps=_steps(sizes_maps))
    meta = edited(meta, uCameraMatrix=["f", list(CARD_CAMERA)])
    if meta["scene"] == "hdri":
        meta = edited(meta, uSunDirection=["f", list(CARD_SUN)])
    uv = {"repeat8": linear_uv(-2.5, 3.5), "repeat_sizes": linear_uv(-2.5, 3.5), "far": far_uv}.get(name, linear_uv(0.0, 1.0))
    case["mesh"] = card(meta, size, uv)
    if name == "one_texel":
        steps = _steps(random_maps(ONE))
    elif name == "repeat8":
        steps = _steps(random_maps(EIGHT))
    elif name == "rebind":
        steps = [sizes_maps, random_maps(OTHER_SIZES, seed=12), dict(random_maps(OTHER_SIZES, seed=12), emissive=None)]
    elif name == "flags_unbound":
        steps = _steps(dict(sizes_maps, emissive=None, metallic=None))
    else:
        steps = _steps(sizes_maps)
    if name == "flip":
        case["invert_y"] = True
        steps = _steps({k: np.ascontiguousarray(m[::-1]) for k, m in sizes_maps.items()})
    if name == "flags_none":
        meta = with_flags(meta, (0, 0, 0, 0))
    elif name.startswith("flags_") and name != "flags_unbound":
        meta = with_flags(meta, tuple(int(c) for c in name[6:]))
        if name == "flags_0100":   # no albedo map: the model's own material, here diffuse, so that the normal shows
            meta = edited(meta, uModelMaterialType=["i", [1]])
    return dict(case, meta=meta, steps=steps)


def case(name, stream, size=SIZE):
    key = (name, stream, size)
    if key not in _CASES:
        _CASES[key] = _build(name, stream, size)
    return _CASES[key]


def unbound(c):
    """The case with no PBR sampler bound."""
    return dict(c, steps=_steps({k: None for k in KINDS}))


def swapped(c):
    """The case with every map, or its environment, replaced by its bytewise complement."""
    if c["hdr"] is not None:
        return dict(c, hdr=complement(c["hdr"]))
    return dict(c, steps=[complement(s) for s in c["steps"]])


def flags_of(c):
    u = _path_uniforms(c["meta"])
    return {k: int(u[FLAG[k]][1][0]) for k in KINDS}


# ------------------------------------------------------------------------------------------ the oracle's run

TAP_CAPACITY = 1 << 18

_REF = {}


def oracle_run(c, taps=False):
    """The oracle over the case from a zero history: {"acc": [after each frame], "can": [canvases], "cnt":
    counter totals}, and with taps=True (one thread, the tap log bound) "taps": the log's rows and "dropped"."""
    import ptoracle as po
    meta, (w, h) = c["meta"], c["size"]
    acc = np.zeros((h, w, 4), np.float32)
    out = {"acc": [], "can": [], "cnt": {}}
    log = po.TapLog(TAP_CAPACITY if taps else 0)
    hdr = c["hdr"] if c["hdr"] is not None else (H.synthetic_hdr() if meta["scene"] == "hdri" else None)
    with log if taps else contextlib.nullcontext():
        for f, maps in zip(meta["frames"], c["steps"]):
            sc = po.Scene(meta["scene"], w, h, H.bluenoise(), c["mesh"]["bvh"], c["mesh"]["tri"], hdr,
                          {k: m for k, m in maps.items() if m is not None})
            acc, cnt = sc.path_trace(H.with_resolution(H.path_call(f)["uniforms"], w, h), acc, nthreads=1 if taps else 0)
            out["acc"].append(acc.copy())
            for k, v in cnt.items():
                out["cnt"][k] = out["cnt"].get(k, 0) + v
            ou = H.output_call(f)["uniforms"]
            out["can"].append(po.screen_output(acc, ou["uOneOverSampleCounter"][1][0],
                                               ou.get("uToneMappingExposure", ["f", [0.0]])[1][0]))
    if taps:
        out["taps"], out["dropped"] = log.rows.copy(), log.dropped
    return out


def reference(name, stream, size=SIZE):
    """oracle_run of a named case, once."""
    key = (name, stream, size)
    if key not in _REF:
        _REF[key] = oracle_run(case(name, stream, size))
    return _REF[key]


def pixels_changed(a, b):
    """The fraction of pixels whose RGBA32F bits differ between two accumulations."""
    return float((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(-1).mean())

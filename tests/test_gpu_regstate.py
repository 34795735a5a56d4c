"""The 8-wave child-pair kernels' register state (pt_trace / pt_cont of the texture-free mesh programs): the path's
small integers and flags carried across a BVH walk as one word (pt_pathstate.h), the wave's placement kept
wave-uniform with the lane's pixel and slab index re-formed from the lane id, the analytic winner's object-space
normal recomputed after the walk, pt_cont's state kept as the record's word between bounces. None of it may change a
bit: every case is bit-exact against the CPU oracle (accumulation as uint32, canvas bytes) on the scaffold of
tests/test_gpu_compaction.py, at 96x64 and at 33x17 (odd edges, quad helpers, a last band of one row) for the
glTF, HDRI and sky + mesh programs.

Run on an MI355X: python -m pytest tests/test_gpu_regstate.py -m gpu
"""
import numpy as np
import pytest

import helpers as H
import test_gpu_compaction as C
from helpers import _with_material

pytestmark = pytest.mark.gpu

SIZES = [(96, 64), (33, 17)]
SIZE_IDS = ["%dx%d" % s for s in SIZES]
PROGRAMS = ("gltf", "hdri", "skymesh")
METAL = 3


def _scene(program, material):
    """(oracle cache key, stream, mesh) of a texture-free mesh program with the model's material set."""
    if program == "gltf":
        return "rs-gltf-m%d" % material, _with_material(H.stream("gltf_teapot_320x180"), material), None
    if program == "hdri":
        return "rs-hdri-m%d" % material, _with_material(H.stream("hdri_teapot_320x180"), material), None
    return "rs-sky-m%d" % material, H.sky_mesh_stream(material), C._small_dragon()


def _case(monkeypatch, program, material, size, cont, layout="pairs", env=None, parts=1):
    key, meta, mesh = _scene(program, material)
    W, Hh = size
    env = dict(env or {}, PT_CONT="1" if cont else "0")
    rep, ref = C._run(monkeypatch, key, meta, W, Hh, env=env, mesh=mesh, layout=layout, parts=parts)
    assert rep["layout"] == layout
    return rep, ref


def _assert_cont(rep, size, cont, bands=1):
    """Compaction on: records went through pt_cont in every still draw; off: none was ever stored."""
    if cont:
        C._assert_compacted(rep, size[0], size[1], bands=bands)
    else:
        assert rep["cs"] == (0, 0) and rep["qs"]["late_bounce_compaction"] == "off", (rep["cs"], rep["qs"])


@pytest.mark.parametrize("layout", ["pairs", "trail"])
@pytest.mark.parametrize("cont", [True, False], ids=["cont", "nocont"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("program", PROGRAMS)
def test_programs_sizes_walks(monkeypatch, program, size, cont, layout):
    """Every program (Metal model) at both sizes, compaction forced on and off, on the stack walk and the trail walk."""
    rep, _ = _case(monkeypatch, program, METAL, size, cont, layout)
    _assert_cont(rep, size, cont)


@pytest.mark.parametrize("cont", [True, False], ids=["cont", "nocont"])
@pytest.mark.parametrize("material", [1, 2, 4], ids=["diffuse", "transparent", "clearcoat"])
@pytest.mark.parametrize("program", PROGRAMS)
def test_materials(monkeypatch, program, material, cont):
    """The other model materials (Diffuse: shadow rays and the any-hit walk; Transparent: double-sided leaves and the
    refraction's flags; ClearCoat: the coat flag) at 33x17, where every tile has helper lanes."""
    rep, _ = _case(monkeypatch, program, material, (33, 17), cont)
    _assert_cont(rep, (33, 17), cont)


@pytest.mark.parametrize("material", [3, 2], ids=["metal", "transparent"])
@pytest.mark.parametrize("program", PROGRAMS)
def test_split_tiles_placement(monkeypatch, program, material):
    """Tile splitting forced (a compacting draw splits none, so compaction is off): the 24 tiles of 96x64 are shaded by
    4x4-pixel waves of 16 lanes, whose pixels the kernel re-forms from the part and the lane id."""
    rep, _ = _case(monkeypatch, program, material, (96, 64), False, env={"PT_SPLIT_ALWAYS": "1", "PT_SPLIT_TILES": "64"})
    _assert_cont(rep, (96, 64), False)
    assert rep["qs"]["split_tiles"] >= 8, rep["qs"]


@pytest.mark.parametrize("cont", [True, False], ids=["cont", "nocont"])
@pytest.mark.parametrize("program", PROGRAMS)
def test_three_way_rows_one_part_owns_nothing(monkeypatch, program, cont):
    """33x17 is two 16-row bands, the second of one row: of three row partitions the third owns no band and draws
    nothing, the other two place their waves from their own band numbers."""
    rep, _ = _case(monkeypatch, program, METAL, (33, 17), cont, parts=3)
    _assert_cont(rep, (33, 17), cont, bands=2)


@pytest.mark.parametrize("program", PROGRAMS)
def test_every_kind_of_object_wins_at_bounce_0_and_later(monkeypatch, program):
    """A sphere, a quad and the mesh each win a segment at bounce 0 and at a later bounce, so the sphere normal
    recomputed after the walk, the quads' attributes and the mesh lookup all run at both. Read from the oracle's
    object ids of the first frame at 96x64: with a Diffuse model the G-buffer's id is bounce 0's winner; with a Metal
    model the pixels whose bounce 0 is the mesh carry bounce 1's winner (a miss leaves the mesh's id, so the mesh
    counts as a later winner only in the glTF scene's closed room). Then the Metal frames are bit-exact with
    compaction on."""
    W, Hh = 96, 64
    ids = {}
    for material in (1, METAL):
        _, meta, mesh = _scene(program, material)
        sc = H.oracle_scene(meta, W, Hh, mesh)
        ids[material] = sc.gbuffer(H.with_resolution(H.path_call(meta["frames"][0])["uniforms"], W, Hh))[..., 6]
    mesh_id = float(ids[1].max())                      # objectCount after the spheres and quads
    assert mesh_id == (8.0 if program == "gltf" else 6.0)
    later = ids[METAL][ids[1] == mesh_id]
    for where, got in (("bounce 0", ids[1]), ("bounce 1", later)):
        assert (got == 1.0).any(), "%s: no sphere wins at %s" % (program, where)
        assert ((got >= 2.0) & (got < mesh_id)).any(), "%s: no quad wins at %s" % (program, where)
    assert (ids[1] == mesh_id).sum() > 50
    if program == "gltf":
        assert (later == mesh_id).any(), "no mesh hit after the mesh"
    rep, ref = _case(monkeypatch, program, METAL, (W, Hh), True)
    _assert_cont(rep, (W, Hh), True)
    assert ref["counters"]["hit_lookups"] > 0

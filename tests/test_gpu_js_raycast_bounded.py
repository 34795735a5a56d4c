"""The JavaScript host's bounded ray queries (js/replay_raycast_bounded.js: Effect.castRays with tMax, with occluded,
and Effect.lineOfSight over the N-API addon) against the Python binding's, byte for byte, on one mesh case.

Run on an MI355X: python -m pytest tests/test_gpu_js_raycast_bounded.py -m gpu
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import raycast_bounded_ref as B
import raycast_cases as C
import raycast_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.skipif(not shutil.which("node"), reason="node not installed")
def test_node_bounded_queries_match_python(engine, tmp_path):
    """The glTF teapot stream as recorded, nothing drawn, the case's rays bounded at the float above t_ref, at half of
    it and at one and a half of it by turns: the shim's records and flags are the Python binding's bytes (which
    tests/test_gpu_raycast_bounded.py holds to the reference), and lineOfSight's answers for the segments from each
    origin to 5 % short of and 5 % beyond its ray's hit are the binding's."""
    import babylon_pt as bp
    name = "gltf_teapot"
    meta = H.stream(C.CASES[name][0])
    assert not C.CASES[name][1], "the script sets the stream's own uniforms"
    o, d, _ = C.rays_of(name)
    n = len(o)
    turn = np.arange(n) % 3
    t = np.select([turn == 0, turn == 1], [B.t_max_of(name, "above_t_ref"), B.t_max_of(name, "half")],
                  B.t_max_of(name, "one_and_a_half")).astype(np.float32)
    ref = C.reference(name)
    ok = np.nonzero((ref["object_id"] >= 0) & np.isfinite(d).all(1))[0]
    p = np.concatenate([o[ok], o[ok]])
    q = np.concatenate([o[ok] + d[ok] * (ref["t"][ok] * np.float32(0.95))[:, None], o[ok] + d[ok] * (ref["t"][ok] * np.float32(1.05))[:, None]]).astype(np.float32)
    H.bluenoise().tofile(tmp_path / "bluenoise.u8")
    payload = H.texture_payloads(meta, C.mesh_of(C.CASES[name][2]))
    for k, v in payload.items():
        v.tofile(tmp_path / (k + ".f32"))
    for f, a in (("origins", o), ("dirs", d), ("tmax", t), ("p", p), ("q", q)):
        np.ascontiguousarray(a, np.float32).tofile(tmp_path / (f + ".f32"))
    out = str(tmp_path / "out")
    script = os.path.join(H.ROOT, "babylon.js-pathtracing-renderer_amd", "js", "replay_raycast_bounded.js")
    subprocess.run(["node", script, os.path.join(H.GOLD, C.CASES[name][0] + ".json"), str(tmp_path), out], check=True, timeout=300)
    js_hits = np.fromfile(out + ".hits.bin", R.RAY_HIT)
    js_occ = np.fromfile(out + ".occluded.bin", np.uint8)
    js_los = json.load(open(out + ".los.json"))

    player = bp.StreamPlayer(engine, meta, H.bluenoise(), payload)
    try:
        call = H.path_call(meta["frames"][0])
        fx = player.wrappers[call["effect"]].effect
        for uname, ent in call["uniforms"].items():
            fx._set_entry(uname, ent)
        for sname, tex in call["samplers"].items():
            fx.setTexture(sname, player.textures.get(tex) if tex else None)
        py_hits = fx.cast_rays(o, d, t)
        py_occ = fx.occluded(o, d, t)
        py_los = fx.line_of_sight(p, q)
    finally:
        for raw in meta["textures"]:
            player.textures[raw].dispose()
    assert js_hits.tobytes() == py_hits.tobytes()
    assert js_occ.tobytes() == py_occ.astype(np.uint8).tobytes()
    assert js_los == py_los.tolist()
    # the inputs did their work: bounded misses and hits among the records, both answers among the segments
    assert (py_hits["object_id"][turn == 1] < 0).all() and (py_hits["triangle"][turn == 2] >= 0).sum() > 5
    # (a ray that grazes a nearer triangle's box may find that triangle on the shorter segment: not every short one is free)
    assert py_los[:len(ok)].sum() > 100 and not py_los[len(ok):].any()

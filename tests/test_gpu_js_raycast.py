"""The JavaScript host's ray queries (js/replay_raycast.js: Effect.castRays and Effect.pick over the N-API addon)
against the Python binding's, byte for byte, on one mesh case.

Run on an MI355X: python -m pytest tests/test_gpu_js_raycast.py -m gpu
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import raycast_cases as C
import raycast_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.skipif(not shutil.which("node"), reason="node not installed")
def test_node_cast_rays_and_pick_match_python(engine, tmp_path):
    """The glTF teapot stream as recorded, nothing drawn: the shim's records for the case's rays are the Python
    binding's bytes (which tests/test_gpu_raycast.py holds to the reference), and so is the record under a pixel."""
    import babylon_pt as bp
    name = "gltf_teapot"
    meta = H.stream(C.CASES[name][0])
    assert not C.CASES[name][1], "the script sets the stream's own uniforms"
    o, d, _ = C.rays_of(name)
    H.bluenoise().tofile(tmp_path / "bluenoise.u8")
    payload = H.texture_payloads(meta, C.mesh_of(C.CASES[name][2]))
    for k, v in payload.items():
        v.tofile(tmp_path / (k + ".f32"))
    o.tofile(tmp_path / "origins.f32")
    d.tofile(tmp_path / "dirs.f32")
    out = str(tmp_path / "out")
    px, py = 150, 80
    script = os.path.join(H.ROOT, "babylon.js-pathtracing-renderer_amd", "js", "replay_raycast.js")
    subprocess.run(["node", script, os.path.join(H.GOLD, C.CASES[name][0] + ".json"), str(tmp_path), out, str(px), str(py)],
                   check=True, timeout=300)
    js = np.fromfile(out + ".hits.bin", R.RAY_HIT)

    player = bp.StreamPlayer(engine, meta, H.bluenoise(), payload)
    try:
        call = H.path_call(meta["frames"][0])
        fx = player.wrappers[call["effect"]].effect
        for uname, ent in call["uniforms"].items():
            fx._set_entry(uname, ent)
        for sname, tex in call["samplers"].items():
            fx.setTexture(sname, player.textures.get(tex) if tex else None)
        py_hits = fx.cast_rays(o, d)
        pick = fx.pick(px, py, meta["width"], meta["height"])
    finally:
        for raw in meta["textures"]:
            player.textures[raw].dispose()
    assert js.tobytes() == py_hits.tobytes()
    assert (py_hits["triangle"] >= 0).sum() > 20
    got = json.load(open(out + ".pick.json"))
    assert pick["object_id"] >= 0 and got["hit"] is True
    assert (np.float32(got["t"]), got["objectId"], got["type"], got["triangle"]) == (pick["t"], pick["object_id"], pick["type"], pick["triangle"])
    assert np.array_equal(np.array(got["normal"] + [got["baryU"]] + got["color"] + [got["baryV"]] + got["uv"], np.float32).view(np.uint32),
                          np.concatenate([pick["normal"], [pick["bary_u"]], pick["color"], [pick["bary_v"]], pick["uv"]]).astype(np.float32).view(np.uint32))

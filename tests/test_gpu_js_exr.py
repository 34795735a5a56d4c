"""The Node host's route to pt_targets_encode_exr and its job form: js/replay_encode_exr.js replays two frames of the
Cornell stream at its recorded size through the shim and the addon and encodes the accumulation as B G R (HALF, at
1 / frames, given out of order) and A (FLOAT); the bytes are the reference's for the texels it read
(tests/exr_enc_ref.py) and the Python binding's for the same frames, and the job's file is the synchronous call's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import exr_enc_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.skipif(not shutil.which("node"), reason="node not installed")
def test_node_route(tmp_path):
    import babylon_pt as bp
    meta = H.stream("cornell_256")
    W, Hh = meta["width"], meta["height"]
    H.bluenoise().tofile(tmp_path / "bluenoise.u8")
    out = str(tmp_path / "out")
    script = os.path.join(H.ROOT, "babylon.js-pathtracing-renderer_amd", "js", "replay_encode_exr.js")
    subprocess.run(["node", script, os.path.join(H.GOLD, "cornell_256.json"), str(tmp_path), out, "2", "jobs"],
                   check=True, timeout=300)
    js = open(out + ".exr", "rb").read()
    acc = np.fromfile(out + ".acc.f32", np.float32).reshape(Hh, W, 4)
    assert acc[..., :3].any()
    assert js == R.encode([("B", acc, 2, 0.5, R.HALF), ("G", acc, 1, 0.5, R.HALF), ("R", acc, 0, 0.5, R.HALF),
                           ("A", acc, 3, 1.0, R.FLOAT)], R.ZIP)
    assert open(out + ".job.exr", "rb").read() == js
    e = bp.Engine(0)
    try:
        player = bp.StreamPlayer(e, meta, H.bluenoise(), None, None, None)
        e.resize_canvas(player.width, player.height)
        for i in range(2):
            player.play_frame(i)
        t = player.textures["pathTracingRenderTarget"]
        data = e.encode_targets_exr([("R", t, 0, 0.5, "half"), ("G", t, 1, 0.5, "half"), ("B", t, 2, 0.5, "half"),
                                     ("A", t, 3, 1.0, "float")], "zip")
    finally:
        e.dispose()
    assert js == data

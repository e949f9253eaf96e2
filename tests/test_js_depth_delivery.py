"""The depth ring through the JavaScript host: `f.depth` holds the Python host's bytes for the same scene and pose (SHA-256), as a
view of the slot's ArrayBuffer where the layout says, and the colour beside it is the Python host's."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_delivery_reference as DD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "depth_delivery_check.js")
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the addon is missing")]


def test_js_depth_is_the_python_hosts(tmp_path):
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H, pose = cfg["width"], cfg["height"], 7
    rows = gh.synth.config_rows("C1")
    f = tmp_path / "c1.splat"
    rows.tofile(f)
    out = tmp_path / "depth.json"
    r = subprocess.run([NODE, DRIVER, "planes", str(f), str(out), str(W), str(H), str(cfg["fx"]), str(pose)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.load(open(out))
    scene = gh.Scene()
    scene.setData(rows)
    py = gh.HIPRenderer(W, H)
    py.render(scene, gh.orbit_camera(pose, width=W, height=H, fx=cfg["fx"]))
    hit = py.read_depth()[1]
    for name, kw, kind in (("u16_2_nv12", dict(format="nv12", depth="u16", depth_step=2, depth_near=0.5), "Uint16Array"),
                           ("f32_1_rgba8", dict(depth="f32"), "Float32Array"),
                           ("u16_1_i420", dict(format="i420", depth="u16"), "Uint16Array")):
        py.open_delivery_depth(2, **kw)
        py.render_async()
        s, px, depth = py.acquire(py.deliver())
        mine = depth.copy()
        colour = px.copy() if isinstance(px, np.ndarray) else np.concatenate([p.ravel() for p in px])
        lay = py.depth_layout()
        py.release(s)
        py.close_delivery()
        want = DD.subsample(hit, kw.get("depth_step", 1))
        if kw["depth"] == "u16":
            want = DD.quantise_u16(want, kw.get("depth_near", 0.1))
        assert np.array_equal(mine.view(np.uint8), want.view(np.uint8)), name
        g = got[name]
        assert g["depthSha256"] == hashlib.sha256(mine.tobytes()).hexdigest(), name
        assert g["pixelsSha256"] == hashlib.sha256(colour.tobytes()).hexdigest(), name
        assert g["kind"] == kind and g["samples"] == mine.size and g["sameBuffer"] and g["sameLayout"]
        assert g["offset"] == lay["offset"] and g["pixelBytes"] == g["layoutBytes"] == colour.size
        assert {k: g["depthLayout"][k] for k in ("format", "step", "width", "height", "stride", "offset", "bytes")} == {k: lay[k] for k in lay if k != "near"}
        assert abs(g["depthLayout"]["near"] - lay["near"]) < 1e-12
    py.dispose()
    assert got["plain"] == {"depth": True, "depthLayout": True, "wholeBuffer": True, "layoutRefused": True}
    assert got["unknownRefused"] and got["stepRefused"]

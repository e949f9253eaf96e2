"""Depth in a group through the JavaScript host, as far as a one-GPU box goes: in a world of one, readFrameDepth() and `f.depth` hold
readDepth().hit sampled and quantised, and the Python host gives the same bytes (SHA-256)."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_delivery_reference as DD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "depth_exchange_check.js")
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the addon is missing")]


def test_js_gathered_depth_is_the_python_hosts(tmp_path):
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H, pose = cfg["width"], cfg["height"], 7
    rows = gh.synth.config_rows("C1")
    f = tmp_path / "c1.splat"
    rows.tofile(f)
    out = tmp_path / "depth.json"
    r = subprocess.run([NODE, DRIVER, "world1", str(f), str(out), str(W), str(H), str(cfg["fx"]), str(pose)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.load(open(out))
    assert got["outsideRefused"] and got["mismatchRefused"] and got["offRefused"]
    scene = gh.Scene()
    scene.setData(rows)
    py = gh.HIPRenderer(W, H)
    py.render(scene, gh.orbit_camera(pose, width=W, height=H, fx=cfg["fx"]))
    hit = py.read_depth()[1]
    py.join_group(gh.new_group_id(), 0, 1, [(0, W)])
    for name, colour_fmt, (fmt, step, near), kind in (("u16_2_rgba8", "rgba8", ("u16", 2, 0.5), "Uint16Array"), ("f32_1_nv12", "nv12", ("f32", 1, 0.1), "Float32Array")):
        py.set_group_depth(fmt, step, near)
        py.open_delivery_depth(2, format=colour_fmt, depth=fmt, depth_step=step, depth_near=near)
        py.render_async()
        py.allgather_frame_async()
        s, px, depth = py.acquire(py.deliver())
        mine = depth.copy()
        colour = px.copy() if isinstance(px, np.ndarray) else np.concatenate([p.ravel() for p in px])
        py.release(s)
        plane = py.read_frame_depth()
        lay = py.frame_depth_layout()
        py.close_delivery()
        want = DD.subsample(hit, step)
        if fmt == "u16":
            want = DD.quantise_u16(want, near)
        assert mine.tobytes() == want.tobytes() == plane.tobytes(), name
        g = got[name]
        assert g["frameDepthSha256"] == g["depthSha256"] == hashlib.sha256(want.tobytes()).hexdigest(), name
        assert g["pixelsSha256"] == hashlib.sha256(colour.tobytes()).hexdigest(), name
        assert g["kind"] == g["ringKind"] == kind and g["samples"] == want.size
        assert {k: g["layout"][k] for k in ("format", "step", "width", "height", "stride", "offset", "bytes")} == {k: lay[k] for k in lay if k != "near"}
        assert g["layout"]["offset"] == 0 and g["ringLayout"]["width"] == lay["width"] and g["ringLayout"]["offset"] > 0
    py.dispose()

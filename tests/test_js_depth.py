"""Depth planes and picking through the JavaScript host: the declared surface (CPU) and, on the GPU, the same bits as the
Python host returns for the same scene and camera, and a picked point that lies on the splat."""
import hashlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "depth_check.js")
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
METHODS = ["setHitAlpha", "depthAsync", "readDepth", "pick"]

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


def run(*args):
    r = subprocess.run([NODE, DRIVER] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_depth_methods_are_declared_and_defined():
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    cls = dts[dts.index("export class HIPRenderer"):]
    cls = cls[:cls.index("\n}")]
    for m in METHODS:
        assert re.search(r"\b%s\(" % m, cls), "index.d.ts does not declare HIPRenderer.%s" % m
    assert "point: Vector3 | null" in cls
    assert json.loads(run("surface")) == {"methods": METHODS}


def test_addon_exports_the_depth_calls():
    if not os.path.exists(ADDON):
        pytest.skip("the addon is not built (no Node headers)")
    out = subprocess.run(["strings", "-a", ADDON], capture_output=True, text=True).stdout
    for name in ("setHitAlpha", "depthAsync", "readDepth", "gsr_pick"):
        assert name in out, name


@pytest.mark.gpu
def test_js_planes_and_picks_are_the_python_hosts(tmp_path):
    if not os.path.exists(ADDON):
        pytest.skip("the addon is not built (no Node headers)")
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H, pose = cfg["width"], cfg["height"], 7
    rows = gh.synth.config_rows("C1")
    f = tmp_path / "c1.splat"
    rows.tofile(f)
    rng = np.random.default_rng(64)
    pts = np.stack([rng.integers(0, W, 64), rng.integers(0, H, 64)], axis=1)
    out = tmp_path / "planes.json"
    run("planes", f, out, W, H, cfg["fx"], pose, ";".join("%d,%d" % (x, y) for x, y in pts))
    got = json.load(open(out))
    scene = gh.Scene()
    scene.setData(rows)
    r = gh.HIPRenderer(W, H)
    r.render(scene, gh.orbit_camera(pose, width=W, height=H, fx=cfg["fx"]))
    mean, hit, index = r.read_depth()
    picks = r.pick(pts)
    r.dispose()
    assert (index != 0xFFFFFFFF).any()
    assert got["filled"] and got["partial"] and got["refused"] and got["alphaRefused"], got
    for name, plane in (("mean", mean), ("hit", hit), ("index", index)):
        assert got[name] == hashlib.sha256(plane.tobytes()).hexdigest(), name
    want = [[int(p["index"]), int(p["depth"].view(np.uint32)), int(p["mean"].view(np.uint32)), int(p["alpha"].view(np.uint32)),
             bool(p["index"] == 0xFFFFFFFF)] for p in picks]
    assert got["picks"] == want


@pytest.mark.gpu
def test_js_picked_point_lies_on_the_splat(tmp_path):
    if not os.path.exists(ADDON):
        pytest.skip("the addon is not built (no Node headers)")
    row = np.zeros(32, dtype=np.uint8)
    row[0:12] = np.zeros(3, dtype=np.float32).view(np.uint8)                # at the orbit target
    row[12:24] = np.full(3, 0.2, dtype=np.float32).view(np.uint8)
    row[24:28] = (255, 255, 255, 255)
    row[28:32] = (255, 128, 128, 128)
    f = tmp_path / "one.splat"
    row.tofile(f)
    out = tmp_path / "point.json"
    run("point", f, out)
    got = json.load(open(out))
    for g in got[:3]:
        assert g["index"] == 0 and abs(g["depth"] - 8.0) < 1e-4 and g["alpha"] > 0.9, g
        assert max(abs(c) for c in g["point"]) < 1e-3, g
    assert got[3] == {"index": 0xFFFFFFFF, "depth": True, "point": None}

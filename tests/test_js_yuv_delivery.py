"""Y'CbCr delivery through the JavaScript host: its payload is the Python host's (SHA-256 of the same pose), and the `planes`
views lie where the layout says."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import yuv_reference as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "yuv_check.js")
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the addon is missing")]


def test_js_payload_is_the_python_hosts(tmp_path):
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H, pose = cfg["width"], cfg["height"], 7
    rows = gh.synth.config_rows("C1")
    f = tmp_path / "c1.splat"
    rows.tofile(f)
    out = tmp_path / "yuv.json"
    r = subprocess.run([NODE, DRIVER, "payload", str(f), str(out), str(W), str(H), str(cfg["fx"]), str(pose)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.load(open(out))
    scene = gh.Scene()
    scene.setData(rows)
    py = gh.HIPRenderer(W, H)
    py.render(scene, gh.orbit_camera(pose, width=W, height=H, fx=cfg["fx"]))
    rgba = py.readPixels()
    for name, kw in (("nv12", dict(format="nv12")), ("i420", dict(format="i420")),
                     ("nv12_full_bg", dict(format="nv12", full_range=True, background=(255, 128, 7)))):
        fmt = kw["format"]
        py.open_delivery(2, **kw)
        py.render_async()
        s, planes = py.acquire(py.deliver())
        mine = np.concatenate([p.ravel() for p in planes])
        py.release(s)
        py.close_delivery()
        assert np.array_equal(mine, yr.payload(rgba, fmt, kw.get("full_range", False), kw.get("background", (0, 0, 0))))
        g = got[name]
        ref = yr.layout(W, H, fmt)
        assert g["sha256"] == hashlib.sha256(mine.tobytes()).hexdigest(), name
        assert g["bytes"] == ref["bytes"] == g["layout"]["bytes"] and g["format"] == fmt == g["layout"]["format"]
        assert [(p["offset"], p["stride"], p["rows"]) for p in g["layout"]["planes"]] == ref["planes"]
        assert [(p["offset"], p["stride"], p["rows"], p["length"]) for p in g["planes"]] == [(o, st, n, st * n) for o, st, n in ref["planes"]]
        assert all(p["sameBuffer"] for p in g["planes"]) and g["planesCoverPayload"]
    py.dispose()
    assert got["rgba8"] == {"format": "rgba8", "planes": 1, "stride": W * 4, "equal": True}
    assert got["unknownRefused"] and got["openWhileOpenRefused"]

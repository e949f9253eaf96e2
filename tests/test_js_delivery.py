"""Frame delivery through the JavaScript host: the declared surface (CPU) and, on the GPU, the delivered pixels, the
identity of the slots' ArrayBuffers and what happens to a view when its memory goes away."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "delivery_check.js")
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
METHODS = ["openDelivery", "closeDelivery", "deliverFrame", "frameReady", "acquireFrame"]

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


def run(*args):
    r = subprocess.run([NODE, DRIVER] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_delivery_methods_are_declared_and_defined():
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    cls = dts[dts.index("export class HIPRenderer"):]
    cls = cls[:cls.index("\n}")]
    for m in METHODS:
        assert re.search(r"\b%s\(" % m, cls), "index.d.ts does not declare HIPRenderer.%s" % m
    frame = dts[dts.index("export interface DeliveredFrame"):]
    frame = frame[:frame.index("\n}")]
    for field in ("serial: number", "pixels: Uint8Array", "release(): void"):
        assert field in frame
    got = json.loads(run("surface"))
    assert got == {"exported": True, "methods": METHODS}


def test_addon_exports_the_delivery_calls():
    if not os.path.exists(ADDON):
        pytest.skip("the addon is not built (no Node headers)")
    out = subprocess.run(["strings", "-a", ADDON], capture_output=True, text=True).stdout
    for name in ("openDelivery", "closeDelivery", "deliverySlots", "detachBuffers", "deliverFrame", "frameReady", "acquireFrame", "releaseFrame"):
        assert name in out, name


def _splat(tmp_path):
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C1"]
    f = tmp_path / "c1.splat"
    gh.synth.config_rows("C1").tofile(f)
    return f, cfg


@pytest.mark.gpu
def test_js_delivered_frames(tmp_path):
    f, cfg = _splat(tmp_path)
    out = tmp_path / "d.json"
    run("deliver", f, out, cfg["width"], cfg["height"], cfg["fx"])
    got = json.load(open(out))
    assert got["equal"] and got["frames"] == 9 and got["serials"] == list(range(1, 10)), got
    assert got["sameBuffer"] and got["distinctBuffers"] == 3, got     # one ArrayBuffer per slot, the same every lap
    assert got["oldestFirst"] and got["busy"] and got["resizeRefused"] and got["closeRefused"], got
    assert got["detachedAfterResize"] and got["resized"] and got["detachedAfterDispose"] and got["safeRead"], got


@pytest.mark.gpu
def test_js_delivery_after_join_group(tmp_path):
    f, cfg = _splat(tmp_path)
    out = tmp_path / "g.json"
    run("group", f, out, cfg["width"], cfg["height"], cfg["fx"])
    assert json.load(open(out)) == {"equal": True, "frames": 4, "equalsReadFrame": True}

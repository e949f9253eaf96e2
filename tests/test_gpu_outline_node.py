"""The selection outline through the Node host, on the GPU (tests/js/outline_device_check.js, in a fresh child process): what
readOverlay, readPixels({ overlay: true }) and a delivered overlay frame return with an outline set are the Python host's bytes
for the same rows, camera, selection and options (SHA-256)."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "outline_device_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "without_overlay_options_it_is_refused", "an_inner_outline_changes_some_inside_pixels_and_no_other", "cover_is_not_changed",
    "a_bad_width_is_refused_by_the_library", "a_delivered_frame_carries_the_outline", "null_switches_it_off",
]


def test_node_host_equals_the_python_host(tmp_path):
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    r = subprocess.run([NODE, DRIVER, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checks"] == EXPECTED
    assert out["failed"] == []

    import gsplat_hip as gh
    load = lambda name, dtype: np.fromfile(os.path.join(str(tmp_path), name), dtype=dtype)
    rows, cam, words = load("rows.bin", np.uint8), load("cameras.bin", np.float32), load("selection.bin", np.uint32)
    py = gh.HIPRenderer(out["width"], out["height"])
    py.set_scene_rows(rows)
    py.set_overlay(out["tint"], out["mix"])
    ol = out["outline"]
    py.set_overlay_outline(ol["color"], ol["alpha"], ol["threshold"], ol["width"], ol["side"])
    assert py.set_selection(words=words) == out["selected"]
    py.set_camera_arrays(cam[0:16].copy(), cam[16:32].copy(), cam[32:48].copy(), float(cam[48]), float(cam[49]))
    py.render_async(); py.sync()
    rgba, cover = py.read_overlay()
    assert hashlib.sha256(rgba.tobytes() + cover.tobytes()).hexdigest() == out["sha256"]
    px = py.read_overlay_rgba8()
    assert hashlib.sha256(px.tobytes()).hexdigest() == out["sha256_rgba8"] == out["sha256_delivered"]
    py.set_overlay_outline(None)
    assert int((py.read_overlay()[0].view(np.uint32) != rgba.view(np.uint32)).any(axis=2).sum()) == out["edge"]
    py.dispose()

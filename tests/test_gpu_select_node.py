"""Selection through the Node host, on the GPU: selectRegion -> readSelection -> Scene.eraseSelection on two renderers that share a
scene and a third with a copy of its own (tests/js/select_device_check.js, in a fresh child process), and the Scene's mirrors
against what the Python host gets from the same rows, camera and lasso."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "select_device_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "two_share_one_has_its_own", "select_region_counts_its_words", "members_have_one_selection", "own_copy_selects_the_same",
    "hit_intersects_through_the_other_member", "ops_and_invert", "erase_once_per_device_copy", "count_follows",
    "mirrors_are_the_kept_splats_in_order", "host_loop_equals_the_devices", "frames_equal_a_fresh_renderer",
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
    rows, cam, words = load("rows.bin", np.uint8), load("camera.bin", np.float32), load("words.bin", np.uint32)
    x0, y0, x1, y1 = out["rect"]
    ys, xs = np.mgrid[0:y1 - y0, 0:x1 - x0]
    mask = np.full((y1 - y0, out["stride"]), 9, dtype=np.uint8)
    mask[:, :x1 - x0] = (xs + 0.5 - 40) ** 2 + (ys + 0.5 - 40) ** 2 <= 1600
    py = gh.HIPRenderer(out["width"], out["height"])
    py.set_scene_rows(rows)
    py.set_camera_arrays(cam[0:16].copy(), cam[16:32].copy(), cam[32:48].copy(), float(cam[48]), float(cam[49]))
    py.render_async(); py.sync()
    assert py.select_region((x0, y0, x1, y1), mask) == out["picked"]
    assert np.array_equal(py.selection_words(), words)
    assert py.scene_erase_selected() == rows.size // 32 - out["picked"]
    data, pos, rot, scl = py.read_scene()
    py.dispose()
    for got, name in ((data, "data"), (pos, "positions"), (rot, "rotations"), (scl, "scales")):
        assert np.array_equal(got.view(np.uint32), load("after_%s.bin" % name, np.uint32)), name

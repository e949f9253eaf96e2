"""Hidden splats through the Node host, on the GPU: selectRegion -> hideSelection -> readHidden -> readPixels, and Scene.setHidden on
renderers with separate device copies (tests/js/hide_device_check.js, in a fresh child process), against the bytes the Python host
produces for the same rows, camera and mask."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "hide_device_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "nothing_hidden_at_first", "hide_selection_hides_the_selection", "members_have_one_hidden_set", "a_change_is_a_scene_edit", "the_hidden_frame_differs",
    "depth_sees_through", "select_hidden_is_a_picker", "ops", "the_other_member_renders_the_hidden_frame", "show_all", "shown_again_bit_for_bit",
    "scene_set_hidden_once_per_device_copy", "reaches_both_copies", "both_copies_render_the_hidden_frame", "scene_show_all",
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
    rows, cam, hidden = load("rows.bin", np.uint8), load("camera.bin", np.float32), load("hidden.bin", np.uint32)
    W, H = out["width"], out["height"]
    py = gh.HIPRenderer(W, H)
    py.set_scene_rows(rows)
    py.set_camera_arrays(cam[0:16].copy(), cam[16:32].copy(), cam[32:48].copy(), float(cam[48]), float(cam[49]))
    py.render_async(); py.sync()
    assert np.array_equal(py.readPixels().reshape(-1), load("pixels_shown.bin", np.uint8))
    assert py.select_region(tuple(out["rect"])) == out["picked"]
    assert py.hide_selected() == out["picked"]
    assert np.array_equal(py.hidden_words(), hidden)          # the same mask ...
    py.render_async(); py.sync()
    assert np.array_equal(py.readPixels().reshape(-1), load("pixels_hidden.bin", np.uint8))   # ... and the same bytes
    fresh = gh.HIPRenderer(W, H)                              # and from the words alone
    fresh.set_scene_rows(rows)
    assert fresh.set_hidden(words=hidden) == out["picked"]
    fresh.set_camera_arrays(cam[0:16].copy(), cam[16:32].copy(), cam[32:48].copy(), float(cam[48]), float(cam[49]))
    fresh.render_async(); fresh.sync()
    assert np.array_equal(fresh.readPixels().reshape(-1), load("pixels_hidden.bin", np.uint8))
    py.dispose(); fresh.dispose()

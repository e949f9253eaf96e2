"""Contribution through the Node host, on the GPU (tests/js/contrib_device_check.js, in a fresh child process): the arrays
readContribution returns are the Python host's for the same rows and cameras (SHA-256), and selectContribution selects as many."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "contrib_device_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "an_empty_tour_is_refused", "arrays_have_the_types_and_the_count", "some_splats_show_and_some_never_do", "never_shown_is_selected",
    "weight_threshold_matches_the_arrays", "ops_fold_like_the_selection_calls",
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
    rows, cams = load("rows.bin", np.uint8), load("cameras.bin", np.float32).reshape(out["poses"], 50)
    py = gh.HIPRenderer(out["width"], out["height"])
    py.set_scene_rows(rows)
    py.contrib_reset()
    for cam in cams:
        py.set_camera_arrays(cam[0:16].copy(), cam[16:32].copy(), cam[32:48].copy(), float(cam[48]), float(cam[49]))
        py.render_async(); py.sync()
        py.contrib_accumulate()
    weight, peak, pixels, frames = py.read_contrib()
    assert frames == out["frames"] == out["poses"]
    assert hashlib.sha256(weight.tobytes() + peak.tobytes() + pixels.tobytes()).hexdigest() == out["sha256"]
    assert py.select_contrib("pixels", 1.0) == out["never"] == int((pixels == 0).sum())
    assert py.select_contrib("weight", 2.5) == out["light"]
    assert py.select_contrib("peak", 0.05, op="intersect") == out["faint"]
    py.dispose()

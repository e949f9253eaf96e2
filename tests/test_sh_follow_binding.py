"""Scene.shFollowsTransforms (gsplat.js_amd/js/core/Scene.js) on a box without a GPU: the JavaScript path and the device-scene
interface, with a plain Scene behind it, leave the same shs_rgb, bandsIndices, shFrame and shHeight; with the option off the
Scene behaves as before (tests/js/sh_follow_check.js)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "sh_follow_check.js")
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

EXPECTED = [
    "frame_identity_after_setData", "js_recount_is_brute_force", "js_rows_move_in_order", "js_zeros_behind_and_height",
    "attach_tells_the_device", "no_sh_read_until_asked", "not_dropped_with_follow", "interface_path_equals_js_path",
    "second_read_pulls_nothing", "nothing_kept_clears_both", "foreign_change_uploads_compacted_sh", "detach_last_refreshes_sh",
    "zero_scale_refused_with_follow", "off_frame_stays_identity", "off_limitbox_sets_shDroppedOnDevice", "off_sh_untouched",
    "off_zero_scale_accepted", "device_without_readSh_forces_js_path",
]


@pytest.fixture(scope="module")
def protocol():
    r = subprocess.run([NODE, DRIVER, "protocol"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_driver_ran_every_check(protocol):
    assert protocol["checks"] == EXPECTED


@pytest.mark.parametrize("name", EXPECTED)
def test_protocol(protocol, name):
    assert name in protocol["checks"] and name not in protocol["failed"]


def test_frame_statements_agree_with_the_specification():
    """Scene.js's f64 frame after rotate; scale; rotate equals tests/sh_follow_reference.py's, bit for bit."""
    import numpy as np
    import sh_follow_reference as ref
    script = ("const G = require(%r); const s = new G.Scene(); s.shFollowsTransforms = true;"
              "s.rotate(new G.Quaternion(0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214));"
              "s.scale(new G.Vector3(1.25, 0.75, 1.5)); s.rotate(new G.Quaternion(-0.5, 0.5, 0.5, 0.5));"
              "console.log(JSON.stringify(Array.from(new BigUint64Array(s.shFrame.buffer), String)));") % os.path.join(ROOT, "gsplat.js_amd", "js")
    r = subprocess.run([NODE, "-e", script], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.array([int(v) for v in json.loads(r.stdout)], dtype=np.uint64)
    want = ref.frame_after((("rotate", (0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214)),
                            ("scale", (1.25, 0.75, 1.5)), ("rotate", (-0.5, 0.5, 0.5, 0.5))))
    assert np.array_equal(got, np.ascontiguousarray(want).reshape(-1).view(np.uint64))

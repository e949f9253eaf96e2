"""The Scene's binding to device scenes (gsplat.js_amd/js/core/Scene.js) on a box without a GPU: the protocol runs against a
stub device scene, a second plain Scene behind the interface the renderer hands over (tests/js/scene_binding_check.js)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "scene_binding_check.js")
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

EXPECTED = [
    "transform_once_per_device", "no_js_loop_until_read", "change_once_per_edit", "first_read_pulls_once", "second_read_pulls_nothing",
    "arrays_equal_unbound_after_rotate", "limitbox_count_at_once", "limitbox_shapes", "listener_reads_edited_words", "toSplatBytes_refreshes",
    "foreign_change_uploads", "foreign_change_while_stale_refreshes_first", "detach_not_last_reads_nothing", "detach_last_refreshes",
    "unattached_again_is_plain_js", "setter_refreshes_then_owns", "edit_after_setter_runs_on_host", "back_on_device_after_upload",
    "setData_uploads_and_owns", "device_path_after_setData", "host_only_attach_sees_edits", "host_only_forces_js_path",
    "limitbox_errors_unchanged", "count_disagreement_throws", "random_sequences_equal_unbound",
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


def test_renderer_hands_the_scene_a_device_scene():
    """The renderer's side of the binding is in place (what it does is checked on the GPU: tests/test_gpu_scene_binding.py)."""
    src = open(os.path.join(ROOT, "gsplat.js_amd", "js", "renderers", "HIPRenderer.js")).read()
    for word in ("attachDevice", "detachDevice", "deviceEditApplied", "shDroppedOnDevice", "setSceneArrays", "readSceneArrays"):
        assert word in src
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("DeviceScene", "attachDevice", "detachDevice", "deviceEditApplied", "shDroppedOnDevice"):
        assert word in dts

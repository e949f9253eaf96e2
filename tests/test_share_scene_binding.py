"""A Scene attached to device scenes of which some are ONE device copy (renderers whose contexts share a scene), on a box without a
GPU: three stub device scenes, two with the same `share` token behind one twin and one without a token
(tests/js/share_scene_binding_check.js).  An edit or an option reaches each distinct copy once."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "share_scene_binding_check.js")
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

EXPECTED = [
    "rotate_once_per_distinct_share_in_attach_order", "rotate_reached_both_copies", "limitbox_once_per_distinct_share_in_attach_order",
    "limitbox_count_from_the_calls", "set_sh_follow_once_per_distinct_share", "mirrors_refresh_from_a_member",
    "arrays_equal_unbound", "without_tokens_every_device_is_called", "third_alone_still_works", "third_alone_arrays_equal_unbound",
]


@pytest.fixture(scope="module")
def protocol():
    r = subprocess.run([NODE, DRIVER], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_driver_ran_every_check(protocol):
    assert protocol["checks"] == EXPECTED


@pytest.mark.parametrize("name", EXPECTED)
def test_protocol(protocol, name):
    assert name in protocol["checks"] and name not in protocol["failed"]


def test_renderer_and_typings_carry_the_share():
    src = open(os.path.join(ROOT, "gsplat.js_amd", "js", "renderers", "HIPRenderer.js")).read()
    for word in ("shareSceneWith", "shareScene", "sceneSharing", "get share()"):
        assert word in src
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("shareSceneWith", "shareScene(other: HIPRenderer)", "sceneSharing()", "share?:"):
        assert word in dts
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    assert '{"shareScene", ShareScene}' in addon and '{"sceneSharing", SceneSharing}' in addon

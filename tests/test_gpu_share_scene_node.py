"""Shared scenes through the Node host, on the GPU: a renderer created with { shareSceneWith } shares the first renderer's device
copy of a Scene instead of uploading it, the Scene issues an edit once for the two, and both render what an unshared renderer
renders (tests/js/share_scene_device_check.js compares bit for bit, in a fresh child process)."""
import json
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "share_scene_device_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "second_renderer_shared_instead_of_uploading", "two_members_same_bytes", "frames_equal_unshared_before_the_edit",
    "rotate_is_one_native_transform", "unshared_renderer_makes_its_own", "frames_equal_unshared_after_the_rotate",
    "orders_equal_unshared_after_the_rotate", "limitbox_reaches_both", "reupload_once_and_shared_again",
    "one_transform_after_the_reupload", "first_renderer_disposed_second_renders_on",
]


def test_node_renderers_share_a_scene():
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    r = subprocess.run([NODE, DRIVER], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checks"] == EXPECTED
    assert out["failed"] == []

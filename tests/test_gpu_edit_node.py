"""Editing the selection through the Node host, on the GPU: a Scene attached to real renderers, two of which share one device copy,
edited through Scene.translateSelection / rotateSelection / scaleSelection / paintSelection; its arrays against the unbound host
loops bit for bit, every renderer's frame against a fresh one, and renderer.selectionBounds() against a JavaScript min / max
(tests/js/edit_device_check.js, in a fresh child process)."""
import json
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "edit_device_check.js")
NODE = shutil.which("node")

STEPS = ("translate", "rotate", "rotate_pivot", "scale", "scale_pivot", "paint_opacity", "paint_colour")
EXPECTED = [s + tail for s in STEPS for tail in ("_once_per_device_copy", "_arrays_equal_the_host_loop", "_every_renderer_renders_the_edited_scene")] + [
    "change_fired_as_a_device_edit_and_nothing_was_uploaded", "the_selection_is_the_mask_on_both_copies", "selection_bounds_equal_a_javascript_min_max",
    "selection_bounds_of_nothing", "a_renderer_edit_is_a_scene_edit", "renderer_edits_equal_the_host_loop", "non_finite_scale_is_refused",
]


def test_scene_attached_to_renderers_edits_its_selection_on_the_device():
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    r = subprocess.run([NODE, DRIVER], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checks"] == EXPECTED
    assert out["failed"] == []

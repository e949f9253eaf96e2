"""HIPRenderer.setSelectionOutline without a GPU (tests/js/outline_binding_check.js): against a stub native layer the method reaches
the addon with the documented arguments; renderer, typings and addon table carry the names."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "outline_binding_check.js")
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

EXPECTED = [
    "options_reach_the_addon_with_defaults", "null_switches_it_off", "bad_options_throw_before_the_addon", "the_overlay_call_is_what_it_was",
    "addon_errors_pass_through",
]


@pytest.fixture(scope="module")
def protocol():
    r = subprocess.run([NODE, DRIVER], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_driver_ran_every_check(protocol):
    assert protocol["checks"] == EXPECTED


@pytest.mark.parametrize("name", EXPECTED)
def test_protocol(protocol, name):
    assert name in protocol["checks"] and name not in protocol["failed"], protocol["failed"]


def test_renderer_typings_and_addon_carry_the_names():
    src = open(os.path.join(ROOT, "gsplat.js_amd", "js", "renderers", "HIPRenderer.js")).read()
    for word in ("this.setSelectionOutline", "this._n.setOutline(this._h, 1,", "this.setSelectionOverlay"):
        assert word in src, word
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ('setSelectionOutline(options: { color?: [number, number, number]; alpha?: number; threshold?: number; width?: number; side?: "outer" | "inner" } | null): void',
                 "setSelectionOverlay(options: { tint?: [number, number, number]; mix?: number } | null): void"):
        assert word in dts, word
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    assert '{"setOutline", SetOutline}' in addon
    for call in ("gsr_set_overlay_outline(c, nullptr)", "gsr_set_overlay_outline(c, &o)"):
        assert call in addon, call

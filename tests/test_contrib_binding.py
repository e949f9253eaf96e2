"""HIPRenderer's contribution methods without a GPU (tests/js/contrib_binding_check.js): against a stub native layer the four
methods reach the addon with the header's codes and hand back its arrays; renderer, typings and addon table carry the names."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "contrib_binding_check.js")
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

EXPECTED = [
    "reset_and_accumulate_reach_the_addon_in_order", "read_returns_the_typed_arrays_and_frames", "select_defaults_are_weight_zero_replace",
    "select_codes_follow_the_header", "unknown_stat_or_op_throws_before_the_addon", "addon_errors_pass_through",
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
    for word in ("this.resetContribution", "this.accumulateContribution", "this.readContribution", "this.selectContribution", "{ weight: 0, peak: 1, pixels: 2 }"):
        assert word in src, word
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("resetContribution(): void", "accumulateContribution(): void", "readContribution(): Contribution",
                 "selectContribution(options?: { stat?: ContribStat; below?: number; op?: SelectOp }): number",
                 'export type ContribStat = "weight" | "peak" | "pixels";',
                 "export interface Contribution { weight: BigUint64Array; peak: Float32Array; pixels: Uint32Array; frames: number }"):
        assert word in dts, word
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    for name, fn in (("contribReset", "Call0<gsr_contrib_reset>"), ("contribAccumulate", "Call0<gsr_contrib_accumulate_async>"), ("readContrib", "ReadContrib"),
                     ("selectContrib", "SelectContrib")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    assert "napi_biguint64_array" in addon

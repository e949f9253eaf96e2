"""HIPRenderer's neighbour methods without a GPU (tests/js/neighbour_binding_check.js): against a stub native layer the two methods
reach the addon with the header's flags and the documented defaults, bad arguments throw before the addon, the addon's refusals
pass through; renderer, typings and addon table carry the names, and the Python host has the same constants and signatures."""
import inspect
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "neighbour_binding_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "constants_follow_the_header", "neighbours_defaults_scopes_and_result", "select_defaults_are_everything_replace", "below_is_lo_0_hi_below",
    "bad_arguments_throw_before_the_addon", "addon_errors_pass_through",
]


@pytest.fixture(scope="module")
def protocol():
    if NODE is None:
        pytest.skip("node is not installed")
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
    for word in ("this.splatNeighbours", "this.selectNeighbours", "{ selected: 1, visible: 2 }"):
        assert word in src, word
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("splatNeighbours(radius: number, options?: NeighbourOptions): SplatNeighbours;",
                 "selectNeighbours(radius: number, options?: NeighbourOptions & { below?: number; lo?: number; hi?: number; op?: SelectOp }): number;",
                 "export interface NeighbourOptions { cap?: number; scope?: NeighbourScope | NeighbourScope[]; budget?: number }",
                 "export interface SplatNeighbours { counts: Uint32Array; hist: Uint32Array; inScope: number; nonfinite: number; pairBound: number }",
                 'export type NeighbourScope = "selected" | "visible";'):
        assert word in dts, word
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    for name, fn in (("neighbours", "Neighbours"), ("selectNeighbours", "SelectNeighbours")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for call in ("gsr_neighbours(c,", "gsr_select_neighbours(c,"):
        assert call in addon, call
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "renderer.selectNeighbours(0.05, { below: 3 }); scene.eraseSelection(renderer.readSelection());" in readme     # floaters removed in two calls


def test_python_host_has_the_same_constants_and_signatures():
    import gsplat_hip as gh
    import neighbour_reference as nr
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert int(re.search(r"#define GSR_NEIGHBOUR_MAX_CAP (\d+)u", header).group(1)) == gh.NEIGHBOUR_MAX_CAP == nr.MAX_CAP == 4095
    shifts = {m.group(1): 1 << int(m.group(2)) for m in re.finditer(r"#define GSR_NEIGHBOUR_(DEFAULT|MAX)_BUDGET\s+\(1ull << (\d+)\)", header)}
    assert shifts == {"DEFAULT": gh.NEIGHBOUR_DEFAULT_BUDGET, "MAX": gh.NEIGHBOUR_MAX_BUDGET} == {"DEFAULT": nr.DEFAULT_BUDGET, "MAX": nr.MAX_BUDGET}
    sig = inspect.signature(gh.HIPRenderer.neighbours)
    assert list(sig.parameters)[1:] == ["radius", "cap", "scope", "budget", "counts", "hist"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [64, (), None, True, True]
    sig = inspect.signature(gh.HIPRenderer.select_neighbours)
    assert list(sig.parameters)[1:] == ["radius", "lo", "hi", "cap", "scope", "op", "budget"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [0, None, 64, (), "replace", None]
    assert gh.HIPRenderer._scope_flags(()) == 0 and gh.HIPRenderer._scope_flags("visible") == 2 and gh.HIPRenderer._scope_flags(("selected", "visible")) == 3
    with pytest.raises(ValueError):
        gh.HIPRenderer._scope_flags(("hidden",))
    for bad in (0, 4096):
        with pytest.raises(ValueError):
            gh.HIPRenderer._neighbour_args(1.0, bad, None)
    assert gh.HIPRenderer._neighbour_args(1, 64, None) == (1.0, 64, 0)
    assert [f[0] for f in gh.GsrNeighbourInfo._fields_] == ["in_scope", "nonfinite", "pair_bound", "budget"]

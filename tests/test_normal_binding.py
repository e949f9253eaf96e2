"""HIPRenderer's normal methods without a GPU (tests/js/normal_binding_check.js): against a stub native layer the two methods reach
the addon with the header's flags and the documented defaults, bad arguments throw before the addon, the addon's refusals pass
through; renderer, typings and addon table carry the names, and the Python host has the same constants and signatures."""
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "normal_binding_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "constants_follow_the_header", "normals_defaults_sources_scopes_and_result", "select_defaults_are_everything_replace",
    "select_passes_the_stat_the_axis_the_range_and_the_op", "bad_arguments_throw_before_the_addon", "addon_errors_pass_through",
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
    for word in ("this.splatNormals", "this.selectNormal", "{ knn: 0, own: 1 }", "{ dot: 0, abs_dot: 1, variation: 2 }"):
        assert word in src, word
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("splatNormals(radius: number | undefined, options?: NormalOptions): SplatNormals;",
                 "selectNormal(stat: NormalStat, options?: NormalOptions & { radius?: number; axis?: ArrayLike<number>; lo?: number; hi?: number; op?: SelectOp }): number;",
                 "export interface NormalOptions { k?: number; source?: NormalSource; toward?: ArrayLike<number>; scope?: NeighbourScope | NeighbourScope[]; budget?: number }",
                 "export interface SplatNormals { normals: Float32Array; variation: Float64Array; found: Uint32Array;",
                 'export type NormalSource = "knn" | "own";', 'export type NormalStat = "dot" | "abs_dot" | "variation";'):
        assert word in dts, word
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    for name, fn in (("normals", "Normals"), ("selectNormal", "SelectNormal")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for call in ("gsr_normals(c,", "gsr_select_normal(c,"):
        assert call in addon, call
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert 'renderer.selectNormal("abs_dot", { axis: [0, 1, 0], hi: 0.2, radius: 0.1, k: 8 });' in readme
    assert 'r.select_normal("abs_dot", hi=0.2, axis=(0, 1, 0), radius=0.1, k=8)' in readme


def test_python_host_has_the_same_constants_and_signatures():
    import gsplat_hip as gh
    import normal_reference as nm
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    sources = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define GSR_NORMAL_(KNN|OWN)\s+(\d+)", header)}
    assert sources == gh.NORMAL_SOURCES == nm.SOURCES == {"knn": 0, "own": 1}
    stats = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define GSR_NORMAL_(DOT|ABS_DOT|VARIATION)\s+(\d+)", header)}
    assert stats == gh.NORMAL_STATS == nm.STATS == {"dot": 0, "abs_dot": 1, "variation": 2}
    assert (nm.MIN_K, nm.MAX_K) == (2, gh.KNN_MAX_K)
    sig = inspect.signature(gh.HIPRenderer.normals)
    assert list(sig.parameters)[1:] == ["radius", "k", "source", "toward", "scope", "budget", "normals", "variation", "found"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None, 8, "knn", None, (), None, True, True, True]
    sig = inspect.signature(gh.HIPRenderer.select_normal)
    assert list(sig.parameters)[1:] == ["stat", "lo", "hi", "axis", "radius", "k", "source", "toward", "scope", "op", "budget"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [-np.inf, np.inf, None, None, 8, "knn", None, (), "replace", None]
    x = object.__new__(gh.HIPRenderer)                                 # (the option builder needs no context)
    for bad in (0, 1, 33):
        with pytest.raises(ValueError):
            x._normal_options(1.0, bad, "knn", None, (), None)
    with pytest.raises(ValueError):
        x._normal_options(1.0, 8, "pca", None, (), None)
    with pytest.raises(ValueError):
        x._normal_options(None, 8, "knn", None, (), None)
    with pytest.raises(ValueError):
        x._normal_options(1.0, 8, "knn", None, (), -1)
    o = x._normal_options(0.5, 32, "knn", (1, 2, 3.5), ("selected", "visible"), 77)
    assert (o.source, o.k, o.radius, o.scope, o.oriented, o.budget, list(o.toward)) == (0, 32, 0.5, 3, 1, 77, [1.0, 2.0, 3.5])
    o = x._normal_options(None, 99, "own", None, (), None)
    assert (o.source, o.k, o.radius, o.scope, o.oriented, o.budget, list(o.toward)) == (1, 0, 0.0, 0, 0, 0, [0.0, 0.0, 0.0])
    assert [f[0] for f in gh.GsrNormalInfo._fields_] == ["in_scope", "nonfinite", "pair_bound", "budget", "valid", "variation_min", "variation_max"]
    info = gh.GsrNormalInfo(variation_min=float("inf"), variation_max=float("-inf")).as_dict()
    assert info["variation_min"] == np.inf and info["variation_max"] == -np.inf and isinstance(info["valid"], int)

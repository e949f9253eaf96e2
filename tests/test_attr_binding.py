"""HIPRenderer's splat-data methods without a GPU (tests/js/attr_binding_check.js): against a stub native layer the three methods
reach the addon with the header's codes and the documented defaults, unknown names throw before the addon, the edges follow the
header's formula; renderer, typings and addon table carry the names, and the Python host has the same tables."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "attr_binding_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "codes_follow_the_header", "stats_defaults_and_scopes", "histogram_reaches_the_addon_and_returns_counts_and_edges", "edges_are_computed_by_the_formula",
    "select_defaults_are_everything_replace", "unknown_names_throw_before_the_addon", "addon_errors_pass_through",
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
    for word in ("this.splatStats", "this.splatHistogram", "this.selectAttribute", "HIPRenderer.attrEdges", "contrib_pixels: 15"):
        assert word in src, word
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("splatStats(attr: SplatAttribute, options?: SplatScope): SplatStats;", "splatHistogram(attr: SplatAttribute,", "selectAttribute(attr: SplatAttribute,",
                 "export type SplatAttribute =", '"scale_max"', '"contrib_weight"', "export interface SplatHistogram { counts: Uint32Array; below: number; above: number; nan: number; edges: Float64Array }",
                 "static attrEdges(lo: number, hi: number, bins: number): Float64Array;"):
        assert word in dts, word
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    for name, fn in (("attrStats", "AttrStats"), ("attrHistogram", "AttrHistogram"), ("selectAttr", "SelectAttr")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for call in ("gsr_attr_stats(c,", "gsr_attr_histogram(c,", "gsr_select_attr(c,"):
        assert call in addon, call


def test_python_host_has_the_same_tables_and_edges():
    import gsplat_hip as gh
    import attr_reference as ar
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define GSR_ATTR_([A-Z_]+) (\d+)", header)}
    assert len(codes) == 16 and gh.ATTRS == codes == ar.ATTRS
    assert gh.SCOPES == {"selected": 1, "visible": 2}
    for lo, hi, bins in ((0.1, 1.3, 7), (-3.7, 11.9, 4096), (0.0, 1.0, 1)):
        assert np.array_equal(gh.attr_edges(lo, hi, bins), ar.edges(lo, hi, bins))
    import inspect
    sig = inspect.signature(gh.HIPRenderer.attr_stats)
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, False, False]
    sig = inspect.signature(gh.HIPRenderer.attr_histogram)
    assert list(sig.parameters)[1:] == ["attr", "lo", "hi", "bins", "origin", "selected", "visible"]
    sig = inspect.signature(gh.HIPRenderer.select_attr)
    assert [p.default for p in list(sig.parameters.values())[2:]] == [-np.inf, np.inf, None, "replace"]

"""HIPRenderer's cluster methods without a GPU (tests/js/cluster_binding_check.js): against a stub native layer the three methods
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
DRIVER = os.path.join(ROOT, "tests", "js", "cluster_binding_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "constants_follow_the_header", "clusters_defaults_scopes_and_result", "select_defaults_are_everything_replace", "below_and_at_least_are_the_size_range",
    "seed_or_largest", "bad_arguments_throw_before_the_addon", "addon_errors_pass_through",
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
    for word in ("this.splatClusters", "this.selectClusters", "this.selectClusterAt", "const CLUSTER_LARGEST = 0xffffffff;"):
        assert word in src, word
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("splatClusters(radius: number, options?: ClusterOptions): SplatClusters;",
                 "selectClusters(radius: number, options?: ClusterOptions & { below?: number; atLeast?: number; op?: SelectOp }): number;",
                 "selectClusterAt(radius: number, options: ClusterOptions & { seed?: number; largest?: boolean; op?: SelectOp }): number;",
                 "export interface ClusterOptions { minPts?: number; scope?: NeighbourScope | NeighbourScope[]; budget?: number }",
                 "export interface SplatClusters { labels: Uint32Array; sizes: Uint32Array; inScope: number; nonfinite: number; pairBound: number; core: number; border: number;"):
        assert word in dts, word
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    for name, fn in (("clusters", "Clusters"), ("selectClusters", "SelectClusters"), ("selectClusterAt", "SelectClusterAt")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for call in ("gsr_clusters(c,", "gsr_select_clusters(c,", "gsr_select_cluster_at(c,"):
        assert call in addon, call
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "const p = renderer.pick(x, y); renderer.selectClusterAt(0.05, { seed: p.index })" in readme     # the island under the cursor


def test_python_host_has_the_same_constants_and_signatures():
    import gsplat_hip as gh
    import cluster_reference as cr
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    words = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define GSR_CLUSTER_(NONE|LARGEST)\s+(0x[0-9a-f]+)u", header)}
    assert words == {"NONE": gh.CLUSTER_NONE, "LARGEST": gh.CLUSTER_LARGEST} == {"NONE": cr.NONE, "LARGEST": cr.LARGEST}
    assert cr.MAX_MIN_PTS == gh.NEIGHBOUR_MAX_CAP
    sig = inspect.signature(gh.HIPRenderer.clusters)
    assert list(sig.parameters)[1:] == ["radius", "min_pts", "scope", "budget", "labels", "sizes"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [0, (), None, True, True]
    sig = inspect.signature(gh.HIPRenderer.select_clusters)
    assert list(sig.parameters)[1:] == ["radius", "lo", "hi", "min_pts", "scope", "op", "budget"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [0, None, 0, (), "replace", None]
    sig = inspect.signature(gh.HIPRenderer.select_cluster_at)
    assert list(sig.parameters)[1:] == ["radius", "seed", "min_pts", "scope", "op", "budget"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [0, (), "replace", None]
    for bad in (-1, 4096):
        with pytest.raises(ValueError):
            gh.HIPRenderer._cluster_args(1.0, bad, None)
    assert gh.HIPRenderer._cluster_args(1, 0, None) == (1.0, 0, 0) and gh.HIPRenderer._cluster_args(0.5, 4095, 7) == (0.5, 4095, 7)
    assert [f[0] for f in gh.GsrClusterInfo._fields_] == ["in_scope", "nonfinite", "pair_bound", "budget", "core", "border", "noise", "clusters", "largest_label",
                                                         "largest_size"]

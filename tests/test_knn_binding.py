"""HIPRenderer's k-nearest-neighbour methods without a GPU (tests/js/knn_binding_check.js): against a stub native layer the three
methods reach the addon with the header's flags and the documented defaults, the outlier threshold is the mean plus the ratio
times the sample standard deviation of the finite values, bad arguments throw before the addon, the addon's refusals pass through;
renderer, typings and addon table carry the names, and the Python host has the same constants and signatures."""
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "knn_binding_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "constants_follow_the_header", "knn_defaults_scopes_and_result", "select_defaults_are_everything_replace", "select_passes_the_range_the_stat_and_the_op",
    "outliers_read_the_mean_and_select_above_the_threshold", "bad_arguments_throw_before_the_addon", "addon_errors_pass_through",
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
    for word in ("this.splatKnn", "this.selectKnn", "this.selectStatisticalOutliers", "{ kth: 0, mean: 1 }"):
        assert word in src, word
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("splatKnn(radius: number, options?: KnnOptions & { lists?: boolean }): SplatKnn;",
                 "selectKnn(radius: number, options?: KnnOptions & { lo?: number; hi?: number; op?: SelectOp }): number;",
                 "selectStatisticalOutliers(radius: number, options?: { k?: number; stdRatio?: number; scope?: NeighbourScope | NeighbourScope[]; budget?: number; "
                 "op?: SelectOp }): { selected: number; threshold: number };",
                 "export interface KnnOptions { k?: number; stat?: KnnStat; scope?: NeighbourScope | NeighbourScope[]; budget?: number }",
                 "export interface SplatKnn { found: Uint32Array; values: Float64Array; hist: Uint32Array; idx?: Uint32Array; d2?: Float64Array;",
                 'export type KnnStat = "kth" | "mean";'):
        assert word in dts, word
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    for name, fn in (("knn", "Knn"), ("selectKnn", "SelectKnn")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for call in ("gsr_knn(c,", "gsr_select_knn(c,"):
        assert call in addon, call
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "renderer.selectStatisticalOutliers(0.1, { k: 8, stdRatio: 2 }); scene.eraseSelection(renderer.readSelection());" in readme


def test_python_host_has_the_same_constants_and_signatures():
    import gsplat_hip as gh
    import knn_reference as kr
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert int(re.search(r"#define GSR_KNN_MAX_K (\d+)u", header).group(1)) == gh.KNN_MAX_K == kr.MAX_K == 32
    assert int(re.search(r"#define GSR_KNN_NONE\s+(0x[0-9a-f]+)u", header).group(1), 16) == gh.KNN_NONE == kr.NONE
    stats = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define GSR_KNN_(KTH|MEAN)\s+(\d+)", header)}
    assert stats == gh.KNN_STATS == kr.STATS == {"kth": 0, "mean": 1}
    sig = inspect.signature(gh.HIPRenderer.knn)
    assert list(sig.parameters)[1:] == ["radius", "k", "stat", "scope", "budget", "found", "idx", "d2", "values", "hist"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [8, "mean", (), None, True, False, False, True, True]
    sig = inspect.signature(gh.HIPRenderer.select_knn)
    assert list(sig.parameters)[1:] == ["radius", "k", "stat", "lo", "hi", "scope", "op", "budget"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [8, "mean", 0.0, None, (), "replace", None]
    sig = inspect.signature(gh.HIPRenderer.select_statistical_outliers)
    assert list(sig.parameters)[1:] == ["radius", "k", "std_ratio", "scope", "op"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [8, 2.0, (), "replace"]
    for bad in (0, 33):
        with pytest.raises(ValueError):
            gh.HIPRenderer._knn_args(1.0, bad, "mean", None)
    with pytest.raises(ValueError):
        gh.HIPRenderer._knn_args(1.0, 8, "median", None)
    with pytest.raises(ValueError):
        gh.HIPRenderer._knn_args(1.0, 8, "mean", -1)
    assert gh.HIPRenderer._knn_args(1, 32, "kth", None) == (1.0, 32, 0, 0)
    assert [f[0] for f in gh.GsrKnnInfo._fields_] == ["in_scope", "nonfinite", "pair_bound", "budget", "complete", "finite_values", "value_min", "value_max"]
    info = gh.GsrKnnInfo(value_min=float("inf"), value_max=float("-inf")).as_dict()
    assert info["value_min"] == np.inf and info["value_max"] == -np.inf and isinstance(info["complete"], int)
    v = np.array([1.0, 2.0, 3.0, np.inf, np.nan, 6.0])
    assert gh.knn_outlier_threshold(v, 2.0) == kr.outlier_threshold(v, 2.0) == pytest.approx(3.0 + 2.0 * np.sqrt(14.0 / 3.0), rel=1e-15)
    assert gh.knn_outlier_threshold(np.array([1.0, np.inf]), 2.0) == np.inf

"""k nearest neighbours through the Node host, on the GPU (tests/js/knn_device_check.js, in a fresh child process): on the cluster
scene and on the coincident scene the lists, the values of both stats, the histogram, the info block and the selections that
splatKnn / selectKnn / selectStatisticalOutliers return are the Python host's for the same rows, bit for bit and word for word,
and both are the reference's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_reference as ar
import knn_reference as kr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "knn_device_check.js")
NODE = shutil.which("node")
SCENES = {"cluster": "clusters and floaters, k 8", "coincident": "300 coincident, k 7"}

EXPECTED = [name + check for name in SCENES for check in ("_results_have_the_types_and_the_sizes", "_the_histogram_sums_to_the_scope",
                                                          "_infinite_values_follow_the_upper_end", "_outliers_are_the_values_at_or_above_the_threshold")]
EXPECTED.append("the_library_refusals_reach_the_caller")


def _rows(p, seed=9):
    """32 bytes per splat: position, scale, colour and rotation bytes"""
    n = p.shape[0]
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 8), np.float32)
    rows[:, 0:3] = p
    rows[:, 3:6] = rng.uniform(0.02, 0.1, (n, 3))
    raw = rows.view(np.uint8).reshape(n, 32)
    raw[:, 24:32] = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    return raw.reshape(-1)


def _bits(a):
    return [str(v) for v in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64).tolist()]


def test_node_host_equals_the_python_host(tmp_path):
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    by_name = {f[0]: f for f in kr.families()}
    args = []
    for name, family in SCENES.items():
        _, p, radius, k = by_name[family]
        _rows(p).tofile(os.path.join(str(tmp_path), name + ".bin"))
        args += [repr(float(radius)), str(k)]
    r = subprocess.run([NODE, DRIVER, str(tmp_path)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checks"] == EXPECTED
    assert out["failed"] == []

    import gsplat_hip as gh
    py = gh.HIPRenderer(out["width"], out["height"])
    try:
        for name, family in SCENES.items():
            _, p, radius, k = by_name[family]
            js = out["scenes"][name]
            n = p.shape[0]
            assert (js["n"], js["radius"], js["k"]) == (n, radius, k)
            py.set_scene_rows(np.fromfile(os.path.join(str(tmp_path), name + ".bin"), dtype=np.uint8))
            py.set_hidden(None)
            pos = py.read_scene()[1]
            wf, wi, wd = kr.lists(pos, radius, k)
            found, idx, d2, mean, hist, info = py.knn(radius, k=k, idx=True, d2=True)
            kth, kinfo = [py.knn(radius, k=k, stat="kth")[t] for t in (3, 5)]
            assert js["found"] == found.tolist() == wf.tolist() and js["idx"] == idx.reshape(-1).tolist() == wi.reshape(-1).tolist()
            assert js["d2"] == _bits(d2) == _bits(wd)
            assert js["mean"] == _bits(mean) == _bits(kr.values(wf, wd, k, "mean")) and js["kth"] == _bits(kth) == _bits(kr.values(wf, wd, k, "kth"))
            assert js["hist"] == hist.tolist() == kr.hist(wf, k).tolist()
            assert js["info"] == [info[key] for key in ("in_scope", "nonfinite", "pair_bound", "complete", "finite_values")]
            assert js["range"] == _bits([info["value_min"], info["value_max"], kinfo["value_min"], kinfo["value_max"]])
            full = kr.select(kr.values(wf, wd, k, "kth"), 0.0, 1e300)
            assert py.select_knn(radius, k=k, stat="kth", hi=1e300)[0] == js["full"] == int(full.sum())
            assert py.selection_words().tolist() == js["fullWords"] == ar.pack(full).tolist()
            hidden = np.arange(n) % 5 == 0
            py.set_hidden(hidden)
            vf, _, vd = kr.lists(pos, radius, k, ~hidden)
            vis = kr.values(vf, vd, k, "mean", ~hidden)
            got = py.knn(radius, k=k, scope="visible")
            assert js["visFound"] == got[0].tolist() == vf.tolist() and js["visMean"] == _bits(got[3]) == _bits(vis)
            # the two hosts sum the finite values in different orders: the thresholds agree to rounding, and each host selects exactly
            # the values at or above its own
            threshold = float(np.array([int(js["threshold"])], np.uint64).view(np.float64)[0])
            mine = kr.outlier_threshold(vis, 1.5, ~hidden)
            assert threshold == mine or abs(threshold - mine) <= 1e-12 * abs(mine)
            after = full | kr.select(vis, threshold, np.inf, ~hidden)
            assert js["outliers"] == int(after.sum()) and js["outWords"] == ar.pack(after).tolist()
            assert py.select_knn(radius, k=k, lo=threshold, scope="visible", op="add")[0] == js["outliers"]
            assert py.selection_words().tolist() == js["outWords"]
    finally:
        py.dispose()

"""Clusters through the Node host, on the GPU (tests/js/cluster_device_check.js, in a fresh child process): the labels, the sizes,
the info and the selections splatClusters / selectClusters / selectClusterAt return are the Python host's for the same rows, number
for number and word for word, and both are the reference's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_reference as ar
import cluster_reference as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "cluster_device_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "results_have_the_types_and_the_sizes", "the_kinds_sum_to_the_scope", "what_the_sizes_show_is_what_the_range_selects", "the_largest_cluster_has_its_size",
    "ops_fold_like_the_selection_calls", "the_library_refusals_reach_the_caller",
]
KEYS = ("in_scope", "nonfinite", "pair_bound", "core", "border", "noise", "clusters", "largest_label", "largest_size")


def test_node_host_equals_the_python_host(tmp_path):
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    r = subprocess.run([NODE, DRIVER, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checks"] == EXPECTED
    assert out["failed"] == []

    import gsplat_hip as gh
    rows = np.fromfile(os.path.join(str(tmp_path), "rows.bin"), dtype=np.uint8)
    n, radius, min_pts = out["n"], out["radius"], out["minPts"]
    py = gh.HIPRenderer(out["width"], out["height"])
    try:
        py.set_scene_rows(rows)
        hidden = np.arange(n) % 5 == 0
        py.set_hidden(hidden)
        pos = py.read_scene()[1]
        want, want_vis = cr.Clusters(pos, radius, min_pts), cr.Clusters(pos, radius, min_pts, ~hidden)
        assert want.info["border"] > 0 and want.info["noise"] > 50 and want.info["clusters"] > 1          # the scattered sixteenth, mostly
        labels, sizes, info = py.clusters(radius, min_pts=min_pts)
        assert out["labels"] == labels.tolist() == want.labels.tolist() and out["sizes"] == sizes.tolist() == want.sizes.tolist()
        assert out["info"] == [info[k] for k in KEYS] and {k: info[k] for k in want.info} == want.info
        labels, sizes, _ = py.clusters(radius, min_pts=min_pts, scope="visible")
        assert out["visLabels"] == labels.tolist() == want_vis.labels.tolist() and out["visSizes"] == sizes.tolist() == want_vis.sizes.tolist()
        small = cr.select(want.sizes, 0, 10)
        assert py.select_clusters(radius, hi=10, min_pts=min_pts)[0] == out["small"] == int(small.sum())
        assert py.selection_words().tolist() == out["words"] == ar.pack(small).tolist()
        largest = cr.select_at(want.labels, cr.LARGEST, want.info["largest_label"])
        assert py.select_cluster_at(radius, "largest", min_pts=min_pts)[0] == out["largest"] == int(largest.sum())
        assert py.selection_words().tolist() == out["largestWords"] == ar.pack(largest).tolist()
        assert py.select_cluster_at(radius, out["seed"], min_pts=min_pts, op="add")[0] == out["at"] == int((largest | cr.select_at(want.labels, out["seed"])).sum())
    finally:
        py.dispose()

"""Neighbours through the Node host, on the GPU (tests/js/neighbour_device_check.js, in a fresh child process): the counts, the
histogram and the floater selection splatNeighbours / selectNeighbours return are the Python host's for the same rows, number for
number and word for word, and both are the reference's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_reference as ar
import neighbour_reference as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "neighbour_device_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "results_have_the_types_and_the_sizes", "the_histogram_sums_to_the_scope", "what_the_histogram_shows_is_what_the_range_selects",
    "ops_fold_like_the_selection_calls", "the_library_refusals_reach_the_caller",
]


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
    n, radius, cap = out["n"], out["radius"], out["cap"]
    py = gh.HIPRenderer(out["width"], out["height"])
    try:
        py.set_scene_rows(rows)
        hidden = np.arange(n) % 5 == 0
        py.set_hidden(hidden)
        pos = py.read_scene()[1]
        want, want_vis = nr.counts(pos, radius, cap), nr.counts(pos, radius, cap, ~hidden)
        counts, hist, info = py.neighbours(radius, cap=cap)
        assert out["counts"] == counts.tolist() == want.tolist() and out["hist"] == hist.tolist() == nr.hist(want, cap).tolist()
        assert out["info"] == [info["in_scope"], info["nonfinite"], info["pair_bound"]] and info["pair_bound"] >= nr.pair_floor(pos, radius)
        counts, hist, _ = py.neighbours(radius, cap=cap, scope="visible")
        assert out["visCounts"] == counts.tolist() == want_vis.tolist() and out["visHist"] == hist.tolist() == nr.hist(want_vis, cap, ~hidden).tolist()
        few = nr.select(want, 0, 3)
        assert 50 < few.sum() < n // 4                                     # the scattered sixteenth, mostly
        assert py.select_neighbours(radius, hi=3, cap=cap)[0] == out["few"] == int(few.sum())
        assert py.selection_words().tolist() == out["words"] == ar.pack(few).tolist()
        assert py.select_neighbours(radius, lo=cap, cap=cap, op="add", scope="visible")[0] == out["added"] == int((few | nr.select(want_vis, cap, cap + 1, ~hidden)).sum())
    finally:
        py.dispose()

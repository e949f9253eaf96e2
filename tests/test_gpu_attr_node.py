"""Splat data through the Node host, on the GPU (tests/js/attr_device_check.js, in a fresh child process): the statistics, the
histograms' counters and the range selections splatStats / splatHistogram / selectAttribute return are the Python host's for the
same rows, number for number and word for word, and both are the reference's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_reference as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "attr_device_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "histograms_have_the_types_and_the_sizes", "counters_add_up_to_the_count", "what_the_histogram_shows_is_what_the_range_selects",
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
    n, origin = out["n"], out["origin"]
    py = gh.HIPRenderer(out["width"], out["height"])
    try:
        py.set_scene_rows(rows)
        picked, hidden = np.arange(n) % 3 == 0, np.arange(n) % 5 == 0
        py.set_hidden(hidden)
        data, pos, _, scl = py.read_scene()
        for case in out["results"]:
            attr, lo, hi, bins = case["attr"], case["lo"], case["hi"], case["bins"]
            v = ar.attr_value(attr, data=data, positions=pos, scales=scl, origin=origin)
            for scope, node in enumerate(case["scopes"]):
                py.set_selection(picked)
                count, nan, mn, mx = py.attr_stats(attr, origin=origin, selected=bool(scope & 1), visible=bool(scope & 2))
                counts, outside, edges = py.attr_histogram(attr, lo, hi, bins, origin=origin, selected=bool(scope & 1), visible=bool(scope & 2))
                assert (node["count"], node["nan"], node["min"], node["max"]) == (count, nan, mn, mx), (attr, scope)
                assert node["counts"] == counts.tolist() and (node["below"], node["above"], node["nanOut"]) == outside, (attr, scope)
                mask = ar.in_scope(n, scope, ar.pack(picked), ar.pack(hidden))
                assert (count, nan, mn, mx) == ar.stats(v, mask) and np.array_equal(counts, ar.histogram(v, lo, hi, bins, mask)[0]), (attr, scope)
            a, b = case["range"]
            assert py.select_attr(attr, edges[a], edges[b], origin=origin) == case["selected"] == int(ar.select(v, edges[a], edges[b]).sum())
            assert py.selection_words().tolist() == case["words"], attr
        py.set_selection(picked)
        assert py.select_attr("opacity", hi=32, op="add") == out["added"]
        assert py.select_attr("opacity", lo=200, op="subtract") == out["cut"]
    finally:
        py.dispose()

"""Merging cells through the Node host, on the GPU (tests/js/merge_device_check.js, in a fresh child process): on the cluster scene the
report and the merged device copy that splatCells / mergeCells return are the Python host's for the same rows, word for word, and
both are the reference's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_reference as ar
import merge_reference as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "merge_device_check.js")
NODE = shutil.which("node")
EXPECTED = ["the_report_has_the_types_and_the_sizes", "the_histogram_sums_to_the_cells", "the_edit_does_what_the_report_announced", "the_selection_is_the_merged_rows",
            "the_device_copy_has_the_new_count", "the_merged_scene_renders", "the_library_refusals_reach_the_caller"]
KEYS = ("in_scope", "candidates", "cells", "merged_cells", "merged_members", "largest", "rows_after", "pair_bound")
CELL = 0.08


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


def test_node_host_equals_the_python_host(tmp_path):
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    positions = {f[0]: f for f in mr.families()}["8192 clustered"][1][1][:2048]
    _rows(positions).tofile(os.path.join(str(tmp_path), "cluster.bin"))
    r = subprocess.run([NODE, DRIVER, str(tmp_path), repr(CELL)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checks"] == EXPECTED
    assert out["failed"] == []

    import gsplat_hip as gh
    py = gh.HIPRenderer(out["width"], out["height"])
    try:
        py.set_scene_rows(np.fromfile(os.path.join(str(tmp_path), "cluster.bin"), dtype=np.uint8))
        data, pos, rot, scl = (a.reshape(-1, k) for a, k in zip(py.read_scene(), (8, 3, 4, 3)))
        n = pos.shape[0]
        assert out["n"] == n == 2048 and out["cell"] == CELL
        wl, wh, winfo = mr.report(pos, rot, scl, CELL, 16)
        leader, hist, info = py.cells(CELL, cap=16, leaders=True)
        js = out["report"]
        assert js["leader"] == leader.tolist() == wl.tolist() and js["hist"] == hist.tolist() == wh.tolist()
        assert js["info"] == [info[k] for k in KEYS] and all(info[k] == v for k, v in winfo.items())
        want = mr.merge(data, pos, rot, scl, CELL)
        count, minfo = py.scene_merge_cells(CELL)
        js = out["merged"]
        assert js["count"] == count == want["info"]["rows_after"] and js["info"] == [minfo[k] for k in KEYS]
        assert js["words"] == py.selection_words().tolist() == ar.pack(want["merged"]).tolist()
        got = py.read_scene()
        assert js["data"] == got[0].tolist() == want["data"].reshape(-1).tolist()
        assert js["positions"] == got[1].view(np.uint32).tolist() == want["positions"].reshape(-1).view(np.uint32).tolist()
        assert np.array_equal(got[2].view(np.uint32), want["rotations"].reshape(-1).view(np.uint32))
        assert np.array_equal(got[3].view(np.uint32), want["scales"].reshape(-1).view(np.uint32))
        assert js["again"] == [py.cells(CELL)[2][k] for k in KEYS]
    finally:
        py.dispose()

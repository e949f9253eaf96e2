"""Planes through the Node host, on the GPU (tests/js/plane_device_check.js, in a fresh child process): what fitPlane, selectPlane,
planeInliers and planeAlignment return, and what scene.rotate / scene.translate leave on the device, are the Python host's for the
same bytes -- the 8192-splat family of tests/plane_reference.py as .splat rows -- number for number and word for word, and both are
the reference's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_reference as ar
import plane_reference as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "plane_device_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "the_fit_has_the_types_and_the_sizes", "the_winner_has_the_largest_score_and_the_smallest_index", "what_the_fit_counted_is_what_the_interval_selects",
    "the_three_intervals_cover_the_scene", "the_scoring_pass_alone_agrees", "the_alignment_is_a_unit_quaternion", "the_floor_lies_at_y_0",
    "the_library_refusals_reach_the_caller",
]


def _rows(p):
    """.splat rows around the positions p: 3 f32 position, 3 f32 scale, 4 bytes colour, 4 bytes rotation"""
    n = p.shape[0]
    rng = np.random.default_rng(5)
    rows = np.zeros((n, 32), np.uint8)
    f = rows.view(np.float32)
    f[:, 0:3] = p
    f[:, 3:6] = rng.uniform(0.02, 0.12, (n, 3)).astype(np.float32)
    rows[:, 24:32] = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    return rows.reshape(-1)


def test_node_host_equals_the_python_host(tmp_path):
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    p, _, _ = pr.floor_scene()
    rows = _rows(p)
    rows.tofile(os.path.join(str(tmp_path), "rows.bin"))
    r = subprocess.run([NODE, DRIVER, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checks"] == EXPECTED
    assert out["failed"] == []

    import gsplat_hip as gh
    t, h = out["threshold"], out["hypotheses"]
    assert (out["n"], t, h) == (pr.FLOOR_N, pr.FLOOR_THRESHOLD, pr.FLOOR_HYPOTHESES)
    py = gh.HIPRenderer(out["width"], out["height"])
    try:
        py.set_scene_rows(rows)
        pos = py.read_scene()[1].reshape(-1, 3)
        assert np.array_equal(pos.view(np.uint32), p.view(np.uint32))
        want, wsc = pr.fit(pos, t, h)
        plane, info, sc = py.fit_plane(t, hypotheses=h, scores=True)
        assert out["scores"] == sc.tolist() == wsc.tolist()
        assert out["plane"] == plane.tolist() == want["plane"].tolist()
        assert (out["best"], tuple(out["triple"]), out["inliers"], out["degenerate"], out["nonfinite"]) == \
               (info["best"], info["triple"], info["inliers"], info["degenerate"], info["nonfinite"]) == \
               (want["best"], want["triple"], want["inliers"], want["degenerate"], want["nonfinite"])
        picked = pr.select(pos, plane, -t, t)
        assert py.select_plane(plane, within=t) == out["within"] == int(picked.sum()) == info["inliers"]
        assert py.selection_words().tolist() == out["words"] == ar.pack(picked).tolist()
        under, over = pr.select(pos, plane, -np.inf, -t), pr.select(pos, plane, t, np.inf)
        assert py.select_plane(plane, hi=-t) == out["under"] == int(under.sum())
        assert py.select_plane(plane, lo=t, op="add") == out["over"] == int((under | over).sum())
        assert py.plane_inliers([plane, (0, 1, 0, 0)], t).tolist() == out["own"]
        q, tr = py.plane_alignment(plane)
        wq, wt = pr.alignment(plane)
        assert out["q"] == q.tolist() == wq.tolist() and out["t"] == tr.tolist() == wt.tolist()
        py.scene_rotate(q)
        py.scene_translate(tr)
        after = int(py.plane_inliers([(0, 1, 0, 0)], t + 2.0 ** -19)[0])
        assert after == out["after"] >= info["inliers"]
    finally:
        py.dispose()

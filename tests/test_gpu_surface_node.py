"""Point-to-plane registration through the Node host, on the GPU (tests/js/surface_device_check.js, in a fresh child process): what
registerTo with residual "surface", matchSurface and SPLAT.surfaceSolve return are the Python host's for the same bytes -- the box
corner of tests/surface_reference.py as .splat rows -- bit for bit, both are the reference's, and residual "point" is registerTo
as it was."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import normal_reference as nref
import register_reference as rr
import surface_reference as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "surface_device_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "residual_point_is_the_call_without_it", "the_surface_registration_converged_in_fewer_steps", "rotation_and_translation_are_the_decomposition",
    "own_normals_are_the_default_and_the_same_call_gives_the_same_bits", "knn_normals_converge_too", "one_step_as_data", "the_pure_solve_is_the_first_step",
    "the_scene_was_not_written", "the_refusals_reach_the_caller",
]


def _rows(p, rotations, seed):
    """.splat rows around the positions p: 3 f32 position, 3 f32 scale, 4 bytes colour, 4 bytes rotation ((r + 1) * 128, so that the
    corner's +-0.5 and 0 are stored exactly)"""
    n = p.shape[0]
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 32), np.uint8)
    f = rows.view(np.float32)
    f[:, 0:3] = p
    f[:, 3:6] = sr.FACE_SCALES
    rows[:, 24:28] = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    rows[:, 28:32] = np.clip(rotations.astype(np.float64) * 128.0 + 128.0, 0, 255).astype(np.uint8)
    return rows.reshape(-1)


def _bits(a):
    return [str(v) for v in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)]


def test_node_host_equals_the_python_host(tmp_path):
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    c = sr.corner_scenario()
    src, tgt = c["source"], c["target"]
    srows, trows = _rows(src, c["source_rotations"], 5), _rows(tgt, c["target_rotations"], 6)
    srows.tofile(os.path.join(str(tmp_path), "source.bin"))
    trows.tofile(os.path.join(str(tmp_path), "target.bin"))
    r = subprocess.run([NODE, DRIVER, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checks"] == EXPECTED
    assert out["failed"] == []

    import gsplat_hip as gh
    radius, steps, tol = out["radius"], out["steps"], 2.0 ** -30
    assert (out["n"], radius) == (src.shape[0], sr.RADIUS)
    a, b = gh.HIPRenderer(out["width"], out["height"]), gh.HIPRenderer(out["width"], out["height"])
    try:
        a.set_scene_rows(srows)
        b.set_scene_rows(trows)
        _, pos, rot, scl = b.read_scene()
        assert np.array_equal(pos.view(np.uint32), tgt.reshape(-1).view(np.uint32))
        nrm = nref.own_normals(pos, rot, scl)[0]
        assert np.array_equal(nrm, c["target_normals"])                # the stored bytes give the faces' normals exactly
        # residual "point" is today's path
        wP, wpoint = rr.register(src, tgt, radius, None, max_iterations=steps, tolerance=tol)
        P, point = a.register(b, radius, max_iterations=steps, tolerance=tol)
        assert out["pointTransform"] == _bits(P) == _bits(wP)
        assert (out["pointStatus"], out["pointIterations"]) == (point["status"], point["iterations"]) == (gh.REGISTER_STATUS[wpoint["status"]], wpoint["iterations"])
        # residual "surface"
        wM, want = sr.register_surface(src, tgt, nrm, radius, max_iterations=steps, tolerance=tol)
        M, info = a.register_surface(b, radius, normals={"source": "own"}, max_iterations=steps, tolerance=tol, history=True)
        assert out["transform"] == _bits(M) == _bits(wM)
        assert (out["status"], out["iterations"], out["pairs"], out["surfacePairs"], out["valid"]) == \
               (info["status"], info["iterations"], info["pairs"], info["surface_pairs"], info["valid"]) == \
               ("converged", want["iterations"], want["pairs"], want["surface_pairs"], tgt.shape[0])
        assert out["rms"] == _bits([info["rms"], info["surface_rms"], info["delta"]]) == _bits([want["rms"], want["surface_rms"], want["delta"]])
        assert out["stepPairs"] == info["step_pairs"].tolist() == want["step_pairs"]
        assert out["stepSurfacePairs"] == info["step_surface_pairs"].tolist() == want["step_surface_pairs"]
        assert out["stepRms"] == _bits(info["step_rms"]) == _bits(want["step_rms"])
        assert out["stepSurfaceRms"] == _bits(info["step_surface_rms"]) == _bits(want["step_surface_rms"])
        assert out["q"] == _bits(gh.rigid_decompose(M)[0]) == _bits(rr.rigid_decompose(wM)[0])
        kn = out["knn"]
        knn = nref.knn_normals(pos, kn["radius"], kn["k"])[0]
        wK, wknn = sr.register_surface(src, tgt, knn, radius, max_iterations=steps, tolerance=tol)
        K, kinfo = a.register_surface(b, radius, normals=kn, max_iterations=steps, tolerance=tol)
        assert out["knnTransform"] == _bits(K) == _bits(wK)
        assert (out["knnIterations"], out["knnValid"]) == (kinfo["iterations"], kinfo["valid"]) == (wknn["iterations"], int((~np.isnan(knn[:, 0])).sum()))
        # one step as data, and the pure solve
        sums, minfo = a.match_surface(b, radius, normals={"source": "own"})
        idx, d2, winfo = rr.match(src, tgt, radius)
        wpairs, wsurface, ws29 = sr.sums(src, tgt, nrm, idx, d2)
        assert out["sums"] == _bits(sums["sum"]) == _bits(ws29) and out["sumPairs"] == [sums["pairs"], sums["surface_pairs"]] == [wpairs, wsurface]
        keys = ("in_scope", "nonfinite", "target_indexed", "matched", "pair_bound")
        assert out["info"] == [minfo[k] for k in keys] == [winfo[k] for k in keys]
        assert out["solved"] == _bits(gh.surface_solve(sums)[0]) == _bits(sr.surface_solve(wsurface, ws29)[0])
    finally:
        a.dispose()
        b.dispose()

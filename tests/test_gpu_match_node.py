"""Matching and registration through the Node host, on the GPU (tests/js/register_device_check.js, in a fresh child process): what
matchScene, selectMatch, registerTo and rigidDecompose return, and what scene.rotate / scene.translate leave on the device, are
the Python host's for the same bytes -- the noiseless scenario of tests/register_reference.py as .splat rows -- bit for bit and
word for word, and both are the reference's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_reference as ar
import register_reference as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "register_device_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "the_match_has_the_types_and_the_sizes", "unmatched_rows_hold_none_and_infinity", "has_and_lacks_cover_the_scene", "the_registration_converged",
    "rotation_and_translation_are_the_decomposition", "the_scene_was_not_written", "applied_once_the_partners_coincide", "the_refusals_reach_the_caller",
]


def _rows(p, seed):
    """.splat rows around the positions p: 3 f32 position, 3 f32 scale, 4 bytes colour, 4 bytes rotation"""
    n = p.shape[0]
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 32), np.uint8)
    f = rows.view(np.float32)
    f[:, 0:3] = p
    f[:, 3:6] = rng.uniform(0.02, 0.12, (n, 3)).astype(np.float32)
    rows[:, 24:32] = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    return rows.reshape(-1)


def _bits(a):
    return [str(v) for v in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)]


def test_node_host_equals_the_python_host(tmp_path):
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    src, tgt, partner = rr.scenario(False)
    srows, trows = _rows(src, 5), _rows(tgt, 6)
    srows.tofile(os.path.join(str(tmp_path), "source.bin"))
    trows.tofile(os.path.join(str(tmp_path), "target.bin"))
    r = subprocess.run([NODE, DRIVER, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checks"] == EXPECTED
    assert out["failed"] == []

    import gsplat_hip as gh
    radius, steps = out["radius"], out["steps"]
    assert (out["n"], radius) == (src.shape[0], rr.RADIUS)
    a, b = gh.HIPRenderer(out["width"], out["height"]), gh.HIPRenderer(out["width"], out["height"])
    try:
        a.set_scene_rows(srows)
        b.set_scene_rows(trows)
        assert np.array_equal(a.read_scene()[1].view(np.uint32), src.reshape(-1).view(np.uint32))
        widx, wd2, winfo = rr.match(src, tgt, radius)
        wpairs, wsum = rr.sums(src, tgt, widx, wd2)
        idx, d2, sums, info = a.match(b, radius, sums=True)
        assert out["idx"] == idx.tolist() == widx.tolist()
        assert out["d2"] == _bits(d2) == _bits(wd2)
        assert out["sums"] == _bits(sums["sum"]) == _bits(wsum) and out["pairs"] == sums["pairs"] == wpairs
        assert out["info"] == [info[k] for k in ("in_scope", "nonfinite", "target_indexed", "matched", "pair_bound")] == \
               [winfo[k] for k in ("in_scope", "nonfinite", "target_indexed", "matched", "pair_bound")]
        assert out["d2MinMax"] == _bits([info["d2_min"], info["d2_max"]]) == _bits([winfo["d2_min"], winfo["d2_max"]])
        picked = rr.select(wd2, 0.0, radius)
        assert a.select_match(b, radius, hi=radius)[0] == out["has"] == int(picked.sum())
        assert a.selection_words().tolist() == out["hasWords"] == ar.pack(picked).tolist()
        assert a.select_match(b, radius, lo=radius)[0] == out["lacks"] == int(rr.select(wd2, radius, None).sum())
        wM, wreg = rr.register(src, tgt, radius, None, max_iterations=steps)
        M, reg = a.register(b, radius, max_iterations=steps, history=True)
        assert out["transform"] == _bits(M) == _bits(wM)
        assert (out["status"], out["iterations"], out["fitPairs"]) == (reg["status"], reg["iterations"], reg["pairs"]) == ("converged", wreg["iterations"], wreg["pairs"])
        assert out["rms"] == _bits([reg["rms"]]) == _bits([wreg["rms"]])
        assert out["stepPairs"] == reg["step_pairs"].tolist() == wreg["step_pairs"] and out["stepRms"] == _bits(reg["step_rms"]) == _bits(wreg["step_rms"])
        q, t = gh.rigid_decompose(M)
        wq, wt = rr.rigid_decompose(wM)
        assert out["q"] == _bits(q) == _bits(wq) and out["t"] == _bits(t) == _bits(wt)
        a.scene_rotate(q)
        a.scene_translate(t)
        idx2, _, _, info2 = a.match(b, 2.0 ** -17)
        assert out["afterIdx"] == idx2.tolist() and out["afterMatched"] == info2["matched"] == rr.PARTNERS
        assert np.array_equal(idx2[:rr.PARTNERS], partner.astype(np.uint32))
    finally:
        a.dispose()
        b.dispose()

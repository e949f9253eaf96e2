"""Normals through the Node host, on the GPU (tests/js/normal_device_check.js, in a fresh child process): on the cluster scene and on
the sphere the normals of both sources, the variation, the list lengths, the info block and the selections that splatNormals /
selectNormal return are the Python host's for the same rows, bit for bit and word for word, and both are the reference's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_reference as ar
import knn_reference as kr
import normal_reference as nm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "normal_device_check.js")
NODE = shutil.which("node")
SCENES = {"cluster": "clusters and floaters, k 8", "sphere": "sphere, k 12"}
TOWARD = (0.3, -2.0, 0.7)
UP = (0.1, 1.0, -0.2)

EXPECTED = [name + check for name in SCENES for check in ("_results_have_the_types_and_the_sizes", "_valid_rows_are_counted_and_oriented",
                                                          "_the_picker_is_the_rule_on_the_returned_arrays", "_a_hidden_splat_has_no_normal")]
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


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32).tolist()


def test_node_host_equals_the_python_host(tmp_path):
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    by_name = {f[0]: f for f in nm.families()}
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
            _, pos, rot, scl = py.read_scene()[:4]
            lists = kr.lists(pos, radius, k)
            wn, wv, wf = nm.knn_normals(pos, radius, k, lists=lists)
            normals, variation, found, info = py.normals(radius, k=k)
            assert js["normals"] == _bits32(normals) == _bits32(wn) and js["variation"] == _bits(variation) == _bits(wv)
            assert js["found"] == found.tolist() == wf.tolist()
            facing = py.normals(radius, k=k, toward=TOWARD)[0]
            assert js["facing"] == _bits32(facing) == _bits32(nm.knn_normals(pos, radius, k, toward=TOWARD, lists=lists)[0])
            on, ov, _ = nm.own_normals(pos, rot, scl)
            own = py.normals(source="own")
            assert js["own"] == _bits32(own[0]) == _bits32(on) and js["ownVariation"] == _bits(own[1]) == _bits(ov)
            assert js["info"] == [info[key] for key in ("in_scope", "nonfinite", "pair_bound", "valid")] + [own[3]["valid"]]
            assert js["range"] == _bits([info["variation_min"], info["variation_max"]])
            walls = nm.select(wn, wv, "abs_dot", -np.inf, 0.25, UP)
            assert py.select_normal("abs_dot", hi=0.25, axis=UP, radius=radius, k=k)[0] == js["walls"] == int(walls.sum())
            assert py.selection_words().tolist() == js["wallWords"] == ar.pack(walls).tolist()
            mid = (info["variation_min"] + info["variation_max"]) / 2
            flat = walls & nm.select(wn, wv, "variation", 0.0, mid)
            assert py.select_normal("variation", lo=0.0, hi=mid, radius=radius, k=k, op="intersect")[0] == js["flat"] == int(flat.sum())
            assert py.selection_words().tolist() == js["flatWords"] == ar.pack(flat).tolist()
            hidden = np.arange(n) % 5 == 0
            py.set_hidden(hidden)
            vn, _, vf = nm.knn_normals(pos, radius, k, ~hidden)
            got = py.normals(radius, k=k, scope="visible")
            assert js["visNormals"] == _bits32(got[0]) == _bits32(vn) and js["visFound"] == got[2].tolist() == vf.tolist()
            hn, hv, _ = nm.own_normals(pos, rot, scl, ~hidden)
            after = flat | nm.select(hn, hv, "dot", 0.0, np.inf, UP)
            assert py.select_normal("dot", lo=0.0, axis=UP, source="own", scope="visible", op="add")[0] == js["ownSelected"] == int(after.sum())
            assert py.selection_words().tolist() == js["ownWords"] == ar.pack(after).tolist()
    finally:
        py.dispose()

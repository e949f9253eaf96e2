"""Growing the scene in the Node host, without a GPU: Scene.duplicateSelection / Scene.append against recording stub device scenes
(tests/js/append_binding_check.js: once per distinct device copy, the mask before the duplicate, vertexCount and the mirrors follow,
"change" as a device edit, the fall-back, the SH refusal), the unbound host loops against tests/append_reference.py bit for bit, and
the Node renderer, typings, addon table and the C ABI benchmark carry the names."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import append_reference as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "gsplat.js_amd", "js")
DRIVER = os.path.join(ROOT, "tests", "js", "append_binding_check.js")
NODE = shutil.which("node")
NAMES_C = ("gsr_scene_reserve", "gsr_scene_capacity", "gsr_scene_duplicate_selected", "gsr_scene_append_selected", "gsr_scene_append_arrays")
N, M = 3000, 257
Q0, S0 = (0.1, -0.3, 0.2, 0.9273618495495703), (1.25, 0.8, 1.1)

EXPECTED = [
    "mask_reaches_each_distinct_copy_once_before_the_duplicate", "both_copies_hold_the_mask", "duplicate_returns_first_and_count",
    "vertex_count_and_height_follow", "change_fires_as_a_device_edit", "mirrors_went_stale_and_refresh_from_a_member",
    "append_reaches_each_distinct_copy_once", "append_hands_over_the_four_arrays", "append_returns_first_and_count",
    "every_call_fired_change_as_a_device_edit", "short_mask_throws", "not_a_mask_throws", "append_needs_another_scene", "an_empty_mask_adds_nothing",
    "device_without_the_methods_falls_back_to_the_host_loop", "sh_rows_refuse_duplicate_and_append", "sh_rows_refuse_before_any_device_call",
    "the_other_scenes_sh_rows_are_not_carried",
]


@pytest.fixture(scope="module")
def protocol():
    if NODE is None:
        pytest.skip("node is not installed")
    r = subprocess.run([NODE, DRIVER, "protocol"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_driver_ran_every_check(protocol):
    assert protocol["checks"] == EXPECTED


@pytest.mark.parametrize("name", EXPECTED)
def test_protocol(protocol, name):
    assert name in protocol["checks"] and name not in protocol["failed"]


def _state(oracle, rows):
    st = oracle.SceneState(rows)
    st.rotate(Q0)
    st.scale(S0)
    return st


def test_unbound_host_loops_equal_the_reference_bit_for_bit(oracle, tmp_path):
    if NODE is None:
        pytest.skip("node is not installed")
    import gsplat_hip as gh
    rows, other = gh.synth.synth_rows(N, 17), gh.synth.synth_rows(M, 5)
    rows_path, other_path, out_path = tmp_path / "rows.splat", tmp_path / "other.splat", tmp_path / "out.bin"
    rows_path.write_bytes(np.ascontiguousarray(rows, dtype=np.uint8).tobytes())
    other_path.write_bytes(np.ascontiguousarray(other, dtype=np.uint8).tobytes())
    r = subprocess.run([NODE, DRIVER, "host", str(rows_path), str(other_path), str(out_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    info = json.loads(r.stdout)
    st, src = _state(oracle, rows), _state(oracle, other)
    for row, k, word in ((1, 1, 0x7fc01234), (4, 0, 0x80000000)):     # the driver's NaN and -0.0, in data as in positions
        st.positions.view(np.uint32)[3 * row + k] = word
        st.data[8 * row + k] = word
    sel = (7 * np.arange(N) + 3) % 5 < 2
    assert sel[1] and sel[4]
    got = np.frombuffer(out_path.read_bytes(), dtype=np.uint32)
    at = 0
    for step, grow in (("duplicate", lambda: ar.duplicate(st, sel)), ("append", lambda: ar.append_selected(st, src, np.ones(M, dtype=bool)))):
        want = grow()
        assert (info["dup" if step == "duplicate" else "app"]) == {"first": want[0], "count": want[1]}, step
        for field, words in (("data", 8), ("positions", 3), ("rotations", 4), ("scales", 3)):
            ref = getattr(st, field).view(np.uint32)[:words * st.n]
            assert np.array_equal(got[at:at + words * st.n], ref), "%s: %s differs" % (step, field)
            at += words * st.n
    assert at == got.size
    k = int(sel.sum())
    assert info["n"] == N and info["m"] == M and info["count"] == N + k + M == st.n and info["changes"] == 2
    assert info["height"] == -(-2 * st.n // 2048) and info["dataLength"] == 2048 * info["height"] * 4


def test_renderer_typings_addon_and_bench_carry_the_names():
    src = open(os.path.join(JS, "renderers", "HIPRenderer.js")).read()
    for word in ("this.reserveScene = (rows)", "this.sceneCapacity = ()", "this.duplicateSelection = ()", "this.appendSelectionFrom = (other)",
                 "duplicateSelected: ()", "appendArrays: (data, positions, rotations, scales, m)"):
        assert word in src, word
    scene = open(os.path.join(JS, "core", "Scene.js")).read()
    for word in ("duplicateSelection(mask)", "append(other)", "this._editDevices(9,", "this._editDevices(10,", "d.duplicateSelected()", "d.appendArrays("):
        assert word in scene, word
    dts = open(os.path.join(JS, "index.d.ts")).read()
    for word in ("reserveScene(rows: number): void;", "sceneCapacity(): number;", "duplicateSelection(): GrownRange;", "appendSelectionFrom(other: HIPRenderer): GrownRange;",
                 "duplicateSelection(mask: Uint32Array): GrownRange;", "append(other: Scene): GrownRange;", "duplicateSelected?(): number;",
                 "appendArrays?(data: Uint32Array, positions: Float32Array, rotations: Float32Array, scales: Float32Array, m: number): number;",
                 "export interface GrownRange { first: number; count: number }"):
        assert word in dts, word
    addon = open(os.path.join(JS, "native", "addon.cc")).read()
    for name, fn in (("reserveScene", "ReserveScene"), ("sceneCapacity", "SceneCapacity"), ("duplicateSelected", "DuplicateSelected"),
                     ("appendSelected", "AppendSelected"), ("appendArrays", "AppendArrays")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for fn in NAMES_C:
        assert fn + "(" in addon, fn
    bench = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    assert '"--duplicate"' in bench and '"--reserve"' in bench and "gsr_scene_duplicate_selected(" in bench and "gsr_scene_reserve(" in bench and '\\"duplicate_ms\\"' in bench

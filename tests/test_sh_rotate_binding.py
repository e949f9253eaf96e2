"""Rotating SH coefficients in the hosts, without a GPU: the Python methods' arguments, SPLAT.shRotation and the Scene's stale
shs_rgb mirror (tests/js/sh_rotate_binding_check.js), and the Node renderer, typings, addon table and the C ABI benchmark carry the
names -- in the manner of tests/test_edit_binding.py."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import sh_rotate_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "gsplat.js_amd", "js")
DRIVER = os.path.join(ROOT, "tests", "js", "sh_rotate_binding_check.js")
NODE = shutil.which("node")
NAMES_C = ("gsr_sh_rotation", "gsr_scene_rotate_sh", "gsr_scene_rotate_selected_sh", "gsr_scene_bake_sh_frame")
Q, PIVOT = (-0.2, 0.5, 0.1, 0.8366600265340756), (0.3, -0.7, 1.9)

EXPECTED = [
    "three_row_major_matrices", "a_quaternion_and_a_typed_array_pass", "the_identity_is_exact", "a_bad_quaternion_throws", "the_addon_checks_its_arguments",
    "a_scene_without_the_mark_reads_nothing", "the_mirror_is_read_back_on_its_next_use", "and_only_once", "a_bake_resets_the_scenes_frame",
    "a_scene_without_sh_stays_unmarked",
]


class _Lib:
    """records the calls the Python host makes"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _f64(p, k):
        return None if p is None else tuple(np.ctypeslib.as_array((ctypes.c_double * k).from_address(p)))

    def gsr_scene_rotate_sh(self, ctx, q, scope, rows):
        self.calls.append(("rotate_sh", self._f64(q, 4), scope))
        rows._obj.value = 11
        return 0

    def gsr_scene_rotate_selected_sh(self, ctx, q, pivot):
        self.calls.append(("rotate_selected_sh", self._f64(q, 4), self._f64(pivot, 3)))
        return 0

    def gsr_scene_bake_sh_frame(self, ctx, q):
        self.calls.append(("bake",))
        (ctypes.c_double * 4).from_address(q)[:] = [0.5, -0.5, 0.5, 0.5]
        return 0


def test_python_host_sends_the_specified_arguments():
    import gsplat_hip as gh
    r = object.__new__(gh.HIPRenderer)
    r._L, r._ctx, r._check = _Lib(), None, lambda rc: None
    assert r.scene_rotate_sh(Q) == 11
    assert r.scene_rotate_sh(Q, selected=True) == 11
    assert r.scene_rotate_sh(np.array(Q, dtype=np.float32), True) == 11
    r.scene_rotate_selected_sh(Q)
    r.scene_rotate_selected_sh(Q, PIVOT)
    r.scene_rotate_selected_sh(Q, pivot=(0, 0, 0))           # a pivot of zero is a pivot, not None
    q = r.scene_bake_sh_frame()
    assert q.dtype == np.float64 and list(q) == [0.5, -0.5, 0.5, 0.5]
    q32 = tuple(float(np.float32(v)) for v in Q)
    assert r._L.calls == [("rotate_sh", Q, gh.GSR_SH_ALL), ("rotate_sh", Q, gh.GSR_SH_SELECTED), ("rotate_sh", q32, gh.GSR_SH_SELECTED),
                          ("rotate_selected_sh", Q, None), ("rotate_selected_sh", Q, PIVOT), ("rotate_selected_sh", Q, (0.0, 0.0, 0.0)), ("bake",)]
    with pytest.raises(ValueError):
        r.scene_rotate_sh((1.0, 2.0, 3.0))
    with pytest.raises(ValueError):
        r.scene_rotate_selected_sh(Q, (1.0, 2.0))


@pytest.fixture(scope="module")
def protocol():
    if NODE is None:
        pytest.skip("node is not installed")
    r = subprocess.run([NODE, DRIVER], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_driver_ran_every_check(protocol):
    assert protocol["checks"] == EXPECTED


@pytest.mark.parametrize("name", EXPECTED)
def test_protocol(protocol, name):
    assert name in protocol["checks"] and name not in protocol["failed"]


def test_the_node_host_returns_the_librarys_matrices(protocol):
    import gsplat_hip as gh
    for got, lib, spec in zip(protocol["matrices"], gh.sh_rotation((0.3, -0.2, 0.5, 0.7)), ref.matrices((0.3, -0.2, 0.5, 0.7))):
        assert np.array_equal(np.array(got), lib.reshape(-1))           # the same function through either host
        assert np.abs(np.array(got) - spec.reshape(-1)).max() <= 2.0 ** -40


def test_renderer_typings_addon_and_bench_carry_the_names():
    src = open(os.path.join(JS, "renderers", "HIPRenderer.js")).read()
    for word in ("this.rotateSH = (q, options)", "this.bakeSHFrame = ()", "this.rotateSelection = (q, options)", "options && options.sh",
                 "this._n.rotateSelectedSh(this._h, vec(q, 4), pivotOf(options))", "options && options.selected ? 1 : 0", "shTurned(true)", "shTurned(false)",
                 "activeScene._deviceTurnedSh(baked)", "function shRotation(q)", "module.exports = { HIPRenderer, sortHost, shRotation }"):
        assert word in src, word
    assert "shRotation: shRotation," in open(os.path.join(JS, "index.js")).read()
    scene = open(os.path.join(JS, "core", "Scene.js")).read()
    for word in ("_deviceTurnedSh(baked)", "if (this._shHeight > 0) this._shStale = true;", "if (baked) this._shFrame.set([1, 0, 0, 0, 1, 0, 0, 0, 1]);"):
        assert word in scene, word
    dts = open(os.path.join(JS, "index.d.ts")).read()
    for word in ("options?: { pivot?: Vec3Like; sh?: boolean }): void;", "options?: { selected?: boolean }): number;", "bakeSHFrame(): Quaternion;",
                 "export function shRotation(q: Quaternion | [number, number, number, number] | Float64Array): [Float64Array, Float64Array, Float64Array];"):
        assert word in dts, word
    addon = open(os.path.join(JS, "native", "addon.cc")).read()
    for name, fn in (("shRotation", "ShRotation"), ("rotateSh", "RotateSh"), ("rotateSelectedSh", "RotateSelectedSh"), ("bakeShFrame", "BakeShFrame")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for fn in NAMES_C:
        assert fn + "(" in addon, fn
    bench = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    for word in ('"--rotate-sh"', "gsr_scene_rotate_sh(", "gsr_scene_rotate_selected_sh(", "gsr_set_scene_sh(", '\\"rotate_selected_sh_ms\\"', '\\"rows_selected\\"'):
        assert word in bench, word

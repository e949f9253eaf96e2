"""Editing the selection in the hosts, without a GPU: the Python methods' arguments, Scene.translateSelection / rotateSelection /
scaleSelection / paintSelection against stub device scenes (tests/js/edit_binding_check.js: the mask once per distinct device copy
and before the edit, "change" as a device edit, mirrors, refusals, the fall-back), the unbound host loops against
tests/edit_reference.py bit for bit, and the Node renderer, typings, addon table and the C ABI benchmark carry the names."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import edit_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "gsplat.js_amd", "js")
DRIVER = os.path.join(ROOT, "tests", "js", "edit_binding_check.js")
NODE = shutil.which("node")
NAMES_C = ("gsr_selection_bounds", "gsr_scene_translate_selected", "gsr_scene_rotate_selected", "gsr_scene_scale_selected", "gsr_scene_set_rgba_selected")
N = 3000
Q0, S0 = (0.1, -0.3, 0.2, 0.9273618495495703), (1.25, 0.8, 1.1)
T, Q, S, PIVOT = (0.25, -0.5, 1.0), (-0.2, 0.5, 0.1, 0.8366600265340756), (0.9, 1.2, 1.05), (0.3, -0.7, 1.9)

EXPECTED = [
    "mask_reaches_each_distinct_copy_once_before_the_edit", "both_copies_hold_the_mask", "rotate_passes_xyzw_and_the_pivot_as_f64",
    "change_fires_as_a_device_edit", "mirrors_refresh_from_a_member", "mirrors_refresh_once", "translate_has_no_pivot", "no_pivot_is_null_not_zero",
    "a_vector3_pivot_passes", "paint_sends_the_word_and_the_byte_mask", "absent_channels_are_left_alone", "every_edit_fired_change_as_a_device_edit",
    "short_mask_throws", "not_a_mask_throws", "non_finite_scale_throws", "a_bad_channel_throws", "device_without_the_methods_falls_back_to_the_host_loop",
    "sh_follow_refusal_throws", "translate_and_paint_pass_under_sh_follow", "rotate_passes_with_sh_follow_off", "rotate_passes_without_sh_rows",
]


class _Lib:
    """records the calls the Python host makes"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _f64(p, k):
        return None if p is None else tuple(np.ctypeslib.as_array((ctypes.c_double * k).from_address(p)))

    def gsr_scene_translate_selected(self, ctx, t):
        self.calls.append(("translate", self._f64(t, 3)))
        return 0

    def gsr_scene_rotate_selected(self, ctx, q, pivot):
        self.calls.append(("rotate", self._f64(q, 4), self._f64(pivot, 3)))
        return 0

    def gsr_scene_scale_selected(self, ctx, s, pivot):
        self.calls.append(("scale", self._f64(s, 3), self._f64(pivot, 3)))
        return 0

    def gsr_scene_set_rgba_selected(self, ctx, rgba, mask):
        self.calls.append(("rgba", rgba, mask))
        return 0


def test_python_host_sends_the_specified_arguments():
    import gsplat_hip as gh
    r = object.__new__(gh.HIPRenderer)
    r._L, r._ctx, r._check = _Lib(), None, lambda rc: None
    r.scene_translate_selected(T)
    r.scene_rotate_selected(Q)
    r.scene_rotate_selected(Q, PIVOT)
    r.scene_scale_selected(S)
    r.scene_scale_selected(S, pivot=(0, 0, 0))           # a pivot of zero is a pivot, not None
    r.scene_set_rgba_selected(0x80112233)
    r.scene_set_rgba_selected((0x33, 0x22, 0x11, 0x80), "a")
    r.scene_set_rgba_selected(0x80112233, "bgr")
    r.scene_set_rgba_selected(0x80112233, 0x0000ff00)
    assert r._L.calls == [("translate", T), ("rotate", Q, None), ("rotate", Q, PIVOT), ("scale", S, None), ("scale", S, (0.0, 0.0, 0.0)),
                          ("rgba", 0x80112233, 0xffffffff), ("rgba", 0x80112233, 0xff000000), ("rgba", 0x80112233, 0x00ffffff),
                          ("rgba", 0x80112233, 0x0000ff00)]
    with pytest.raises(ValueError, match="channels"):
        r.scene_set_rgba_selected(0, "rgbx")
    with pytest.raises(ValueError):
        r.scene_rotate_selected(Q, (1.0, 2.0))


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


def test_unbound_host_loops_equal_the_reference_bit_for_bit(oracle, tmp_path):
    if NODE is None:
        pytest.skip("node is not installed")
    import gsplat_hip as gh
    rows = gh.synth.synth_rows(N, 17)
    rows_path, out_path = tmp_path / "rows.splat", tmp_path / "out.bin"
    rows_path.write_bytes(np.ascontiguousarray(rows, dtype=np.uint8).tobytes())
    r = subprocess.run([NODE, DRIVER, "host", str(rows_path), str(out_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    info = json.loads(r.stdout)
    assert info == {"n": N, "steps": 7, "changes": 7}
    got = np.frombuffer(out_path.read_bytes(), dtype=np.uint32).reshape(7, 18 * N)
    st = oracle.SceneState(rows)
    st.rotate(Q0)
    st.scale(S0)
    sel = (7 * np.arange(N) + 3) % 5 < 2
    walk = (("translate", T, None), ("rotate", Q, None), ("rotate", Q, PIVOT), ("scale", S, None), ("scale", S, PIVOT),
            ("paint", 0x60000000, 0xff000000), ("paint", 0x0040c020, 0x00ffffff))
    for k, (name, arg, extra) in enumerate(walk):
        if name == "paint":
            er.paint(st, sel, arg, extra)
        else:
            er.apply(st, sel, name, arg, extra)
        at = 0
        for field, words in (("data", 8), ("positions", 3), ("rotations", 4), ("scales", 3)):
            want = getattr(st, field).view(np.uint32)
            assert np.array_equal(got[k, at:at + words * N], want), "step %d (%s): %s differs" % (k, name, field)
            at += words * N


def test_renderer_typings_addon_and_bench_carry_the_names():
    src = open(os.path.join(JS, "renderers", "HIPRenderer.js")).read()
    for word in ("this.selectionBounds = ()", "this.translateSelection = (v)", "this.rotateSelection = (q, options)", "this.scaleSelection = (s, options)",
                 "this.paintSelection = (rgba)", "editSelected: (kind, f64, pivot)", "paintSelected: (rgba, byteMask)"):
        assert word in src, word
    scene = open(os.path.join(JS, "core", "Scene.js")).read()
    for word in ("translateSelection(mask, v)", "rotateSelection(mask, q, options)", "scaleSelection(mask, s, options)", "paintSelection(mask, rgba)",
                 "this._editDevices(5,", "this._editDevices(6,", "this._editDevices(7,", "this._editDevices(8,", "d.setSelection(args.mask);"):
        assert word in scene, word
    dts = open(os.path.join(JS, "index.d.ts")).read()
    for word in ("selectionBounds(): SelectionBounds;", "translateSelection(v: Vec3Like): void;", "scaleSelection(s: Vec3Like, options?: { pivot?: Vec3Like }): void;",
                 "paintSelection(rgba: PaintChannels): void;", "translateSelection(mask: Uint32Array, v: Vector3): void;",
                 "rotateSelection(mask: Uint32Array, q: Quaternion, options?: { pivot?: Vec3Like }): void;",
                 "scaleSelection(mask: Uint32Array, s: Vector3, options?: { pivot?: Vec3Like }): void;", "paintSelection(mask: Uint32Array, rgba: PaintChannels): void;",
                 "editSelected?(kind: number, args: Float64Array, pivot: Float64Array | null): void;", "paintSelected?(rgba: number, byteMask: number): void;"):
        assert word in dts, word
    addon = open(os.path.join(JS, "native", "addon.cc")).read()
    for name, fn in (("selectionBounds", "SelectionBounds"), ("editSelected", "EditSelected"), ("paintSelected", "PaintSelected")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for fn in NAMES_C:
        assert fn + "(" in addon, fn
    bench = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    assert '"--edit-selected"' in bench and "gsr_scene_rotate_selected(" in bench and "gsr_selection_set(" in bench and '\\"edit_ms\\"' in bench

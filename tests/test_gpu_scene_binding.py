"""Scene transforms on the device behind the Scene API, on the GPU: gsr_set_scene_arrays and the device-side gsr_read_scene at
the ABI (against oracle.SceneState, the reference's transforms restated in f64), the bounds-checked twin over the same cases,
and the Node host with a Scene attached to real renderers (tests/js/scene_device_check.js compares bit for bit)."""
import ctypes
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
DRIVER = os.path.join(ROOT, "tests", "js", "scene_device_check.js")
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
W, H, FX = 640, 480, 560.0
COUNTS = (0, 1, 255, 256, 257, 20000)
Q0, S0 = (0.1, -0.3, 0.2, 0.9273618495495703), (1.25, 0.8, 1.1)
STEPS = (("rotate", (-0.2, 0.5, 0.1, 0.8366600265340756)), ("translate", (0.25, -0.5, 1.0)), ("scale", (0.9, 1.2, 1.05)),
         ("limit_box", (-2.0, 2.2, -1.8, 2.0, -2.5, 1.9)))
GSR_ERR_ARG, GSR_ERR_SCENE = -1, -4


def _state(oracle, n, seed=17):
    """A Scene that was rotated and scaled on the host before its first frame: float rotations / scales no .splat row can express."""
    import gsplat_hip as gh
    rows = gh.synth.synth_rows(n, seed) if n else np.zeros(0, dtype=np.uint8)
    st = oracle.SceneState(rows)
    st.rotate(Q0)
    st.scale(S0)
    return st


def _same_state(got, st, what):
    data, pos, rot, scl = got
    for name, a, b in (("data", data, st.data[:8 * st.n]), ("positions", pos, st.positions), ("rotations", rot, st.rotations), ("scales", scl, st.scales)):
        assert a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %s differs" % (what, name)


def _frame(r, cam):
    r.set_camera(cam)
    r._check(r._L.gsr_render(r._ctx))
    return r.lastDepthIndex(), r.readPixelsFloat()


def _walk(oracle, n, lib_path=None):
    import gsplat_hip as gh
    cam = gh.orbit_camera(3, width=W, height=H, fx=FX)
    st = _state(oracle, n)
    r = gh.HIPRenderer(W, H, lib_path=lib_path)
    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        for name, arg in (("upload", None),) + STEPS:
            if name == "limit_box":
                st.limit_box(arg)
                assert r.scene_limit_box(arg) == st.n
            elif name != "upload":
                getattr(st, name)(arg)
                getattr(r, "scene_" + name)(arg)
            _same_state(r.read_scene(), st, "%s at n = %d" % (name, n))
            if st.n:
                fresh = gh.HIPRenderer(W, H, lib_path=lib_path)
                try:
                    fresh.set_raw_scene(st.data, st.positions)
                    want, got = _frame(fresh, cam), _frame(r, cam)
                finally:
                    fresh.dispose()
                assert np.array_equal(got[0], want[0]), "depthIndex after %s at n = %d" % (name, n)
                assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "image after %s at n = %d" % (name, n)
    finally:
        r.dispose()
    return st.n


@pytest.mark.parametrize("n", COUNTS)
def test_arrays_upload_then_device_transforms_equal_the_oracle(oracle, n):
    kept = _walk(oracle, n)
    assert kept <= n and (n < 20000 or 0 < kept < n)


def test_bounds_twin_counts_nothing_over_the_same_cases(oracle):
    import gsplat_hip as gh
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    for n in COUNTS:
        _walk(oracle, n, lib_path=BOUNDS_LIB)
    buf = (ctypes.c_uint32 * 8)()
    assert L.gsr_debug_bounds_scene(buf) == 0
    assert list(buf) == [0] * 8


def test_mismatching_positions_are_refused_and_the_context_keeps_its_scene(oracle):
    import gsplat_hip as gh
    cam = gh.orbit_camera(3, width=W, height=H, fx=FX)
    a, b = _state(oracle, 5000, seed=3), _state(oracle, 4000, seed=4)
    r = gh.HIPRenderer(W, H)
    try:
        r.set_scene_arrays(a.data, a.positions, a.rotations, a.scales)
        before = _frame(r, cam)
        bad = b.positions.copy()
        bad[3 * 1234 + 1] = np.nextafter(bad[3 * 1234 + 1], np.float32(np.inf))
        with pytest.raises(gh.GsplatError) as e:
            r.set_scene_arrays(b.data, bad, b.rotations, b.scales)
        assert e.value.code == GSR_ERR_SCENE
        r._n = a.n
        _same_state(r.read_scene(), a, "after the refused upload")
        after = _frame(r, cam)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
        # NULL arrays and too many splats on a live context: refused, nothing touched
        p = b.data.ctypes.data
        for args in ((None, p, p, p, 1), (p, None, p, p, 1), (p, p, None, p, 1), (p, p, p, None, 1), (p, p, p, p, 0x7fffffff // 8 + 1)):
            assert r._L.gsr_set_scene_arrays(r._ctx, *args) == GSR_ERR_ARG
        _same_state(r.read_scene(), a, "after the refused arguments")
        r.scene_rotate(STEPS[0][1])          # and the scene still takes transforms
        a.rotate(STEPS[0][1])
        _same_state(r.read_scene(), a, "rotate after the refusals")
    finally:
        r.dispose()


def test_read_scene_gives_the_same_bytes_for_every_combination_of_outputs(oracle):
    import gsplat_hip as gh
    st = _state(oracle, 20000 + 77)
    r = gh.HIPRenderer(W, H)
    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        r.scene_translate(STEPS[1][1])
        full = r.read_scene()
        sizes = (8, 3, 4, 3)
        for mask in itertools.product((False, True), repeat=4):
            outs = [np.full(k * st.n, 0xA5A5A5A5, dtype=np.uint32) if on else None for k, on in zip(sizes, mask)]
            cnt = ctypes.c_uint32(0)
            r._check(r._L.gsr_read_scene(r._ctx, *[o.ctypes.data if o is not None else None for o in outs], ctypes.byref(cnt)))
            assert cnt.value == st.n
            for o, f in zip(outs, full):
                assert o is None or np.array_equal(o, f.view(np.uint32)), mask
        plain = gh.HIPRenderer(W, H)     # a scene without rotations / scales still refuses them, and reads the other two
        try:
            plain.set_raw_scene(st.data, st.positions)
            with pytest.raises(gh.GsplatError):
                plain.read_scene()
            d, p, _, _ = plain.read_scene(with_rows=False)
            assert np.array_equal(d, st.data) and np.array_equal(p.view(np.uint32), st.positions.view(np.uint32))
        finally:
            plain.dispose()
    finally:
        r.dispose()


def _node(*args, timeout=900):
    assert NODE is not None and os.path.exists(ADDON), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    r = subprocess.run([NODE] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("mode, least", (("edits", 15), ("roundrobin", 5), ("sh", 6), ("delivery", 4)))
def test_node_scene_attached_to_renderers(mode, least):
    out = _node(DRIVER, mode)
    assert out["failed"] == [] and len(out["checks"]) >= least, out


def test_an_edit_per_frame_is_far_faster_attached_than_through_the_host():
    """1 M splats, scene.rotate(q); renderer.render(scene, camera): loosely bounded here, reported exactly by the tool."""
    out = _node(os.path.join(ROOT, "tools", "bench_scene_edit.js"), 1000000, 20)
    print(json.dumps(out))
    assert out["speedup_rotate"] >= 20 and out["speedup_scale"] >= 20, out

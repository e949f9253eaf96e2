"""Editing the selection on the GPU: gsr_scene_translate_selected / _rotate_selected / _scale_selected / _set_rgba_selected and
gsr_selection_bounds against tests/edit_reference.py -- the oracle's own transforms on a sub-scene holding only the selected
splats -- bit for bit, over the word, half-wave, wave and workgroup edges and every kind of selection; the frame state, the
refusals, a shared scene, and the bounds-checked twin over the same walk."""
import copy
import ctypes
import os

import numpy as np
import pytest

import edit_reference as er

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
W, H, FX = 640, 480, 560.0
COUNTS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 20000)   # word, half-wave, wave and workgroup edges
BIG = 20000
Q0, S0 = (0.1, -0.3, 0.2, 0.9273618495495703), (1.25, 0.8, 1.1)
T, Q, S, PIVOT = (0.25, -0.5, 1.0), (-0.2, 0.5, 0.1, 0.8366600265340756), (0.9, 1.2, 1.05), (0.3, -0.7, 1.9)
RGBA = 0x6040c020
WALK = (("translate", T, None), ("rotate", Q, None), ("rotate", Q, PIVOT), ("scale", S, None), ("scale", S, PIVOT),
        ("paint", RGBA, 0xff000000), ("paint", RGBA, 0x00ffffff))
SELECTIONS = ("empty", "all", "first", "last", "alternating bits", "alternating words", "random half")
GSR_ERR_ARG = -1


def _selection(kind, n):
    i = np.arange(n)
    if kind == "empty":
        return np.zeros(n, dtype=bool)
    if kind == "all":
        return np.ones(n, dtype=bool)
    if kind == "first":
        return i == 0
    if kind == "last":
        return i == n - 1
    if kind == "alternating bits":
        return i % 2 == 1
    if kind == "alternating words":   # the zero-word early return and its neighbours both run
        return (i >> 5) % 2 == 0
    return np.random.default_rng(1234 + n).random(n) < 0.5


def _hidden(n):
    return np.arange(n) % 3 == 1


def _state(oracle, n, seed=17):
    """A Scene that was rotated and scaled on the host before its first frame: float rotations / scales no .splat row can express."""
    import gsplat_hip as gh
    st = oracle.SceneState(gh.synth.synth_rows(n, seed))
    st.rotate(Q0)
    st.scale(S0)
    return st


def _same_state(got, st, what):
    data, pos, rot, scl = got
    for name, a, b in (("data", data, st.data[:8 * st.n]), ("positions", pos, st.positions), ("rotations", rot, st.rotations), ("scales", scl, st.scales)):
        assert a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %s differs" % (what, name)


def _step(r, st, sel, step):
    """one step of the walk on the device and on the reference"""
    name, arg, extra = step
    if name == "paint":
        r.scene_set_rgba_selected(arg, extra)
        er.paint(st, sel, arg, extra)
    else:
        if name == "translate":
            r.scene_translate_selected(arg)
        else:
            getattr(r, "scene_%s_selected" % name)(arg, extra)
        er.apply(st, sel, name, arg, extra)


def _frame(r, cam):
    r.set_camera(cam)
    r._check(r._L.gsr_render(r._ctx))
    return r.lastDepthIndex(), r.readPixelsFloat()


def _same_frame(got, want, what):
    assert np.array_equal(got[0], want[0]), "depthIndex " + what
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "image " + what


def _fresh_frame(fresh, st, hid, cam):
    fresh.set_raw_scene(st.data, st.positions)
    fresh.set_hidden(hid)
    return _frame(fresh, cam)


def _walk(oracle, n, lib_path=None):
    import gsplat_hip as gh
    cam = gh.orbit_camera(3, width=W, height=H, fx=FX)
    base = _state(oracle, n)
    hid = _hidden(n)
    r = gh.HIPRenderer(W, H, lib_path=lib_path)
    fresh = gh.HIPRenderer(W, H, lib_path=lib_path) if n == BIG else None
    try:
        for kind in SELECTIONS:
            st, sel = copy.deepcopy(base), _selection(kind, n)
            r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
            assert r.set_hidden(hid) == int(hid.sum())
            assert r.set_selection(sel) == int(sel.sum())
            count, mn, mx = r.selection_bounds()
            want = er.bounds(st.positions, sel)
            assert count == want[0] and np.all(mn == want[1]) and np.all(mx == want[2]), ("bounds", kind, n)
            for step in WALK:
                what = "%s %s at n = %d, selection %s" % (step[0], "with a pivot" if step[2] is not None and step[0] != "paint" else hex(step[2] or 0), n, kind)
                _step(r, st, sel, step)
                _same_state(r.read_scene(), st, what)
                assert np.array_equal(r.selection(), sel) and np.array_equal(r.hidden(), hid), what
                if fresh is not None:
                    _same_frame(_frame(r, cam), _fresh_frame(fresh, st, hid, cam), what)
            count, mn, mx = r.selection_bounds()   # hidden splats that are selected count like any other
            want = er.bounds(st.positions, sel)
            assert count == want[0] and np.all(mn == want[1]) and np.all(mx == want[2]), ("bounds after the walk", kind, n)
    finally:
        r.dispose()
        if fresh is not None:
            fresh.dispose()


@pytest.mark.parametrize("n", COUNTS)
def test_walk_equals_the_reference_bit_for_bit(oracle, n):
    _walk(oracle, n)


@pytest.mark.parametrize("n", (65, 1025, BIG))
def test_everything_selected_without_a_pivot_is_the_whole_scene_transform(oracle, n):
    import gsplat_hip as gh
    st = _state(oracle, n)
    a, b = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    try:
        for r in (a, b):
            r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        assert a.set_selection(np.ones(n, dtype=bool)) == n
        for name, arg in (("rotate", Q), ("scale", S), ("translate", T)):
            if name == "translate":
                a.scene_translate_selected(arg)
            else:
                getattr(a, "scene_%s_selected" % name)(arg)
            getattr(b, "scene_" + name)(arg)
            for x, y, field in zip(a.read_scene(), b.read_scene(), ("data", "positions", "rotations", "scales")):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (name, field, n)
    finally:
        a.dispose()
        b.dispose()


def test_bounds_with_a_nan_position_and_hidden_splats_selected(oracle):
    import gsplat_hip as gh
    n = 1025
    st = _state(oracle, n)
    nan = np.array([0x7fc00000], dtype=np.uint32)
    st.positions.view(np.uint32)[3 * 700 + 1] = nan[0]   # y of splat 700, in data as in positions
    st.data[8 * 700 + 1] = nan[0]
    r = gh.HIPRenderer(W, H)
    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        count, mn, mx = r.selection_bounds()     # never selected in: the empty selection, nothing launched
        assert count == 0 and np.all(mn == np.inf) and np.all(mx == -np.inf)
        for kind in SELECTIONS:
            sel = _selection(kind, n)
            sel[700] = kind != "empty"
            r.set_selection(sel)
            r.set_hidden(sel & (np.arange(n) % 2 == 0))   # hidden splats that are selected count like any other
            count, mn, mx = r.selection_bounds()
            want = er.bounds(st.positions, sel)
            assert count == want[0] == int(sel.sum()) and np.all(mn == want[1]) and np.all(mx == want[2]), kind
            assert not np.isnan(mn).any() and not np.isnan(mx).any()
        r.set_selection(np.arange(n) == 700)     # the NaN alone: counted, and its y never enters the box
        count, mn, mx = r.selection_bounds()
        assert count == 1 and mn[1] == np.inf and mx[1] == -np.inf and mn[0] == mx[0] == st.positions[3 * 700]
    finally:
        r.dispose()


def test_an_edit_invalidates_the_frame_until_the_next_one(oracle):
    import gsplat_hip as gh
    n = BIG
    cam = gh.orbit_camera(3, width=W, height=H, fx=FX)
    st = _state(oracle, n)
    r = gh.HIPRenderer(W, H)
    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        r.set_overlay()
        r.contrib_reset()
        sel = _selection("random half", n)
        r.set_selection(sel)
        needs_frame = (lambda: r.select_region((100, 100, 200, 200), op="add"), lambda: r.pick([(320, 240)]), r.overlay_async, r.contrib_accumulate,
                       r.depth_async)
        edits = (lambda: r.scene_translate_selected(T), lambda: r.scene_rotate_selected(Q, PIVOT), lambda: r.scene_scale_selected(S),
                 lambda: r.scene_set_rgba_selected(RGBA, "a"),
                 lambda: r.scene_translate_selected((0.0, 0.0, 0.0)))   # changes no bit: an edit all the same
        for edit in edits:
            _frame(r, cam)
            r.set_selection(sel)
            for call in needs_frame:
                call()
            r.sync()
            r.set_selection(sel)
            edit()
            for call in needs_frame:
                with pytest.raises(gh.GsplatError, match="no frame") as e:
                    call()
                assert e.value.code == GSR_ERR_ARG
            assert r.selection_bounds()[0] == int(sel.sum())   # (no edit and no frame needed)
        _frame(r, cam)
        for call in needs_frame:
            call()
        r.sync()
    finally:
        r.dispose()


def test_refusals_leave_the_scene_untouched(oracle):
    import gsplat_hip as gh
    n = 5000
    st = _state(oracle, n)
    sel = _selection("random half", n)
    rng = np.random.default_rng(11)
    band = np.array([999, 2000, 3000], dtype=np.int32)
    tex = [rng.integers(0, 1 << 32, 8 * (n - 1000), dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    r = gh.HIPRenderer(W, H)
    flat = gh.HIPRenderer(W, H)
    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        # a never-selected context accepts every call and changes nothing
        r.scene_translate_selected(T)
        r.scene_rotate_selected(Q, PIVOT)
        r.scene_scale_selected(S)
        r.scene_set_rgba_selected(RGBA)
        _same_state(r.read_scene(), st, "never selected")
        assert r.selection_count() == 0
        r.set_selection(sel)
        # a non-finite scale, NULL pointers
        for bad in ((np.inf, 1.0, 1.0), (1.0, np.nan, 1.0), (1.0, 1.0, -np.inf)):
            with pytest.raises(gh.GsplatError, match="finite") as e:
                r.scene_scale_selected(bad, PIVOT)
            assert e.value.code == GSR_ERR_ARG
        L, ctx = r._L, r._ctx
        assert L.gsr_scene_translate_selected(ctx, None) == GSR_ERR_ARG and L.gsr_scene_rotate_selected(ctx, None, None) == GSR_ERR_ARG
        assert L.gsr_scene_scale_selected(ctx, None, None) == GSR_ERR_ARG and L.gsr_selection_bounds(ctx, None) == GSR_ERR_ARG
        _same_state(r.read_scene(), st, "after refused arguments")
        r.scene_scale_selected((0.0, 1.0, 1.0))   # zero is allowed: there is no frame to invert here
        er.apply(st, sel, "scale", (0.0, 1.0, 1.0))
        _same_state(r.read_scene(), st, "scale by zero")
        # SH follow on and SH rows present: rotate and scale are refused, translate and paint pass
        r.set_sh_follow(True)
        r.scene_rotate_selected(Q)                # (no SH rows yet: allowed)
        er.apply(st, sel, "rotate", Q)
        r.set_sh(tex, band)
        for call in (lambda: r.scene_rotate_selected(Q), lambda: r.scene_rotate_selected(Q, PIVOT), lambda: r.scene_scale_selected(S),
                     lambda: r.scene_scale_selected(S, PIVOT)):
            with pytest.raises(gh.GsplatError, match="SH") as e:
                call()
            assert e.value.code == GSR_ERR_ARG
        _same_state(r.read_scene(), st, "after the SH-follow refusals")
        frame = r.sh_frame()
        r.scene_translate_selected(T)
        er.apply(st, sel, "translate", T)
        r.scene_set_rgba_selected(RGBA, "a")
        er.paint(st, sel, RGBA, 0xff000000)
        _same_state(r.read_scene(), st, "translate and paint under SH follow")
        assert np.array_equal(np.asarray(r.sh_frame()[0]), np.asarray(frame[0]))
        r.set_sh_follow(False)
        r.scene_rotate_selected(Q, PIVOT)
        er.apply(st, sel, "rotate", Q, PIVOT)
        _same_state(r.read_scene(), st, "rotate with SH follow off")
        # a scene without rotations / scales refuses the edits, and still answers the bounds
        flat.set_raw_scene(st.data, st.positions)
        flat.set_selection(sel)
        for call in (lambda: flat.scene_translate_selected(T), lambda: flat.scene_rotate_selected(Q), lambda: flat.scene_scale_selected(S),
                     lambda: flat.scene_set_rgba_selected(RGBA)):
            with pytest.raises(gh.GsplatError, match="gsr_set_scene_rows") as e:
                call()
            assert e.value.code == GSR_ERR_ARG
        count, mn, mx = flat.selection_bounds()
        want = er.bounds(st.positions, sel)
        assert count == want[0] and np.all(mn == want[1]) and np.all(mx == want[2])
    finally:
        r.dispose()
        flat.dispose()


def test_shared_scene_members_see_the_edit(oracle):
    import gsplat_hip as gh
    n = BIG
    cam = gh.orbit_camera(3, width=W, height=H, fx=FX)
    st = _state(oracle, n)
    sel = _selection("random half", n)
    a, b = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H, throughput=True)
    fresh = {a: gh.HIPRenderer(W, H), b: gh.HIPRenderer(W, H, throughput=True)}   # a fresh context of either member's kind
    try:
        a.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        b.share_scene(a)
        assert a.scene_sharing()[0] == 2
        before = {m: _fresh_frame(fresh[m], st, None, cam) for m in (a, b)}
        before8 = fresh[a].readPixels().reshape(H, W, 4).copy()
        for m, name in ((a, "a"), (b, "b")):
            _same_frame(_frame(m, cam), before[m], "member %s before the edit" % name)
        assert b.set_selection(sel) == int(sel.sum())
        a.open_delivery(3)
        a.set_camera(cam)
        a.render_async()                                   # a frame enqueued before the edit (and its delivery) reads the old scene ...
        first = a.deliver()
        b.scene_rotate_selected(Q, PIVOT)                  # ... the edit arrives through the other member, with no host wait ...
        with pytest.raises(gh.GsplatError, match="no frame"):
            a.pick([(320, 240)])                           # (every member's frame state is marked as edited)
        a.render_async()                                   # ... and a frame enqueued behind it reads the new one
        second = a.deliver()
        er.apply(st, sel, "rotate", Q, PIVOT)
        after = {m: _fresh_frame(fresh[m], st, None, cam) for m in (a, b)}
        after8 = fresh[a].readPixels().reshape(H, W, 4).copy()
        assert not np.array_equal(before8, after8)
        for serial, want, what in ((first, before8, "enqueued before the edit"), (second, after8, "enqueued behind the edit")):
            got_serial, px = a.acquire(serial)
            assert got_serial == serial and np.array_equal(px, want), what
            a.release(serial)
        a.sync()
        a.close_delivery()
        for m, name in ((b, "b"), (a, "a")):
            _same_frame(_frame(m, cam), after[m], "member %s after the edit" % name)
        a.scene_set_rgba_selected(RGBA, "rgb")             # and an edit through the first member
        er.paint(st, sel, RGBA, 0x00ffffff)
        _same_state(a.read_scene(), st, "read through member a")
        _same_state(b.read_scene(), st, "read through member b")
        for m, name in ((b, "b"), (a, "a")):
            _same_frame(_frame(m, cam), _fresh_frame(fresh[m], st, None, cam), "member %s after the paint" % name)
        assert a.scene_sharing()[0] == 2 and b.scene_sharing()[0] == 2
        assert np.array_equal(a.selection(), sel) and a.selection_bounds()[0] == int(sel.sum())
    finally:
        for x in (a, b) + tuple(fresh.values()):
            x.dispose()


def test_bounds_twin_counts_nothing_over_the_same_walk(oracle):
    import gsplat_hip as gh
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    for n in COUNTS:
        _walk(oracle, n, lib_path=BOUNDS_LIB)   # every size, every selection, the frames at 20000 included
    for name in ("gsr_debug_bounds_edit", "gsr_debug_bounds_scene"):
        buf = (ctypes.c_uint32 * 8)()
        assert getattr(L, name)(buf) == 0
        assert list(buf) == [0] * 8, name

"""Growing the scene on the GPU: gsr_scene_duplicate_selected / _append_selected / _append_arrays / _reserve / _capacity against
tests/append_reference.py bit for bit -- over the word, half-wave, wave and workgroup edges of source and destination and every kind
of selection, with a NaN and a -0.0 among the copied rows; the frame state, the workflow the default selection exists for, the
capacity rule, the contribution accumulators, a shared scene, the refusals, and the bounds-checked twin over the same walk."""
import copy
import ctypes
import os

import numpy as np
import pytest

import append_reference as ar
import contrib_reference as CR
import edit_reference as er
import hide_reference as hr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
W, H, FX = 640, 480, 560.0
COUNTS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 20000)   # test_gpu_edit.py's: word, half-wave, wave and workgroup edges
BIG = 20000
Q0, S0 = (0.1, -0.3, 0.2, 0.9273618495495703), (1.25, 0.8, 1.1)
T = (0.25, -0.5, 1.0)
SELECTIONS = ("empty", "all", "first", "last", "alternating bits", "alternating words", "random half")
ROUNDS = 3          # duplicates in a row: the selection is the last copies, so n = 31, all selected, ends at 124 across a word and a wave edge
GSR_ERR_ARG, GSR_ERR_SCENE = -1, -4
NAN, NEG0 = np.uint32(0x7fc01234), np.uint32(0x80000000)


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


def _poison(st, sel):
    """one NaN position and one -0.0 among the selected rows, in data as in positions (the upload's check compares bits)"""
    idx = np.flatnonzero(sel)
    if idx.size:
        for row, k, word in ((idx[0], 1, NAN), (idx[-1], 0, NEG0)):
            st.positions.view(np.uint32)[3 * row + k] = word
            st.data[8 * row + k] = word
    return st


def _same_state(got, st, what):
    data, pos, rot, scl = got
    for name, a, b in (("data", data, st.data[:8 * st.n]), ("positions", pos, st.positions), ("rotations", rot, st.rotations), ("scales", scl, st.scales)):
        assert a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %s differs" % (what, name)


def _same_bounds(r, st, sel, what):
    count, mn, mx = r.selection_bounds()
    want = er.bounds(st.positions, sel)
    assert count == want[0] and np.all(mn == want[1]) and np.all(mx == want[2]), ("bounds", what)


def _grown(r, st, sel, hid, got, want, what):
    """everything the header says of the state after a growing call: the scene, the count, (first, count), the selection = exactly the
    tail, the hidden set = the old bits and a clear tail, the bounds of the copies"""
    assert tuple(got) == tuple(want), (what, got, want)
    assert r.scene_count() == st.n, what
    _same_state(r.read_scene(), st, what)
    assert np.array_equal(r.selection(), sel) and r.selection_count() == int(sel.sum()), what
    assert np.array_equal(r.hidden(), hid) and r.hidden_count() == int(hid.sum()), what
    _same_bounds(r, st, sel, what)


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
    r = gh.HIPRenderer(W, H, lib_path=lib_path)
    fresh = gh.HIPRenderer(W, H, lib_path=lib_path) if n == BIG else None
    try:
        for kind in SELECTIONS:
            sel, hid = _selection(kind, n), _hidden(n)
            st = _poison(copy.deepcopy(base), sel)
            r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
            assert r.set_hidden(hid) == int(hid.sum())
            assert r.set_selection(sel) == int(sel.sum())
            capacity = n
            assert r.scene_capacity() == capacity
            for k in range(ROUNDS):
                what = "duplicate %d at n = %d, selection %s" % (k, n, kind)
                got = r.scene_duplicate_selected()
                want = ar.duplicate(st, sel)
                sel, hid = ar.selection_after(st.n, *want), ar.hidden_after(hid, want[1])
                _grown(r, st, sel, hid, got, want, what)
                capacity = ar.capacity_after(capacity, st.n)   # without a reserve the capacity follows the growth rule exactly
                assert r.scene_capacity() == capacity, what
                if fresh is not None and k == ROUNDS - 1:
                    _same_frame(_frame(r, cam), _fresh_frame(fresh, st, hid, cam), what)
    finally:
        r.dispose()
        if fresh is not None:
            fresh.dispose()


@pytest.mark.parametrize("n", COUNTS)
def test_duplicates_equal_the_reference_bit_for_bit(oracle, n):
    _walk(oracle, n)


@pytest.mark.parametrize("throughput", (False, True))
def test_a_duplicate_invalidates_the_frame_and_the_next_one_is_a_fresh_contexts(oracle, throughput):
    import gsplat_hip as gh
    n = BIG
    cam = gh.orbit_camera(3, width=W, height=H, fx=FX)
    st, hid = _state(oracle, n), _hidden(n)
    r, fresh = gh.HIPRenderer(W, H, throughput=throughput), gh.HIPRenderer(W, H, throughput=throughput)
    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        r.set_hidden(hid)
        r.set_overlay()
        needs_frame = (lambda: r.pick([(320, 240)]), r.depth_async, r.overlay_async)
        _frame(r, cam)
        # nothing selected: (n, 0), nothing touched, no edit -- the last frame stays valid and gsr_pick still answers
        assert r.scene_duplicate_selected() == (n, 0) and r.scene_count() == n
        for call in needs_frame:
            call()
        r.sync()
        sel = _selection("random half", n)
        r.set_selection(sel)
        got = r.scene_duplicate_selected()
        want = ar.duplicate(st, sel)
        assert got == want
        for call in needs_frame:
            with pytest.raises(gh.GsplatError, match="no frame") as e:
                call()
            assert e.value.code == GSR_ERR_ARG
        hid = ar.hidden_after(hid, want[1])
        _same_frame(_frame(r, cam), _fresh_frame(fresh, st, hid, cam), "the frame after the duplicate")
        for call in needs_frame:
            call()
        r.sync()
    finally:
        r.dispose()
        fresh.dispose()


@pytest.mark.parametrize("n", (33, 1025, BIG))
def test_duplicate_then_move_the_copies(oracle, n):
    """the use the default selection exists for"""
    import gsplat_hip as gh
    st = _state(oracle, n)
    sel = _selection("random half", n)
    r = gh.HIPRenderer(W, H)
    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        r.set_selection(sel)
        got = r.scene_duplicate_selected()
        want = ar.duplicate(st, sel)
        assert got == want
        tail = ar.selection_after(st.n, *want)
        r.scene_translate_selected(T)
        er.apply(st, tail, "translate", T)
        _same_state(r.read_scene(), st, "duplicate, then translate the copies")
        assert np.array_equal(r.selection(), tail)
    finally:
        r.dispose()


def test_reserve_and_the_capacity_rule(oracle):
    import gsplat_hip as gh
    n = 1025
    st = _state(oracle, n)
    sel, hid = _selection("alternating bits", n), _hidden(n)
    k = int(sel.sum())
    r = gh.HIPRenderer(W, H)
    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        r.set_hidden(hid)
        r.set_selection(sel)
        r.contrib_reset()
        assert r.scene_capacity() == n
        r.scene_reserve(n - 5)                        # below the capacity: a no-op
        assert r.scene_capacity() == n
        small = r.scene_sharing()[1]
        r.scene_reserve(n + 3 * k)                    # the growth alone: no splat, no selection, no hidden bit changes
        assert r.scene_capacity() == n + 3 * k and r.scene_count() == n
        _same_state(r.read_scene(), st, "after the reserve")
        assert np.array_equal(r.selection(), sel) and np.array_equal(r.hidden(), hid)
        reserved = r.scene_sharing()[1]
        assert reserved > small                       # scene_bytes reports the capacity
        for j in range(3):                            # nothing is re-allocated: the capacity and the bytes stay
            got = r.scene_duplicate_selected()
            want = ar.duplicate(st, sel)
            sel, hid = ar.selection_after(st.n, *want), ar.hidden_after(hid, want[1])
            _grown(r, st, sel, hid, got, want, "duplicate %d inside the reserve" % j)
            assert r.scene_capacity() == n + 3 * k and r.scene_sharing()[1] == reserved, j
        r.scene_reserve(n)
        assert r.scene_capacity() == n + 3 * k        # never shrinks
        got = r.scene_duplicate_selected()            # one more: past the reserve, by the rule
        want = ar.duplicate(st, sel)
        assert got == want and r.scene_capacity() == ar.capacity_after(n + 3 * k, st.n) == (n + 3 * k) + (n + 3 * k) // 2
        _same_state(r.read_scene(), st, "past the reserve")
        box = (0.0, 100.0, -100.0, 100.0, -100.0, 100.0)   # limitBox after growth still compacts correctly (about half stays)
        kept = r.scene_limit_box(box)
        st.limit_box(box)
        assert 0 < kept == st.n < n + 4 * k
        _same_state(r.read_scene(), st, "limitBox after growth")
        assert r.scene_capacity() >= kept
    finally:
        r.dispose()


def _view(oracle, cam, st):
    v, p, vp = cam.f32()
    rec, bbox, _ = oracle.project(st.data, v, p, cam.fx, cam.fy, W, H)
    return rec, bbox, oracle.sort(vp, st.positions)[0], W, H


def _same_contrib(a, b, what):
    for x, y, name in zip(a[:3], b[:3], ("weight", "peak", "pixels")):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert x.size == y.size and np.array_equal(x, y), (what, name)


def test_contribution_accumulators_keep_the_old_rows_and_start_the_new_at_zero(oracle):
    import gsplat_hip as gh
    n = 1025
    cam = gh.orbit_camera(3, width=W, height=H, fx=FX)
    st = _state(oracle, n)
    sel = _selection("random half", n)
    r, fresh = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        never = gh.HIPRenderer(W, H)                  # never reset: stays "never reset" through a duplicate
        try:
            never.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
            never.set_selection(sel)
            never.scene_duplicate_selected()
            with pytest.raises(gh.GsplatError, match="nothing was ever reset"):
                never.read_contrib()
        finally:
            never.dispose()
        r.contrib_reset()
        _frame(r, cam)
        r.contrib_accumulate()
        before = r.read_contrib()
        assert before[3] == 1 and before[2].any()
        r.set_selection(sel)
        got = r.scene_duplicate_selected()
        want = ar.duplicate(st, sel)
        assert got == want
        after = r.read_contrib()
        _same_contrib(after, ar.contrib_after(before[:3], want[1]), "the accumulators after the duplicate")
        assert after[3] == 1
        # a pass on the grown scene adds to them: the sums add, the peaks take the maximum (contrib_reference.combine) ...
        fresh.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        fresh.contrib_reset()
        _frame(fresh, cam)
        fresh.contrib_accumulate()
        one = fresh.read_contrib()
        _frame(r, cam)
        r.contrib_accumulate()
        both = r.read_contrib()
        assert both[3] == 2
        _same_contrib(both, CR.combine(after[:3], one[:3]), "old rows' values + a pass on the grown scene")
        # ... and that pass is the specification's of the grown scene for this view: pixels word for word, weight and peak inside its bounds
        ref = CR.contrib_reference([_view(oracle, cam, st)], st.n)
        assert np.array_equal(one[2], ref["pixels"])
        ratios = CR.excess(one, ref)
        print("append: contribution of the grown scene, max |gpu - ref| / bound: weight %.3f peak %.3f" % ratios)
        assert ratios[0] <= 1.0 and ratios[1] <= 1.0, ratios
    finally:
        r.dispose()
        fresh.dispose()


def test_shared_scene_members_see_the_growth(oracle):
    import gsplat_hip as gh
    n = BIG
    cam = gh.orbit_camera(3, width=W, height=H, fx=FX)
    st = _state(oracle, n)
    sel = _selection("random half", n)
    a, b = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H, throughput=True)
    fresh = gh.HIPRenderer(W, H, throughput=True)
    try:
        a.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        b.share_scene(a)
        assert a.scene_sharing()[0] == 2
        _frame(b, cam)
        assert b.set_selection(sel) == int(sel.sum())      # the selection is the one both members see
        got = a.scene_duplicate_selected()
        want = ar.duplicate(st, sel)
        assert got == want
        with pytest.raises(gh.GsplatError, match="no frame"):
            b.pick([(320, 240)])                           # (every member's frame state is marked as edited)
        _same_frame(_frame(b, cam), _fresh_frame(fresh, st, None, cam), "member b after the duplicate through a")
        assert a.scene_sharing()[0] == 2 and b.scene_sharing()[0] == 2
        tail = ar.selection_after(st.n, *want)
        assert np.array_equal(a.selection(), tail) and np.array_equal(b.selection(), tail)
        assert b.scene_count() == st.n
        _same_state(b.read_scene(), st, "read through member b")
        # from = a member of the same shared scene is exactly duplicate
        got = a.scene_append_selected(b)
        want = ar.duplicate(st, tail)
        assert got == want
        _same_state(a.read_scene(), st, "append_selected from a member of the same scene")
        _same_frame(_frame(b, cam), _fresh_frame(fresh, st, None, cam), "member b after the second growth")
    finally:
        for x in (a, b, fresh):
            x.dispose()


def test_append_selected_from_another_scene(oracle):
    import gsplat_hip as gh
    n, m = 1023, 257
    cam = gh.orbit_camera(3, width=W, height=H, fx=FX)
    st, src = _state(oracle, n), _state(oracle, m, seed=5)
    sel = _selection("random half", m)
    _poison(src, sel)
    rng = np.random.default_rng(11)
    band = np.array([99, 150, 200], dtype=np.int32)
    tex = [rng.integers(0, 1 << 32, 8 * (m - 100), dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    dst, frm, fresh = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    try:
        dst.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        frm.set_scene_arrays(src.data, src.positions, src.rotations, src.scales)
        frm.set_sh(tex, band)                              # `from` has SH rows: they are not carried
        assert frm.set_selection(sel) == int(sel.sum())
        _frame(frm, cam)
        hid = _hidden(n)
        dst.set_hidden(hid)
        got = dst.scene_append_selected(frm)
        want = ar.append_selected(st, src, sel)
        tail, hid = ar.selection_after(st.n, *want), ar.hidden_after(hid, want[1])
        _grown(dst, st, tail, hid, got, want, "append_selected 257 -> 1023")
        assert dst.read_scene_sh()[0][0].size == 0
        # the destination renders the copies with their rgba word
        _same_frame(_frame(dst, cam), _fresh_frame(fresh, st, hid, cam), "the destination's frame")
        # `from` is unchanged: scene, selection, SH rows, and its last frame is still valid
        _same_state(frm.read_scene(), src, "from's scene")
        assert np.array_equal(frm.selection(), sel) and frm.scene_count() == m
        assert all(np.array_equal(x, y) for x, y in zip(frm.read_scene_sh()[0], tex))
        frm.pick([(320, 240)])
        # from == ctx is exactly duplicate
        got = dst.scene_append_selected(dst)
        want = ar.duplicate(st, tail)
        tail, hid = ar.selection_after(st.n, *want), ar.hidden_after(hid, want[1])
        _grown(dst, st, tail, hid, got, want, "append_selected from itself")
    finally:
        for x in (dst, frm, fresh):
            x.dispose()


def test_append_arrays(oracle):
    import gsplat_hip as gh
    n, m = 1023, 257
    st, add = _state(oracle, n), _state(oracle, m, seed=5)
    _poison(add, np.ones(m, dtype=bool))
    r, whole, empty = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        hid, sel = _hidden(n), _selection("alternating words", n)
        r.set_hidden(hid)
        r.set_selection(sel)
        # a bad positions array: GSR_ERR_SCENE, and the count, the scene, the selection and the capacity are unchanged
        bad = add.positions.copy()
        bad[3 * 100 + 2] += 1.0
        with pytest.raises(gh.GsplatError, match="positions differ") as e:
            r.scene_append_arrays(add.data, bad, add.rotations, add.scales)
        assert e.value.code == GSR_ERR_SCENE
        assert r.scene_count() == n and r.scene_capacity() == n
        _same_state(r.read_scene(), st, "after the refused upload")
        assert np.array_equal(r.selection(), sel) and np.array_equal(r.hidden(), hid)
        # a good one: set_scene_arrays of the concatenation, read back
        first = r.scene_append_arrays(add.data, add.positions, add.rotations, add.scales)
        want = ar.append_arrays(st, add.data, add.positions, add.rotations, add.scales)
        tail, hid = ar.selection_after(st.n, *want), ar.hidden_after(hid, m)
        _grown(r, st, tail, hid, (first, m), want, "append_arrays 257 -> 1023")
        whole.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        for x, y, name in zip(r.read_scene(), whole.read_scene(), ("data", "positions", "rotations", "scales")):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
        assert r.scene_capacity() == ar.capacity_after(n, n + m)
        # a scene with no splats and no rows accepts the call and becomes a scene with rows
        assert empty.scene_count() == 0
        assert empty.scene_append_arrays(add.data, add.positions, add.rotations, add.scales) == 0
        _same_state(empty.read_scene(), add, "append_arrays into the empty scene")
        assert empty.selection().all() and empty.scene_count() == m
        empty.scene_translate_selected(T)                  # it has rows: the edits accept it
        er.apply(add, np.ones(m, dtype=bool), "translate", T)
        _same_state(empty.read_scene(), add, "the appended rows, moved")
    finally:
        for x in (r, whole, empty):
            x.dispose()


def _refusals(oracle, lib_path=None):
    import gsplat_hip as gh
    n = 5000
    st = _state(oracle, n)
    sel = _selection("random half", n)
    rng = np.random.default_rng(11)
    band = np.array([999, 2000, 3000], dtype=np.int32)
    tex = [rng.integers(0, 1 << 32, 8 * (n - 1000), dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    r, flat = gh.HIPRenderer(W, H, lib_path=lib_path), gh.HIPRenderer(W, H, lib_path=lib_path)
    u32 = ctypes.c_uint32
    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        r.set_selection(sel)
        flat.set_raw_scene(st.data, st.positions)
        flat.set_selection(sel)
        L, ctx = r._L, r._ctx
        a, b = u32(0), u32(0)
        d, p, q, s = (np.ascontiguousarray(x) for x in (st.data, st.positions, st.rotations, st.scales))

        def unchanged(what):
            assert r.scene_count() == n and r.scene_capacity() == n, what
            _same_state(r.read_scene(), st, what)
            assert np.array_equal(r.selection(), sel), what

        # a NULL from; NULL arrays with m > 0
        assert L.gsr_scene_append_selected(ctx, None, ctypes.byref(a), ctypes.byref(b)) == GSR_ERR_ARG
        for args in ((None, p.ctypes.data, q.ctypes.data, s.ctypes.data), (d.ctypes.data, None, q.ctypes.data, s.ctypes.data),
                     (d.ctypes.data, p.ctypes.data, None, s.ctypes.data), (d.ctypes.data, p.ctypes.data, q.ctypes.data, None)):
            assert L.gsr_scene_append_arrays(ctx, *args, 10, ctypes.byref(a)) == GSR_ERR_ARG
        unchanged("NULL pointers")
        # a destination without rotations / scales; a `from` without them
        for call in (flat.scene_duplicate_selected, lambda: flat.scene_append_selected(r), lambda: flat.scene_reserve(2 * n),
                     lambda: flat.scene_append_arrays(st.data, st.positions, st.rotations, st.scales)):
            with pytest.raises(gh.GsplatError, match="gsr_set_scene_rows") as e:
                call()
            assert e.value.code == GSR_ERR_ARG
        assert flat.scene_count() == n and flat.scene_capacity() == n
        with pytest.raises(gh.GsplatError, match="`from` needs") as e:
            r.scene_append_selected(flat)
        assert e.value.code == GSR_ERR_ARG
        unchanged("a destination or a from without rows")
        # n + k above the upload's limit (refused before any pointer is read), a reserve above it
        assert L.gsr_scene_append_arrays(ctx, d.ctypes.data, p.ctypes.data, q.ctypes.data, s.ctypes.data, ar.MAX_ROWS, ctypes.byref(a)) == GSR_ERR_ARG
        assert b"too many" in L.gsr_last_error(ctx)
        assert L.gsr_scene_reserve(ctx, ar.MAX_ROWS + 1) == GSR_ERR_ARG
        unchanged("above the upload's limit")
        # a destination that has SH rows
        r.set_sh(tex, band)
        for call in (r.scene_duplicate_selected, lambda: r.scene_append_selected(r), lambda: r.scene_append_arrays(st.data, st.positions, st.rotations, st.scales)):
            with pytest.raises(gh.GsplatError, match="SH rows") as e:
                call()
            assert e.value.code == GSR_ERR_ARG
        unchanged("a destination with SH rows")
        assert all(np.array_equal(x, y) for x, y in zip(r.read_scene_sh()[0], tex))
    finally:
        r.dispose()
        flat.dispose()


def test_refusals_leave_the_scene_untouched(oracle):
    _refusals(oracle)


def test_bounds_twin_counts_nothing_over_the_same_walk(oracle):
    import gsplat_hip as gh
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    for n in COUNTS:
        _walk(oracle, n, lib_path=BOUNDS_LIB)   # every size, every selection, the frames at 20000 included
    _refusals(oracle, lib_path=BOUNDS_LIB)
    for name in ("gsr_debug_bounds_append", "gsr_debug_bounds_scene", "gsr_debug_bounds_edit", "gsr_debug_bounds_select"):
        buf = (ctypes.c_uint32 * 8)()
        assert getattr(L, name)(buf) == 0
        assert list(buf) == [0] * 8, name


SET_COUNTS = (1, 63, 65, 8191, 8193)   # a word is 32 splats, a wave's ballot 64, one k_select_apply workgroup 256 words = 8192 splats


def _set_layout_bytes(capacity, with_rows=True):
    """scene_bytes of a scene with both sets allocated, no region bytes, no SH and no contribution accumulators, from the documented
    layout: 7 (15 with rotations / scales) words per capacity row; the selection's two and the hidden set's three word buffers of
    the capacity's fold words (even, at least 2); for each set two counter words and one per 256 words"""
    fold = max((-(-capacity // 32) + 1) & ~1, 2)
    counters = 2 + -(-fold // 256)
    return 4 * (capacity * (15 if with_rows else 7) + (2 + 3) * fold + 2 * counters)


def _sets_through_growth(oracle, n, lib_path=None):
    import gsplat_hip as gh
    mix = (np.arange(n, dtype=np.uint64) * 2654435761 % 2 ** 32) >> 7   # fixed pseudo-random thirds; splat 0 is selected
    sel, third, hid = mix % 3 == 0, mix % 3 == 1, np.zeros(n, dtype=bool)   # (sel, hid: what the device is expected to hold)
    st = _state(oracle, n)
    r = gh.HIPRenderer(W, H, lib_path=lib_path)

    def same(what):
        assert np.array_equal(r.selection_words(), hr.pack(sel)) and r.selection_count() == int(sel.sum()), (what, n, "selection")   # (pack: tail bits zero)
        assert np.array_equal(r.hidden_words(), hr.pack(hid)) and r.hidden_count() == int(hid.sum()), (what, n, "hidden set")

    try:
        r.set_scene_arrays(st.data, st.positions, st.rotations, st.scales)
        assert r.set_selection(sel) == int(sel.sum())
        same("select")
        hid = hr.hidden_set(hid, third)
        assert r.set_hidden(third) == int(hid.sum())
        same("hide")
        got = r.scene_duplicate_selected()   # past the allocated words at the small sizes, past one apply workgroup at 8191
        want = ar.duplicate(st, sel)
        assert tuple(got) == tuple(want) == (n, int(sel.sum()))
        sel, hid = ar.selection_after(st.n, *want), ar.hidden_after(hid, want[1])   # the new rows selected and not hidden
        same("duplicate")
        capacity = ar.capacity_after(n, st.n)
        assert r.scene_capacity() == capacity and r.scene_count() == st.n
        sel = ~sel
        assert r.invert_selection() == int(sel.sum())
        same("invert")
        hid = hr.hide_selected(hid, sel, "add")
        assert r.hide_selected("add") == int(hid.sum())
        same("hide_selected")
        assert r.scene_sharing() == (1, _set_layout_bytes(capacity))
    finally:
        r.dispose()


@pytest.mark.parametrize("n", SET_COUNTS)
def test_the_sets_survive_growth_across_word_and_workgroup_edges(oracle, n):
    """select a third, hide another third, duplicate, invert, hide the selection: both sets word for word and both counts after every
    step, and the scene's bytes from the documented layout -- on the shipped build and on the bounds-checked twin, which counts nothing"""
    import gsplat_hip as gh
    _sets_through_growth(oracle, n)
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    _sets_through_growth(oracle, n, lib_path=BOUNDS_LIB)
    for name in ("gsr_debug_bounds_append", "gsr_debug_bounds_select", "gsr_debug_bounds_scene", "gsr_debug_bounds_edit"):
        buf = (ctypes.c_uint32 * 8)()
        assert getattr(L, name)(buf) == 0
        assert list(buf) == [0] * 8, name

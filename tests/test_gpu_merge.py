"""Merging cells on the GPU: gsr_cells and gsr_scene_merge_cells (k_merge.hip, gsr_merge.cpp) against tests/merge_reference.py, the
specification in Python f64, EXACTLY: every array read back after the edit -- positions, rotations and scales as bit patterns, the
covariance words, rgba -- and leader, hist, every info field but pair_bound, and new_count.  pair_bound is at least the sum of m over
the candidates and at most the budget.  The shapes are merge_reference.families(); the state checks follow them."""
import ctypes
import os

import numpy as np
import pytest

import attr_reference as ar
import merge_reference as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
W, H, FX = 128, 96, 110.0
GSR_ERR_ARG = -1
FAMILIES = mr.families()
BY_NAME = {f[0]: f for f in FAMILIES}
BIG = "8192 clustered"
_WANT = {}


def _want(key, arrays, cell, mask=None, hidden=None):
    """the reference's merge, computed once per key, shared and left unchanged"""
    if key not in _WANT:
        _WANT[key] = mr.merge(*arrays, cell, mask, hidden)
    return _WANT[key]


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


@pytest.fixture(scope="module")
def r(gh):
    x = gh.HIPRenderer(W, H)
    yield x
    x.dispose()


def _load(x, arrays):
    x.set_scene_arrays(*[a.reshape(-1) for a in arrays])
    x.set_selection(None)
    x.set_hidden(None)


def _read(x):
    data, pos, rot, scl = x.read_scene()
    return data.reshape(-1, 8), pos.reshape(-1, 3), rot.reshape(-1, 4), scl.reshape(-1, 3)


def _same_scene(got, want, what):
    for name, a, b in zip(("data", "positions", "rotations", "scales"), got, want):
        a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
        assert not bad.size, (what, name, bad[:8], a[bad[:2]], b[bad[:2]])


def _scope_names(scope):
    return tuple(name for name, bit in (("selected", 1), ("visible", 2)) if scope & bit)


def _check_info(info, want, arrays, cell, mask, what):
    print(what, info)
    for key, v in want.items():
        assert info[key] == v, (what, key, info[key], v)
    assert mr.pair_floor(arrays[1], arrays[2], arrays[3], cell, mask) <= info["pair_bound"] <= info["budget"], what


def _check_report(x, arrays, cell, mask=None, scope=0, what="", caps=(64, 1, 3)):
    n = arrays[1].shape[0]
    for cap in caps:
        wl, wh, winfo = mr.report(arrays[1], arrays[2], arrays[3], cell, cap, mask)
        leader, hist, info = x.cells(cell, cap=cap, scope=_scope_names(scope), leaders=True)
        assert leader.dtype == np.uint32 and leader.shape == (n,) and hist.shape == (cap + 1,)
        assert np.array_equal(leader, wl), (what, np.nonzero(leader != wl)[0][:8])
        assert np.array_equal(hist, wh) and hist[0] == 0 and int(hist.sum()) == winfo["cells"], (what, cap, hist[:8], wh[:8])
        _check_info(info, winfo, arrays, cell, mask, "%s cap %d" % (what, cap))
        lead2, hist2, info2 = x.cells(cell, cap=cap, scope=_scope_names(scope))       # the leaders are optional
        assert lead2 is None and np.array_equal(hist2, hist) and info2 == info
    return info


def _check_merge(x, key, arrays, cell, mask=None, scope=0, hidden=None, what=""):
    """the report, then the edit: every array, the count, the info, the selection and the hidden set against the reference"""
    want = _want(key, arrays, cell, mask, hidden)
    announced = _check_report(x, arrays, cell, mask, scope, what, caps=(64,))
    before = x.selection_words().copy()
    count, info = x.scene_merge_cells(cell, scope=_scope_names(scope))
    _check_info(info, want["info"], arrays, cell, mask, what + " merge")
    assert count == want["info"]["rows_after"] == announced["rows_after"] == x.scene_count(), (what, count)
    _same_scene(_read(x), (want["data"], want["positions"], want["rotations"], want["scales"]), what)
    if want["info"]["merged_cells"]:
        assert np.array_equal(x.selection_words(), ar.pack(want["merged"])), what      # the selection is exactly the merged rows
        assert x.selection_count() == want["info"]["merged_cells"]
    else:
        assert np.array_equal(x.selection_words(), before), what                       # nothing to merge: nothing changes
    assert np.array_equal(x.hidden_words(), ar.pack(want["hidden"])), what
    return want


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_report_and_merged_scene_equal_the_reference(r, case):
    name, arrays, cell = case
    _load(r, arrays)
    want = _check_merge(r, name, arrays, cell, what=name)
    # stateless: the same call now describes the merged scene, and merging it again is the reference's second merge
    left = (want["data"], want["positions"], want["rotations"], want["scales"])
    _check_merge(r, name + " again", left, cell, what=name + " again")


def test_small_cases_by_hand(r):
    _, arrays, cell = BY_NAME["one splat"]
    _load(r, arrays)
    leader, hist, info = r.cells(cell, cap=2, leaders=True)
    assert leader.tolist() == [0] and hist.tolist() == [0, 1, 0] and info["rows_after"] == 1 and info["merged_cells"] == 0
    assert r.scene_merge_cells(cell)[0] == 1
    _same_scene(_read(r), arrays, "one splat")
    _, arrays, cell = BY_NAME["two splats in two cells"]
    _load(r, arrays)
    assert r.cells(cell, cap=2, leaders=True)[0].tolist() == [0, 1] and r.scene_merge_cells(cell)[0] == 2
    _same_scene(_read(r), arrays, "two cells")
    _, arrays, cell = BY_NAME["two splats in one cell"]
    _load(r, arrays)
    leader, hist, info = r.cells(cell, cap=2, leaders=True)
    assert leader.tolist() == [0, 0] and hist.tolist() == [0, 0, 1] and info["rows_after"] == 1 and info["largest"] == 2
    assert r.scene_merge_cells(cell)[0] == 1 and r.selection().tolist() == [True]
    _, arrays, cell = BY_NAME["non-finite rows"]
    _load(r, arrays)
    leader = r.cells(cell, leaders=True)[0]
    assert (leader[[2, 5, 7, 8, 9, 10]] == mr.NONE).all() and (leader[[0, 1, 3, 4, 6, 11]] == 0).all()
    r.scene_merge_cells(cell)
    data, pos, rot, scl = _read(r)
    keep = [2, 5, 7, 8, 9, 10]                                          # kept bit for bit, NaN payloads and all, behind the merged row
    _same_scene((data[1:], pos[1:], rot[1:], scl[1:]), tuple(a[keep] for a in arrays), "non-finite rows")


def _sets(n):
    return np.arange(n) % 7 < 5, np.arange(n) % 3 == 1


@pytest.mark.parametrize("scope", [0, 1, 2, 3])
def test_every_scope_on_the_clustered_scene(r, scope):
    _, arrays, cell = BY_NAME[BIG]
    n = arrays[1].shape[0]
    sel, hid = _sets(n)
    _load(r, arrays)
    r.set_selection(sel)
    r.set_hidden(hid)
    mask = ar.in_scope(n, scope, ar.pack(sel), ar.pack(hid))
    want = _check_merge(r, "%s scope %d" % (BIG, scope), arrays, cell, None if scope == 0 else mask, scope, hid, "%s scope %d" % (BIG, scope))
    assert 0 < want["info"]["merged_cells"] and want["hidden"].any()
    out = ~mask & want["keep"] if scope else np.zeros(n, bool)
    if scope:                                                           # the rows out of scope are all still there
        assert int(out.sum()) == int((~mask).sum())
    r.set_hidden(None)


def _frame(x, cam):
    x.set_camera(cam)
    x._check(x._L.gsr_render(x._ctx))
    return x.lastDepthIndex().copy(), x.readPixelsFloat().copy()


def test_nothing_to_merge_keeps_the_frame_and_the_selection(gh, r):
    _, arrays, _ = BY_NAME[BIG]
    n = arrays[1].shape[0]
    _load(r, arrays)
    sel = np.arange(n) % 5 == 0
    r.set_selection(sel)
    cam = gh.orbit_camera(3, width=W, height=H, fx=FX)
    frame = _frame(r, cam)
    picked = r.pick([(W // 2, H // 2)])
    count, info = r.scene_merge_cells(1e-5)
    assert count == n == info["rows_after"] and info["merged_cells"] == 0 and info["cells"] == info["candidates"] == n
    assert np.array_equal(r.selection_words(), ar.pack(sel)) and r.selection_count() == int(sel.sum())
    assert np.array_equal(r.pick([(W // 2, H // 2)]), picked)           # the last frame is still valid: a pick needs it
    assert np.array_equal(r.readPixelsFloat().view(np.uint32), frame[1].view(np.uint32))
    _same_scene(_read(r), arrays, "no-op")
    # and a real merge invalidates it, like every scene edit
    r.scene_merge_cells(0.08)
    with pytest.raises(gh.GsplatError):
        r.pick([(W // 2, H // 2)])


def test_frame_after_the_merge_equals_a_fresh_context(gh, r):
    _, arrays, cell = BY_NAME[BIG]
    _load(r, arrays)
    cam = gh.orbit_camera(3, width=W, height=H, fx=FX)
    _frame(r, cam)
    count, _ = r.scene_merge_cells(cell)
    got = _frame(r, cam)
    fresh = gh.HIPRenderer(W, H)
    try:
        fresh.set_scene_arrays(*r.read_scene())
        assert fresh.scene_count() == count
        want = _frame(fresh, cam)
    finally:
        fresh.dispose()
    assert np.array_equal(got[0], want[0]), "depthIndex"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "image"
    assert got[1].any()


def test_two_members_of_a_shared_scene_both_see_the_merged_scene(gh, r):
    _, arrays, cell = BY_NAME["400 cells of two"]
    _load(r, arrays)
    want = _want("400 cells of two", arrays, cell)
    b = gh.HIPRenderer(W, H)
    try:
        b.share_scene(r)
        assert b.cells(cell)[2]["rows_after"] == 400
        assert b.scene_merge_cells(cell)[0] == 400                      # through the other member
        for m in (r, b):
            assert m.scene_count() == 400
            _same_scene(_read(m), (want["data"], want["positions"], want["rotations"], want["scales"]), "member")
            assert np.array_equal(m.selection_words(), ar.pack(want["merged"]))
            assert m.cells(cell)[2]["merged_cells"] == 0
    finally:
        b.dispose()


def test_the_edit_refuses_sh_rows_and_the_report_answers(gh, r):
    _, arrays, cell = BY_NAME["65 members in one cell"]
    _load(r, arrays)
    n = arrays[1].shape[0]
    r.set_sh([np.zeros(16, np.uint32)] * 3, [n - 3, n - 2, n - 1])
    try:
        assert r.cells(cell)[2]["rows_after"] == 3
        with pytest.raises(gh.GsplatError) as ei:
            r.scene_merge_cells(cell)
        assert ei.value.code == GSR_ERR_ARG and "SH" in str(ei.value)
        _same_scene(_read(r), arrays, "refused for its SH rows")
        assert r.scene_count() == n
    finally:
        _load(r, arrays)                                                # (a new scene drops the SH state)


def test_every_refusal_leaves_the_scene_alone(gh, r):
    _, arrays, cell = BY_NAME["65 members in one cell"]
    _load(r, arrays)
    n = arrays[1].shape[0]
    prior = np.arange(n) % 3 == 0
    r.set_selection(prior)
    L, ctx = r._L, r._ctx
    leader = np.zeros(n, np.uint32)
    info = gh.GsrCellInfo()
    count = ctypes.c_uint32(77)
    rep = lambda cell=cell, cap=8, scope=0, budget=0, m=n: L.gsr_cells(ctx, cell, cap, scope, budget, leader.ctypes.data, m, None, ctypes.byref(info))
    edit = lambda cell=cell, scope=0, budget=0: L.gsr_scene_merge_cells(ctx, cell, scope, budget, ctypes.byref(count), ctypes.byref(info))
    refused = [lambda v=v: rep(cell=v) for v in (0.0, -1.0, np.nan, np.inf, 1e-320, 1.7e308)]
    refused += [lambda v=v: edit(cell=v) for v in (0.0, -0.5, np.nan, np.inf, 1e-320)]
    refused += [lambda: rep(cap=0), lambda: rep(cap=4096), lambda: rep(scope=4), lambda: edit(scope=8)]
    refused += [lambda: rep(m=n - 1), lambda: rep(m=n + 1)]
    refused += [lambda: rep(budget=mr.MAX_BUDGET + 1), lambda: edit(budget=mr.MAX_BUDGET + 1), lambda: rep(budget=1), lambda: edit(budget=1)]
    for t, call in enumerate(refused):
        assert call() == GSR_ERR_ARG, t
        assert L.gsr_last_error(ctx), t
        assert count.value == 77 and not leader.any(), t
        assert r.selection_count() == int(prior.sum()) and r.scene_count() == n, t
    _same_scene(_read(r), arrays, "refusals")
    assert np.array_equal(r.selection_words(), ar.pack(prior))
    assert L.gsr_cells(None, cell, 8, 0, 0, None, 0, None, None) == GSR_ERR_ARG
    assert L.gsr_scene_merge_cells(None, cell, 0, 0, None, None) == GSR_ERR_ARG
    # a scene without rotations and scales
    r.set_raw_scene(arrays[0].reshape(-1), arrays[1].reshape(-1))
    assert rep() == GSR_ERR_ARG and edit() == GSR_ERR_ARG and r.scene_count() == n
    # and what is NOT refused: every pointer NULL
    _load(r, arrays)
    assert L.gsr_cells(ctx, cell, 8, 0, 0, None, 0, None, None) == 0
    assert L.gsr_scene_merge_cells(ctx, cell, 0, 0, None, None) == 0 and r.scene_count() == 3
    for bad in (0, 4096):
        with pytest.raises(ValueError):
            r.cells(cell, cap=bad)


def test_a_budget_of_one_fills_info_and_launches_no_walk(gh, r):
    _, arrays, cell = BY_NAME[BIG]
    _load(r, arrays)
    n = arrays[1].shape[0]
    for call in (lambda: r.cells(cell, budget=1), lambda: r.scene_merge_cells(cell, budget=1)):
        with pytest.raises(gh.GsplatError) as ei:
            call()
        assert ei.value.code == GSR_ERR_ARG
        info = ei.value.info
        assert info["budget"] == 1 and info["in_scope"] == info["candidates"] == n and info["pair_bound"] >= mr.pair_floor(arrays[1], arrays[2], arrays[3], cell)
        assert info["cells"] == info["merged_cells"] == info["merged_members"] == info["largest"] == 0       # no walk ran
        assert str(info["pair_bound"]) in str(ei.value) and "budget of 1" in str(ei.value)
    _same_scene(_read(r), arrays, "budget")
    info = r.cells(cell)[2]
    assert r.cells(cell, budget=info["pair_bound"])[2]["budget"] == info["pair_bound"]       # at the bound: not above it


def test_an_empty_scene_and_an_empty_scope_return_zeros(gh, r):
    _, arrays, cell = BY_NAME["64 members in one cell"]
    _load(r, arrays)
    n = arrays[1].shape[0]
    leader, hist, info = r.cells(cell, cap=4, scope="selected", leaders=True)
    assert (leader == mr.NONE).all() and not hist.any() and info["rows_after"] == n
    assert info["in_scope"] == info["candidates"] == info["cells"] == info["pair_bound"] == 0
    assert r.scene_merge_cells(cell, scope=("selected", "visible"))[0] == n
    _same_scene(_read(r), arrays, "empty scope")
    e = gh.HIPRenderer(W, H)                                            # (never given a scene: the empty one)
    try:
        leader, hist, info = e.cells(cell, leaders=True)
        assert leader.size == 0 and not hist.any() and info["in_scope"] == info["rows_after"] == 0 and info["budget"] == mr.DEFAULT_BUDGET
        assert e.scene_merge_cells(cell)[0] == 0
    finally:
        e.dispose()


def _scratch(x):
    fn = x._L.gsr_debug_merge_scratch
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    out = ctypes.c_uint64(1)
    assert fn(x._ctx, ctypes.byref(out)) == 0
    return out.value


def test_a_context_that_never_calls_it_allocates_nothing(gh):
    _, arrays, cell = BY_NAME["257 members in one cell"]
    x = gh.HIPRenderer(W, H)
    try:
        _load(x, arrays)
        x.neighbours(0.05)
        assert _scratch(x) == 0
        n = arrays[1].shape[0]
        words = max((-(-n // 32) + 1) & ~1, 2)
        x.cells(cell)
        assert _scratch(x) == 32 + 4 * words + 12 * n                   # the report's share only
        x.scene_merge_cells(cell)
        assert _scratch(x) == 32 + 4 * words + 12 * n + 8 * n + 8 * (n // 2 + 1) + 12 * words
    finally:
        x.dispose()


def test_bounds_twin_counts_nothing(gh):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    x = gh.HIPRenderer(W, H, lib_path=BOUNDS_LIB)
    try:
        for name in ("one splat", "two splats in one cell", "two splats in two cells", "65 members in one cell", "257 members in one cell",
                     "lattice on the cell edges", "rows beyond the clamp", "400 cells of two", "non-finite rows"):
            _, arrays, cell = BY_NAME[name]
            _load(x, arrays)
            _check_merge(x, name, arrays, cell, what="bounds twin " + name)
        _, arrays, cell = BY_NAME[BIG]
        n = arrays[1].shape[0]
        sel, hid = _sets(n)
        _load(x, arrays)
        x.set_selection(sel)
        x.set_hidden(hid)
        _check_merge(x, "%s scope 3" % BIG, arrays, cell, ar.in_scope(n, 3, ar.pack(sel), ar.pack(hid)), 3, hid, "bounds twin scope 3")
        buf = (ctypes.c_uint32 * 8)()
        for unit in ("merge", "neighbours", "scene"):
            assert getattr(L, "gsr_debug_bounds_" + unit)(buf) == 0
            assert list(buf) == [0] * 8, unit
    finally:
        x.dispose()

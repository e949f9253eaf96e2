"""Neighbours on the GPU: gsr_neighbours and gsr_select_neighbours (k_neighbours.hip, gsr_neighbours.cpp) against
tests/neighbour_reference.py, the blocked O(n^2) specification in numpy f64, EXACTLY: counts, histogram, info and the selection's
words bit for bit.  The shapes are neighbour_reference.families(): the smallest that can still go wrong -- one and two splats, the
wave and workgroup edges, coincident splats under a small and the largest cap, lattices at exact multiples of the radius through
negative coordinates, 2^19 radii out and beyond the cell clamp, non-finite rows, and 8192 splats of clusters with floaters."""
import ctypes
import os

import numpy as np
import pytest

import attr_reference as ar
import neighbour_reference as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
W, H = 128, 96
GSR_ERR_ARG = -1
OPS = {"replace": 0, "add": 1, "subtract": 2, "intersect": 3}
FAMILIES = nr.families()
BY_NAME = {f[0]: f for f in FAMILIES}
_WANT = {}


def _want(name, scope_key=None, mask=None):
    """the reference's counts of a family in a scope, computed once"""
    key = (name, scope_key)
    if key not in _WANT:
        _, p, radius, cap = BY_NAME[name]
        _WANT[key] = nr.counts(p, radius, cap, mask)
        _WANT[key].setflags(write=False)
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


def _arrays(p, seed=1):
    """(data, positions, rotations, scales) around the positions p"""
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    data[:, 0:3] = p.view(np.uint32)
    rot = rng.normal(0, 1, (n, 4)).astype(np.float32)
    scl = rng.uniform(0.01, 0.1, (n, 3)).astype(np.float32)
    return data.reshape(-1), p.reshape(-1), rot.reshape(-1), scl.reshape(-1)


def _scope_names(scope):
    return tuple(name for name, bit in (("selected", 1), ("visible", 2)) if scope & bit)


def _check(r, p, radius, cap, want, mask=None, scope=0, what=""):
    """counts, hist and info of one call against the reference; returns (hist, info)"""
    n = np.asarray(p).reshape(-1, 3).shape[0]
    counts, hist, info = r.neighbours(radius, cap=cap, scope=_scope_names(scope))
    print(what, "in_scope", info["in_scope"], "nonfinite", info["nonfinite"], "pair_bound", info["pair_bound"])
    assert counts.dtype == np.uint32 and counts.shape == (n,) and hist.shape == (cap + 1,)
    assert np.array_equal(counts, want), (what, np.nonzero(counts != want)[0][:8])
    assert np.array_equal(hist, nr.hist(want, cap, mask)), what
    in_scope = n if mask is None else int(np.asarray(mask).sum())
    assert info["in_scope"] == in_scope == int(hist.sum()), what
    assert info["nonfinite"] == nr.nonfinite(p, mask), what
    assert info["budget"] == nr.DEFAULT_BUDGET
    assert nr.pair_floor(p, radius, mask) <= info["pair_bound"] <= info["budget"], what
    return hist, info


def _check_select(r, want, lo, hi, radius, cap, mask=None, scope=0, op="replace", prior=None, what=""):
    got, info = r.select_neighbours(radius, lo=lo, hi=hi, cap=cap, scope=_scope_names(scope), op=op)
    picked = nr.select(want, lo, hi, mask)
    after = picked if prior is None else ar.fold(prior, picked, OPS[op])
    assert got == int(after.sum()) == r.selection_count(), (what, got, int(after.sum()))
    assert np.array_equal(r.selection_words(), ar.pack(after)), what
    return after


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_counts_histogram_info_and_selection_equal_the_reference(r, case):
    name, p, radius, cap = case
    r.set_scene_arrays(*_arrays(p))
    want = _want(name)
    hist, _ = _check(r, p, radius, cap, want, what=name)
    for lo, hi in ((0, 1), (0, cap + 1), (1, min(3, cap + 1)), (cap, cap + 1), (2, 2)):
        after = _check_select(r, want, lo, hi, radius, cap, what="%s [%d, %d)" % (name, lo, hi))
        assert int(after.sum()) == int(hist[lo:hi].sum())              # the consistency guarantee
    # a scope: every third splat hidden, the walk sees only the others
    n = p.shape[0]
    hid = np.arange(n) % 3 == 1
    r.set_hidden(hid)
    want_vis = _want(name, "visible", ~hid)
    _check(r, p, radius, cap, want_vis, ~hid, 2, name + " visible")
    r.set_hidden(None)


def test_small_cases_by_hand(r):
    _, p, radius, cap = BY_NAME["n = 2 at exactly radius"]
    r.set_scene_arrays(*_arrays(p))
    assert r.neighbours(radius, cap=cap)[0].tolist() == [1, 1]
    _, p, radius, cap = BY_NAME["n = 2 one ulp beyond"]
    r.set_scene_arrays(*_arrays(p))
    assert r.neighbours(radius, cap=cap)[0].tolist() == [0, 0]
    _, p, radius, cap = BY_NAME["300 coincident, cap 7"]
    r.set_scene_arrays(*_arrays(p))
    counts, hist, _ = r.neighbours(radius, cap=cap)
    assert (counts == 7).all() and hist.tolist() == [0] * 7 + [300]
    counts, hist, _ = r.neighbours(radius, cap=nr.MAX_CAP)
    assert (counts == 299).all() and hist[299] == 300 and int(hist.sum()) == 300 and hist[nr.MAX_CAP] == 0
    counts, hist, info = r.neighbours(radius, cap=3, counts=False, hist=False)
    assert counts is None and hist is None and info["in_scope"] == 300


def _cluster_scene(r):
    name, p, radius, cap = BY_NAME["clusters and floaters"]
    r.set_scene_arrays(*_arrays(p))
    return name, p, radius, cap


def test_every_scope_after_select_box_and_hide_selected(r):
    name, p, radius, cap = _cluster_scene(r)
    n = p.shape[0]
    box = (-1.0, 0.4, -1.0, 0.6, -1.0, 1.0)
    r.select_box(box)
    r.hide_selected()
    hid = ar.unpack(r.hidden_words(), n)
    assert 0 < hid.sum() < n
    r.select_box((-0.2, 30.0, -30.0, 30.0, -30.0, 30.0))
    sel = ar.unpack(r.selection_words(), n)
    assert 0 < (sel & hid).sum() < sel.sum() < n
    for scope in (0, 1, 2, 3):
        mask = ar.in_scope(n, scope, ar.pack(sel), ar.pack(hid))
        want = _want(name, "scope %d" % scope, None if scope == 0 else mask)
        _check(r, p, radius, cap, want, None if scope == 0 else mask, scope, "%s scope %d" % (name, scope))
        assert np.array_equal(r.selection_words(), ar.pack(sel))       # gsr_neighbours reads the selection and leaves it
    r.set_hidden(None)


def test_select_with_every_op(r):
    name, p, radius, cap = _cluster_scene(r)
    n = p.shape[0]
    want = _want(name)
    prior = np.arange(n) % 7 < 3
    for op in OPS:
        r.set_selection(prior)
        _check_select(r, want, 0, 4, radius, cap, op=op, prior=prior, what=op)
    # in the selected scope the pick is made among the selected, counted among the selected
    r.set_selection(prior)
    want_sel = _want(name, "selected %7<3", prior)
    _check_select(r, want_sel, 0, 2, radius, cap, mask=prior, scope=1, op="intersect", prior=prior, what="selected scope")


def test_the_floater_filter_leaves_the_references_survivors(r):
    name, p, radius, cap = _cluster_scene(r)
    want = _want(name)
    k = 3
    floaters = nr.select(want, 0, k)
    assert 150 <= floaters.sum() < p.shape[0] // 4                     # the scattered ones, and a few of the clusters' own edges
    got, _ = r.select_neighbours(radius, hi=k, cap=cap)
    assert got == int(floaters.sum())
    assert r.scene_erase_selected() == p.shape[0] - got
    left = r.read_scene()[1].reshape(-1, 3)
    assert np.array_equal(left.view(np.uint32), p[~floaters].view(np.uint32))
    # stateless: the same call now describes the scene that is left
    want_left = nr.counts(left, radius, cap)
    _check(r, left, radius, cap, want_left, what="after the erase")
    assert (want_left < k).any()                                       # (removing floaters can strand their neighbours: the filter is one pass)


def test_the_call_follows_an_edit_of_the_scene(r):
    _, p, radius, cap = BY_NAME["n = 257"]
    r.set_scene_arrays(*_arrays(p))
    n = p.shape[0]
    moved = np.arange(n) % 2 == 0
    r.set_selection(moved)
    r.scene_translate_selected((0.25, 0.0, -0.125))
    now = r.read_scene()[1].reshape(-1, 3)
    assert not np.array_equal(now, p)
    _check(r, now, radius, cap, nr.counts(now, radius, cap), what="after translate_selected")
    _check(r, now, radius, cap, nr.counts(now, radius, cap, moved), moved, 1, "after translate_selected, selected")


def test_two_members_of_a_shared_scene_agree(gh, r):
    name, p, radius, cap = _cluster_scene(r)
    b = gh.HIPRenderer(W, H)
    try:
        b.share_scene(r)
        want = _want(name)
        for m in (r, b):
            _check(m, p, radius, cap, want, what="member")
        assert b.select_neighbours(radius, hi=2, cap=cap)[0] == r.selection_count() == int(nr.select(want, 0, 2).sum())
    finally:
        b.dispose()


def test_the_budget(gh, r):
    p = np.tile(np.array([[0.5, 0.5, 0.5]], np.float32), (512, 1))
    r.set_scene_arrays(*_arrays(p))
    radius, cap = 0.01, 8
    floor = nr.pair_floor(p, radius)
    assert floor == 512 * 512
    prior = np.arange(512) % 5 == 0
    r.set_selection(prior)
    for call in (lambda: r.neighbours(radius, cap=cap, budget=1), lambda: r.select_neighbours(radius, hi=2, cap=cap, budget=1)):
        with pytest.raises(gh.GsplatError) as ei:
            call()
        assert ei.value.code == GSR_ERR_ARG
        info = ei.value.info
        assert info["budget"] == 1 and info["in_scope"] == 512 and info["nonfinite"] == 0 and info["pair_bound"] >= floor
        assert str(info["pair_bound"]) in str(ei.value) and "budget of 1" in str(ei.value)   # the message names both numbers
        assert r.selection_count() == int(prior.sum()) and np.array_equal(r.selection_words(), ar.pack(prior))
    counts, _, info = r.neighbours(radius, cap=cap)                    # the default budget passes
    assert (counts == cap).all() and info["budget"] == nr.DEFAULT_BUDGET and floor <= info["pair_bound"]
    assert r.neighbours(radius, cap=cap, budget=info["pair_bound"])[2]["budget"] == info["pair_bound"]   # at the bound: not above it
    with pytest.raises(gh.GsplatError) as ei:
        r.neighbours(radius, cap=cap, budget=nr.MAX_BUDGET + 1)
    assert ei.value.code == GSR_ERR_ARG and "GSR_NEIGHBOUR_MAX_BUDGET" in str(ei.value)
    assert r.neighbours(radius, cap=cap, budget=nr.MAX_BUDGET)[2]["budget"] == nr.MAX_BUDGET


def test_every_refusal_leaves_the_selection_alone(gh, r):
    _, p, radius, cap = BY_NAME["n = 65"]
    r.set_scene_arrays(*_arrays(p))
    n = p.shape[0]
    prior = np.arange(n) % 3 == 0
    r.set_selection(prior)
    L, ctx = r._L, r._ctx
    counts = np.zeros(n, np.uint32)
    info = gh.GsrNeighbourInfo()
    sel = ctypes.c_uint32(77)
    nb = lambda radius=radius, cap=cap, scope=0, budget=0, m=n: L.gsr_neighbours(ctx, radius, cap, scope, budget, counts.ctypes.data, m, None, ctypes.byref(info))
    pick = lambda radius=radius, cap=cap, scope=0, budget=0, lo=0, hi=1, op=0: L.gsr_select_neighbours(ctx, radius, cap, scope, budget, lo, hi, op,
                                                                                                      ctypes.byref(sel), ctypes.byref(info))
    tiny, huge = 1e-200, 1e200                                         # radius * radius underflows; overflows
    refused = [lambda v=v: nb(radius=v) for v in (0.0, -1.0, np.nan, np.inf, tiny, huge, 5e-324)]
    refused += [lambda v=v: pick(radius=v) for v in (0.0, np.nan, tiny, huge)]
    refused += [lambda: nb(cap=0), lambda: nb(cap=4096), lambda: pick(cap=0), lambda: pick(cap=4096)]
    refused += [lambda: nb(scope=4), lambda: pick(scope=8), lambda: pick(op=4), lambda: pick(op=-1)]
    refused += [lambda: pick(lo=2, hi=1), lambda: pick(hi=cap + 2), lambda: nb(m=n - 1), lambda: nb(m=n + 1)]
    refused += [lambda: nb(budget=nr.MAX_BUDGET + 1), lambda: pick(budget=nr.MAX_BUDGET + 1)]
    for k, call in enumerate(refused):
        assert call() == GSR_ERR_ARG, k
        assert L.gsr_last_error(ctx), k
        assert sel.value == 77 and not counts.any(), k
        assert r.selection_count() == int(prior.sum()), k
    assert np.array_equal(r.selection_words(), ar.pack(prior))
    assert L.gsr_neighbours(None, radius, cap, 0, 0, None, 0, None, None) == GSR_ERR_ARG
    assert L.gsr_select_neighbours(None, radius, cap, 0, 0, 0, 1, 0, None, None) == GSR_ERR_ARG
    # and what is NOT refused: every pointer NULL, lo == hi, hi == cap + 1
    assert L.gsr_neighbours(ctx, radius, cap, 0, 0, None, 0, None, None) == 0
    assert pick(lo=cap + 1, hi=cap + 1, op=1) == 0 and sel.value == int(prior.sum())
    assert np.array_equal(r.selection_words(), ar.pack(prior))


def test_an_empty_scene_and_an_empty_scope_return_zeros(gh, r):
    _, p, radius, cap = BY_NAME["n = 64"]
    r.set_scene_arrays(*_arrays(p))
    r.set_selection(None)
    counts, hist, info = r.neighbours(radius, cap=cap, scope="selected")
    assert not counts.any() and not hist.any() and info["in_scope"] == info["nonfinite"] == info["pair_bound"] == 0
    assert r.select_neighbours(radius, cap=cap, scope=("selected", "visible"))[0] == 0
    e = gh.HIPRenderer(W, H)                                           # (never given a scene: the empty one)
    try:
        counts, hist, info = e.neighbours(radius, cap=cap)
        assert counts.size == 0 and not hist.any() and info == {"in_scope": 0, "nonfinite": 0, "pair_bound": 0, "budget": nr.DEFAULT_BUDGET}
        assert e.select_neighbours(radius, cap=cap)[0] == 0
    finally:
        e.dispose()


def test_bounds_twin_counts_nothing(gh):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    x = gh.HIPRenderer(W, H, lib_path=BOUNDS_LIB)
    try:
        for name in ("n = 1", "n = 65", "n = 257", "300 coincident, cap 7", "lattice beyond the clamp", "non-finite rows", "clusters and floaters"):
            _, p, radius, cap = BY_NAME[name]
            x.set_scene_arrays(*_arrays(p))
            want = _want(name)
            _check(x, p, radius, cap, want, what="bounds twin " + name)
            _check_select(x, want, 0, 2, radius, cap, what="bounds twin " + name)
            _check(x, p, radius, cap, nr.counts(p, radius, cap, nr.select(want, 0, 2)), nr.select(want, 0, 2), 1, "bounds twin selected " + name)
        buf = (ctypes.c_uint32 * 8)()
        assert L.gsr_debug_bounds_neighbours(buf) == 0
        assert list(buf) == [0] * 8
    finally:
        x.dispose()

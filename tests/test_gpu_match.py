"""Matching on the GPU: gsr_match and gsr_select_match (k_match.hip, gsr_match.cpp) against tests/register_reference.py, the
specification in numpy f64, EXACTLY: idx, every integer of info, pairs and the selection's words as integers, d2, d2_min / d2_max
and the 16 sums by their 64-bit patterns.  The shapes are register_reference.families(): the smallest that can still go wrong --
one splat against one, the wave, workgroup and tree-group edges against 300 targets, the tree's third level and its padding,
coincident targets, a lattice whose spacing is the radius, queries exactly on cell faces, coordinates 2^19 radii out and beyond the
cell clamp, non-finite rows on both sides and a transform that overflows for some rows."""
import ctypes
import math
import os

import numpy as np
import pytest

import attr_reference as ar
import register_reference as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
W, H = 128, 96
GSR_ERR_ARG = -1
OPS = {"replace": 0, "add": 1, "subtract": 2, "intersect": 3}
FAMILIES = rr.families()
BY_NAME = {f[0]: f for f in FAMILIES}
SMALL = [f[0] for f in FAMILIES if f[1].shape[0] < 4096]
_WANT = {}


def _want(name, key=None, smask=None, tmask=None):
    """the reference's (idx, d2, info, pairs, sum16) of a family under a pair of scopes, computed once"""
    if (name, key) not in _WANT:
        _, src, tgt, radius, M = BY_NAME[name]
        idx, d2, info = rr.match(src, tgt, radius, M, smask, tmask)
        pairs, s16 = rr.sums(src, tgt, idx, d2, M)
        for a in (idx, d2, s16):
            a.setflags(write=False)
        _WANT[(name, key)] = (idx, d2, info, pairs, s16)
    return _WANT[(name, key)]


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


@pytest.fixture(scope="module")
def pair(gh):
    """(source renderer, target renderer)"""
    a, b = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    yield a, b
    a.dispose()
    b.dispose()


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


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_info(got, want, what):
    assert set(got) == set(want), what
    for k, v in want.items():
        if k in ("d2_min", "d2_max"):
            assert _bits([got[k]])[0] == _bits([v])[0], (what, k, got[k], v)
        else:
            assert got[k] == v, (what, k, got[k], v)


def _check(a, b, case, want, scope=(), target_scope=(), what=""):
    """idx, d2, sums and info of one match against the reference; returns d2"""
    name, src, tgt, radius, M = case
    widx, wd2, winfo, wpairs, wsum = want
    idx, d2, sums, info = a.match(b, radius, transform=M, scope=scope, target_scope=target_scope, sums=True)
    print(what, info, sums["pairs"])
    assert idx.dtype == np.uint32 and d2.dtype == np.float64 and idx.shape == d2.shape == (src.shape[0],)
    assert np.array_equal(idx, widx), (what, np.nonzero(idx != widx)[0][:8])
    assert np.array_equal(_bits(d2), _bits(wd2)), (what, np.nonzero(_bits(d2) != _bits(wd2))[0][:8])
    _same_info(info, winfo, what)
    assert sums["pairs"] == wpairs == info["matched"], what
    assert np.array_equal(_bits(sums["sum"]), _bits(wsum)), (what, sums["sum"], wsum)
    # without the sums, without the arrays: the same info, nothing else
    i2, d22, s2, info2 = a.match(b, radius, transform=M, scope=scope, target_scope=target_scope, idx=False, d2=False)
    assert i2 is None and d22 is None and s2 is None
    _same_info(info2, winfo, what + " (info only)")
    return d2


def _ranges(v):
    """value ranges that cut a family's finite values in two, take the +inf ones in (hi=None) and leave them out (a finite hi):
    tests/test_gpu_knn.py::_ranges"""
    fin = np.sort(v[np.isfinite(v)])
    mid = float(fin[fin.size // 2]) if fin.size else 0.5
    top = float(fin[-1]) if fin.size else 1.0
    return ((0.0, None), (0.0, 1e300), (mid, None), (0.0, mid), (mid, top), (top, np.nextafter(top, np.inf)), (mid, mid), (np.inf, None), (np.inf, np.inf))


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_match_sums_info_and_selection_equal_the_reference(pair, case):
    a, b = pair
    name, src, tgt, radius, M = case
    n, m = src.shape[0], tgt.shape[0]
    a.set_scene_arrays(*_arrays(src))
    b.set_scene_arrays(*_arrays(tgt, seed=2))
    d2 = _check(a, b, case, _want(name), what=name)
    # the picker over ranges of the distance, and the consistency guarantee
    with np.errstate(invalid="ignore"):
        v = np.sqrt(d2)
    for lo, hi in _ranges(v) if n < 4096 else ((0.0, radius), (radius / 2, None)):
        picked = rr.select(d2, lo, hi)
        got, info = a.select_match(b, radius, lo=lo, hi=hi, transform=M)
        assert got == int(picked.sum()) == a.selection_count(), (name, lo, hi)
        assert np.array_equal(a.selection_words(), ar.pack(picked)), (name, lo, hi)
        _same_info(info, _want(name)[2], name)
    if n >= 4096:
        return
    # every op over a prior selection
    picked = rr.select(d2, 0.0, radius / 2)
    prior = np.arange(n) % 7 < 3
    for op in OPS:
        a.set_selection(prior)
        got, _ = a.select_match(b, radius, lo=0.0, hi=radius / 2, transform=M, op=op)
        after = ar.fold(prior, picked, OPS[op])
        assert got == int(after.sum()) == a.selection_count(), (name, op)
        assert np.array_equal(a.selection_words(), ar.pack(after)), (name, op)
    # scopes: on the source, on the target, on both; neither side's sets are changed by gsr_match
    hid = np.arange(n) % 3 == 1
    sel = np.arange(n) % 5 != 2
    thid = np.arange(m) % 4 == 2
    tsel = np.arange(m) % 3 != 1
    a.set_hidden(hid)
    a.set_selection(sel)
    b.set_hidden(thid)
    b.set_selection(tsel)
    try:
        _check(a, b, case, _want(name, "source visible", ~hid, None), scope="visible", what=name + " source visible")
        _check(a, b, case, _want(name, "target selected", None, tsel), target_scope="selected", what=name + " target selected")
        both = _want(name, "both", sel & ~hid, tsel & ~thid)
        d2 = _check(a, b, case, both, scope=("selected", "visible"), target_scope=("selected", "visible"), what=name + " both")
        assert np.array_equal(a.selection_words(), ar.pack(sel)) and np.array_equal(b.selection_words(), ar.pack(tsel))
        picked = rr.select(d2, 0.0, None, sel & ~hid)                  # everything in scope, the unmatched included; nothing outside it
        got, _ = a.select_match(b, radius, transform=M, scope=("selected", "visible"), target_scope=("selected", "visible"))
        assert got == int(picked.sum()) == int((sel & ~hid).sum())
        assert np.array_equal(a.selection_words(), ar.pack(picked))
        assert np.array_equal(b.selection_words(), ar.pack(tsel)) and np.array_equal(b.hidden_words(), ar.pack(thid))
    finally:
        a.set_hidden(None)
        b.set_hidden(None)
        b.set_selection(None)


def test_target_is_the_context_itself(pair):
    a, _ = pair
    p = np.random.default_rng(5).normal(0.0, 0.5, (260, 3)).astype(np.float32)
    p[100:130] = p[10:40]                              # coincident splats: each matches the smallest index among them
    p[200] = np.nan
    a.set_scene_arrays(*_arrays(p))
    idx, d2, sums, info = a.match(a, 0.05, sums=True)
    want = np.arange(260, dtype=np.uint32)
    want[100:130] = np.arange(10, 40)
    want[200] = rr.NONE
    assert np.array_equal(idx, want)
    assert (np.delete(d2, 200) == 0.0).all() and d2[200] == np.inf
    assert info["matched"] == 259 and info["nonfinite"] == 1 and info["target_indexed"] == 259 and info["d2_min"] == info["d2_max"] == 0.0
    widx, wd2, winfo = rr.match(p, p, 0.05)
    _same_info(info, winfo, "self")
    assert np.array_equal(_bits(sums["sum"]), _bits(rr.sums(p, p, widx, wd2)[1]))


def test_members_of_a_shared_scene_as_source_and_as_target(gh, pair):
    a, b = pair
    case = BY_NAME["257 x 300"]
    name, src, tgt, radius, M = case
    a.set_scene_arrays(*_arrays(src))
    b.set_scene_arrays(*_arrays(tgt, seed=2))
    a2, b2 = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    try:
        a2.share_scene(a)
        b2.share_scene(b)
        for s in (a, a2):
            for t in (b, b2):
                _check(s, t, case, _want(name), what="members")
        # a member of the source's own scene as the target, with the identity: every finite splat matches itself
        idx, d2, _, info = a2.match(a, radius)
        assert np.array_equal(idx, np.arange(257, dtype=np.uint32)) and not d2.any() and info["matched"] == 257
    finally:
        a2.dispose()
        b2.dispose()


def test_the_budget(gh, pair):
    a, b = pair
    name, src, tgt, radius, M = BY_NAME["257 x 300"]
    a.set_scene_arrays(*_arrays(src))
    b.set_scene_arrays(*_arrays(tgt, seed=2))
    winfo = _want(name)[2]
    bound = winfo["pair_bound"]
    prior = np.arange(257) % 5 == 0
    a.set_selection(prior)
    for call in (lambda: a.match(b, radius, transform=M, budget=bound - 1), lambda: a.select_match(b, radius, transform=M, budget=bound - 1),
                 lambda: a.register(b, radius, transform=M, budget=bound - 1)):
        with pytest.raises(gh.GsplatError) as ei:
            call()
        assert ei.value.code == GSR_ERR_ARG
        assert str(bound) in str(ei.value) and "budget of %d" % (bound - 1) in str(ei.value)   # the message names both numbers
        assert np.array_equal(a.selection_words(), ar.pack(prior)) and a.selection_count() == int(prior.sum())
        info = getattr(ei.value, "info", None)
        if info is not None:                           # (register carries none)
            assert (info["budget"], info["pair_bound"], info["in_scope"], info["nonfinite"], info["target_indexed"]) == (bound - 1, bound, 257, 0, 300)
            assert info["matched"] == 0 and info["d2_min"] == math.inf and info["d2_max"] == -math.inf
    _, _, _, info = a.match(b, radius, transform=M, budget=bound)      # at the budget: not above it
    assert info["budget"] == bound and info["matched"] == winfo["matched"]
    with pytest.raises(gh.GsplatError) as ei:
        a.match(b, radius, budget=rr.MAX_BUDGET + 1)
    assert ei.value.code == GSR_ERR_ARG and "GSR_NEIGHBOUR_MAX_BUDGET" in str(ei.value)
    assert a.match(b, radius, budget=rr.MAX_BUDGET)[3]["budget"] == rr.MAX_BUDGET


def test_every_refusal_leaves_the_selection_alone(gh, pair):
    a, b = pair
    name, src, tgt, radius, M = BY_NAME["65 x 300"]
    a.set_scene_arrays(*_arrays(src))
    b.set_scene_arrays(*_arrays(tgt, seed=2))
    n = src.shape[0]
    prior = np.arange(n) % 3 == 0
    a.set_selection(prior)
    L, ctx, tctx = a._L, a._ctx, b._ctx
    info, rinfo = gh.GsrMatchInfo(), gh.GsrRegisterInfo()
    sel = ctypes.c_uint32(77)
    idx = np.full(n, 77, np.uint32)
    out = np.full(12, 77.0)
    good = np.ascontiguousarray(M, dtype=np.float64)
    ptr = lambda m: None if m is None else m.ctypes.data
    mat = lambda t=tctx, m=good, r=radius, scope=0, ts=0, budget=0, cnt=n: L.gsr_match(ctx, t, ptr(m), r, scope, ts, budget, idx.ctypes.data, None, cnt, None, ctypes.byref(info))
    pick = lambda t=tctx, m=good, r=radius, scope=0, ts=0, budget=0, lo=0.0, hi=1.0, op=0: L.gsr_select_match(ctx, t, ptr(m), r, scope, ts, budget, lo, hi, op,
                                                                                                                  ctypes.byref(sel), ctypes.byref(info))
    reg = lambda t=tctx, m=good, r=radius, scope=0, ts=0, budget=0, it=4, tol=0.0, ri=rinfo: L.gsr_register(ctx, t, ptr(m), r, scope, ts, budget, it, tol, out.ctypes.data,
                                                                                                             ctypes.byref(ri))
    bad = [good.copy() for _ in range(3)]
    bad[0][0], bad[1][7], bad[2][11] = np.nan, np.inf, -np.inf
    short = gh.GsrRegisterInfo()
    steps = np.zeros(3, np.uint64)
    short.step_pairs, short.step_rows = steps.ctypes.data, 3
    refused = []
    for f in (mat, pick, reg):
        refused += [lambda f=f: f(t=None)]
        refused += [lambda f=f, v=v: f(r=v) for v in (0.0, -1.0, np.nan, np.inf, 1e-200, 1e200)]
        refused += [lambda f=f: f(scope=4), lambda f=f: f(ts=8), lambda f=f: f(budget=rr.MAX_BUDGET + 1)]
        refused += [lambda f=f, m=m: f(m=m) for m in bad]
    refused += [lambda: mat(cnt=n - 1), lambda: mat(cnt=n + 1)]
    refused += [lambda: pick(op=4), lambda: pick(op=-1), lambda: pick(lo=np.nan), lambda: pick(hi=np.nan), lambda: pick(lo=1.0, hi=0.5)]
    refused += [lambda: reg(it=0), lambda: reg(it=257), lambda: reg(tol=-1.0), lambda: reg(tol=np.nan), lambda: reg(ri=short)]
    for k, call in enumerate(refused):
        assert call() == GSR_ERR_ARG, k
        assert L.gsr_last_error(ctx), k
        assert sel.value == 77 and (idx == 77).all() and (out == 77.0).all(), k
        assert a.selection_count() == int(prior.sum()), k
    assert np.array_equal(a.selection_words(), ar.pack(prior))
    assert L.gsr_match(None, tctx, None, radius, 0, 0, 0, None, None, 0, None, None) == GSR_ERR_ARG
    assert L.gsr_select_match(None, tctx, None, radius, 0, 0, 0, 0.0, 1.0, 0, None, None) == GSR_ERR_ARG
    assert L.gsr_register(None, tctx, None, radius, 0, 0, 0, 4, 0.0, None, None) == GSR_ERR_ARG
    # and what is NOT refused: no out pointer at all, a NULL transform, lo == hi, a tolerance of 0 or +inf
    assert L.gsr_match(ctx, tctx, None, radius, 0, 0, 0, None, None, 0, None, None) == 0
    assert L.gsr_register(ctx, tctx, None, radius, 0, 0, 0, 1, np.inf, None, None) == 0
    assert np.array_equal(a.selection_words(), ar.pack(prior))         # neither touches the selection
    assert L.gsr_select_match(ctx, tctx, None, radius, 0, 0, 0, 0.5, 0.5, 1, None, None) == 0


def test_empty_scene_empty_scope_and_empty_target(gh, pair):
    a, b = pair
    name, src, tgt, radius, M = BY_NAME["64 x 300"]
    a.set_scene_arrays(*_arrays(src))
    b.set_scene_arrays(*_arrays(tgt, seed=2))
    a.set_selection(None)
    b.set_selection(None)
    none, nan, inf = np.full(64, rr.NONE, np.uint32), np.full(64, np.nan), np.full(64, np.inf)
    # an empty source scope: every row outside it
    idx, d2, sums, info = a.match(b, radius, transform=M, scope="selected", sums=True)
    assert np.array_equal(idx, none) and np.array_equal(_bits(d2), _bits(nan)) and sums["pairs"] == 0 and not _bits(sums["sum"]).any()
    _same_info(info, rr.match(src, tgt, radius, M, np.zeros(64, bool))[2], "empty scope")
    assert a.select_match(b, radius, transform=M, scope="selected")[0] == 0
    # an empty target scope, and a target without a scene: everything in scope unmatched
    e = gh.HIPRenderer(W, H)                           # (never given a scene: the empty one)
    try:
        for t, ts, tmask, ttgt in ((b, "selected", np.zeros(300, bool), tgt), (e, (), None, np.zeros((0, 3), np.float32))):
            idx, d2, sums, info = a.match(t, radius, transform=M, target_scope=ts, sums=True)
            assert np.array_equal(idx, none) and np.array_equal(_bits(d2), _bits(inf)) and sums["pairs"] == 0 and not _bits(sums["sum"]).any()
            _same_info(info, rr.match(src, ttgt, radius, M, None, tmask)[2], "empty target")
            assert info["in_scope"] == 64 and info["target_indexed"] == 0 and info["pair_bound"] == 0
            assert a.select_match(t, radius, lo=radius, transform=M, target_scope=ts)[0] == 64     # "what the other capture lacks": everything
            Mr, rinfo = a.register(t, radius, transform=M, target_scope=ts, history=True)
            assert rinfo["status"] == "too_few" and rinfo["iterations"] == 1 and rinfo["pairs"] == 0 and rinfo["rms"] == math.inf
            assert np.array_equal(_bits(Mr.reshape(12)), _bits(M)) and rinfo["step_pairs"].tolist() == [0]
        # an empty source scene
        idx, d2, sums, info = e.match(b, radius, sums=True)
        assert idx.size == 0 and d2.size == 0 and sums["pairs"] == 0 and not sums["sum"].any()
        _same_info(info, rr.match(np.zeros((0, 3), np.float32), tgt, radius)[2] | {"target_indexed": 0}, "empty scene")
        assert e.select_match(b, radius)[0] == 0
        assert e.register(b, radius)[1]["status"] == "too_few"
    finally:
        e.dispose()


def test_no_scratch_before_the_first_call(gh):
    x, y = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    try:
        name, src, tgt, radius, M = BY_NAME["257 x 300"]
        x.set_scene_arrays(*_arrays(src))
        y.set_scene_arrays(*_arrays(tgt, seed=2))
        fn = x._L.gsr_debug_match_scratch
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        got = ctypes.c_uint64(99)
        for c in (x, y):
            assert fn(c._ctx, ctypes.byref(got)) == 0 and got.value == 0
        x.match(y, radius, transform=M)
        assert fn(x._ctx, ctypes.byref(got)) == 0 and got.value == 48 + 257 * 12        # the info words, idx and d2; no tree yet
        x.match(y, radius, transform=M, sums=True)
        assert fn(x._ctx, ctypes.byref(got)) == 0 and got.value == 48 + 257 * 12 + 3 * 128   # two groups and their sum: three rows
        assert fn(y._ctx, ctypes.byref(got)) == 0 and got.value == 0                     # the scratch is the source context's
    finally:
        x.dispose()
        y.dispose()


def test_bounds_twin_counts_nothing(gh):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    x, y = gh.HIPRenderer(W, H, lib_path=BOUNDS_LIB), gh.HIPRenderer(W, H, lib_path=BOUNDS_LIB)
    try:
        for name in SMALL:
            case = BY_NAME[name]
            _, src, tgt, radius, M = case
            x.set_scene_arrays(*_arrays(src))
            y.set_scene_arrays(*_arrays(tgt, seed=2))
            d2 = _check(x, y, case, _want(name), what="bounds twin " + name)
            assert x.select_match(y, radius, hi=radius, transform=M)[0] == int(rr.select(d2, 0.0, radius).sum())
            hid = np.arange(src.shape[0]) % 3 == 1
            x.set_hidden(hid)
            _check(x, y, case, _want(name, "source visible", ~hid, None), scope="visible", what="bounds twin visible " + name)
            x.set_hidden(None)
            x.register(y, radius, transform=M, max_iterations=2)
        for fn in (L.gsr_debug_bounds_match, L.gsr_debug_bounds_neighbours):
            buf = (ctypes.c_uint32 * 8)()
            assert fn(buf) == 0
            assert list(buf) == [0] * 8
    finally:
        x.dispose()
        y.dispose()

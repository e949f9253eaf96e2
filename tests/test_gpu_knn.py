"""k nearest neighbours on the GPU: gsr_knn and gsr_select_knn (k_knn.hip, gsr_knn.cpp) against tests/knn_reference.py, the
blocked O(n^2) specification in numpy f64, EXACTLY: found, idx, hist, every info field and the selection's words as integers, d2
and the values of both stats as their 64-bit patterns.  The shapes are knn_reference.families(): one and two splats, the wave and
workgroup edges, coincident splats (the tie rule, and the full list that rejects an equal distance with a larger index), lattices
with exact ties at the radius through negative coordinates, 2^19 radii out and beyond the cell clamp, non-finite rows, and 8192
splats of clusters with floaters whose lists stay short."""
import ctypes
import os

import numpy as np
import pytest

import attr_reference as ar
import knn_reference as kr
import neighbour_reference as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
W, H = 128, 96
GSR_ERR_ARG = -1
OPS = {"replace": 0, "add": 1, "subtract": 2, "intersect": 3}
FAMILIES = kr.families()
BY_NAME = {f[0]: f for f in FAMILIES}
CLUSTER = "clusters and floaters, k 8"
_LISTS = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _want(key, p, radius, k, mask=None):
    """the reference's (found, idx, d2) of positions in a scope at k: computed once per key at MAX_K -- the order is total, so the
    list at k is the first k slots of the list at MAX_K -- and left unchanged"""
    if key not in _LISTS:
        _LISTS[key] = kr.lists(p, radius, kr.MAX_K, mask)
        for a in _LISTS[key]:
            a.setflags(write=False)
    found, idx, d2 = _LISTS[key]
    return np.minimum(found, k).astype(np.uint32), idx[:, :k], d2[:, :k]


def _family_key(name):
    return name.rsplit(", k ", 1)[0]


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


def _check(r, p, radius, k, want, mask=None, scope=0, what=""):
    """every output of gsr_knn, with both stats, against the reference; returns {stat: values}"""
    n = np.asarray(p).reshape(-1, 3).shape[0]
    wf, wi, wd = want
    in_scope = n if mask is None else int(np.asarray(mask).sum())
    out = {}
    for stat in kr.STATS:
        found, idx, d2, values, hist, info = r.knn(radius, k=k, stat=stat, scope=_scope_names(scope), idx=True, d2=True)
        wv = kr.values(wf, wd, k, stat, mask)
        winfo = kr.info(p, wf, wv, k, mask)
        print(what, stat, {key: info[key] for key in ("in_scope", "nonfinite", "pair_bound", "complete", "finite_values", "value_min", "value_max")})
        assert found.dtype == np.uint32 and found.shape == (n,) and idx.shape == (n, k) and d2.shape == (n, k) and values.shape == (n,) and hist.shape == (k + 1,)
        assert np.array_equal(found, wf), (what, np.nonzero(found != wf)[0][:8])
        assert np.array_equal(idx, wi), (what, np.nonzero((idx != wi).any(axis=1))[0][:8])
        assert np.array_equal(_bits(d2), _bits(wd)), (what, np.nonzero((_bits(d2) != _bits(wd)).any(axis=1))[0][:8])
        assert np.array_equal(_bits(values), _bits(wv)), (what, stat, np.nonzero(_bits(values) != _bits(wv))[0][:8])
        assert np.array_equal(hist, kr.hist(wf, k, mask)) and int(hist.sum()) == in_scope, what
        for key, v in winfo.items():
            assert info[key] == v, (what, stat, key, info[key], v)
        assert _bits([info["value_min"], info["value_max"]]).tolist() == _bits([winfo["value_min"], winfo["value_max"]]).tolist()
        assert info["budget"] == kr.DEFAULT_BUDGET
        assert nr.pair_floor(p, radius, mask) <= info["pair_bound"] <= info["budget"], what
        # the lists are optional: without them the same found, values and hist
        f2, i2, d22, v2, h2, info2 = r.knn(radius, k=k, stat=stat, scope=_scope_names(scope))
        assert i2 is None and d22 is None and info2 == info
        assert np.array_equal(f2, wf) and np.array_equal(_bits(v2), _bits(wv)) and np.array_equal(h2, hist)
        out[stat] = wv
    return out


def _check_select(r, values, lo, hi, radius, k, stat, mask=None, scope=0, op="replace", prior=None, what=""):
    got, info = r.select_knn(radius, k=k, stat=stat, lo=lo, hi=hi, scope=_scope_names(scope), op=op)
    picked = kr.select(values, lo, np.inf if hi is None else hi, mask)
    after = picked if prior is None else ar.fold(prior, picked, OPS[op])
    assert got == int(after.sum()) == r.selection_count(), (what, got, int(after.sum()))
    assert np.array_equal(r.selection_words(), ar.pack(after)), what
    return after


def _ranges(v):
    """value ranges that cut a family's finite values in two, take the +inf ones in (hi=None) and leave them out (a finite hi)"""
    fin = np.sort(v[np.isfinite(v)])
    mid = float(fin[fin.size // 2]) if fin.size else 0.5
    top = float(fin[-1]) if fin.size else 1.0
    return ((0.0, None), (0.0, 1e300), (mid, None), (0.0, mid), (mid, top), (top, np.nextafter(top, np.inf)), (mid, mid), (np.inf, None), (np.inf, np.inf))


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_lists_values_histogram_info_and_selection_equal_the_reference(r, case):
    name, p, radius, k = case
    r.set_scene_arrays(*_arrays(p))
    want = _want(_family_key(name), p, radius, k)
    values = _check(r, p, radius, k, want, what=name)
    for stat, v in values.items():
        for lo, hi in _ranges(v):
            after = _check_select(r, v, lo, hi, radius, k, stat, what="%s %s [%r, %r)" % (name, stat, lo, hi))
            if lo == hi and np.isfinite(lo):
                assert not after.any()
    # a scope: every third splat hidden, the walk sees only the others
    n = p.shape[0]
    hid = np.arange(n) % 3 == 1
    r.set_hidden(hid)
    want_vis = _want(_family_key(name) + " visible", p, radius, k, ~hid)
    vis = _check(r, p, radius, k, want_vis, ~hid, 2, name + " visible")
    _check_select(r, vis["mean"], 0.0, None, radius, k, "mean", ~hid, 2, what=name + " visible")
    r.set_hidden(None)


def test_small_cases_by_hand(r):
    _, p, radius, k = BY_NAME["n = 1, k 3"]
    r.set_scene_arrays(*_arrays(p))
    found, idx, d2, values, hist, info = r.knn(radius, k=k, idx=True, d2=True)
    assert found.tolist() == [0] and (idx == kr.NONE).all() and np.isposinf(d2).all() and np.isposinf(values).all() and hist.tolist() == [1, 0, 0, 0]
    assert info["finite_values"] == 0 and info["value_min"] == np.inf and info["value_max"] == -np.inf
    _, p, radius, k = BY_NAME["n = 2 at exactly radius, k 3"]
    r.set_scene_arrays(*_arrays(p))
    found, idx, d2, values, hist, _ = r.knn(radius, k=k, idx=True, d2=True)
    assert found.tolist() == [1, 1] and idx.tolist() == [[1, kr.NONE, kr.NONE], [0, kr.NONE, kr.NONE]]
    assert d2[:, 0].tolist() == [radius * radius] * 2 and values.tolist() == [radius, radius] and hist.tolist() == [0, 2, 0, 0]
    _, p, radius, k = BY_NAME["n = 2 one ulp beyond, k 3"]
    r.set_scene_arrays(*_arrays(p))
    assert r.knn(radius, k=k)[0].tolist() == [0, 0]
    _, p, radius, k = BY_NAME["300 coincident, k 7"]
    r.set_scene_arrays(*_arrays(p))
    found, idx, d2, values, hist, info = r.knn(radius, k=k, stat="kth", idx=True, d2=True)
    assert (found == 7).all() and not d2.any() and not values.any() and hist.tolist() == [0] * 7 + [300] and info["complete"] == 300
    assert idx[0].tolist() == [1, 2, 3, 4, 5, 6, 7] and idx[3].tolist() == [0, 1, 2, 4, 5, 6, 7] and idx[299].tolist() == [0, 1, 2, 3, 4, 5, 6]
    out = r.knn(radius, k=3, found=False, values=False, hist=False)
    assert out[:5] == (None, None, None, None, None) and out[5]["in_scope"] == 300


def _cluster_scene(r):
    name, p, radius, k = BY_NAME[CLUSTER]
    r.set_scene_arrays(*_arrays(p))
    return name, p, radius, k


def test_short_lists_are_padded_and_infinite_values_follow_the_upper_end(r):
    name, p, radius, k = _cluster_scene(r)
    wf, wi, wd = _want(_family_key(name), p, radius, k)
    short = (wf > 0) & (wf < k)
    assert short.sum() > 10 and (wf == 0).sum() > 100                 # floaters with some neighbours, and with none
    found, idx, d2, values, _, info = r.knn(radius, k=k, stat="kth", idx=True, d2=True)
    t = np.arange(k)[None, :] >= found[:, None]
    assert (idx[t] == kr.NONE).all() and np.isposinf(d2[t]).all() and not (idx[~t] == kr.NONE).any() and np.isfinite(d2[~t]).all()
    assert np.isposinf(values[wf < k]).all() and info["finite_values"] == info["complete"] == int((wf == k).sum())
    assert r.select_knn(radius, k=k, stat="kth", lo=0.0, hi=None)[0] == p.shape[0]
    assert r.select_knn(radius, k=k, stat="kth", lo=0.0, hi=1e300)[0] == info["complete"]
    assert r.select_knn(radius, k=k, stat="kth", lo=np.inf, hi=None)[0] == p.shape[0] - info["complete"]


def test_every_scope_after_select_box_and_hide_selected(r):
    name, p, radius, k = _cluster_scene(r)
    n = p.shape[0]
    r.select_box((-1.0, 0.4, -1.0, 0.6, -1.0, 1.0))
    r.hide_selected()
    hid = ar.unpack(r.hidden_words(), n)
    assert 0 < hid.sum() < n
    r.select_box((-0.2, 30.0, -30.0, 30.0, -30.0, 30.0))
    sel = ar.unpack(r.selection_words(), n)
    assert 0 < (sel & hid).sum() < sel.sum() < n
    for scope in (1, 3):
        mask = ar.in_scope(n, scope, ar.pack(sel), ar.pack(hid))
        want = _want("%s scope %d" % (_family_key(name), scope), p, radius, k, mask)
        _check(r, p, radius, k, want, mask, scope, "%s scope %d" % (name, scope))
        assert np.array_equal(r.selection_words(), ar.pack(sel))       # gsr_knn reads the selection and leaves it
    r.set_hidden(None)


def test_select_with_every_op(r):
    name, p, radius, k = _cluster_scene(r)
    n = p.shape[0]
    wf, _, wd = _want(_family_key(name), p, radius, k)
    v = kr.values(wf, wd, k, "mean")
    cut = float(np.median(v[np.isfinite(v)]))
    prior = np.arange(n) % 7 < 3
    for op in OPS:
        r.set_selection(prior)
        _check_select(r, v, cut, None, radius, k, "mean", op=op, prior=prior, what=op)
    # in the selected scope the pick is made among the selected, with neighbours among the selected
    r.set_selection(prior)
    sf, _, sd = _want(_family_key(name) + " selected %7<3", p, radius, k, prior)
    _check_select(r, kr.values(sf, sd, k, "mean", prior), cut, None, radius, k, "mean", mask=prior, scope=1, op="intersect", prior=prior, what="selected scope")


def test_statistical_outliers_and_the_scene_that_is_left(r, gh):
    name, p, radius, k = _cluster_scene(r)
    wf, _, wd = _want(_family_key(name), p, radius, k)
    v = kr.values(wf, wd, k, "mean")
    selected, threshold, info = r.select_statistical_outliers(radius, k=k, std_ratio=2.0)
    assert threshold == kr.outlier_threshold(v, 2.0) == gh.knn_outlier_threshold(v, 2.0) and np.isfinite(threshold)
    outliers = v >= threshold                                          # exactly the values at or above the threshold it returns, +inf included
    assert selected == int(outliers.sum()) == r.selection_count() and np.array_equal(r.selection_words(), ar.pack(outliers))
    assert (wf == 0).sum() <= selected < p.shape[0] // 8 and info["in_scope"] == p.shape[0]
    # erase them; stateless: the same call now describes the compacted scene
    assert r.scene_erase_selected() == p.shape[0] - selected
    left = r.read_scene()[1].reshape(-1, 3)
    assert np.array_equal(left.view(np.uint32), p[~outliers].view(np.uint32))
    _check(r, left, radius, k, kr.lists(left, radius, k), what="after the erase")
    # fewer than two finite values: only the splats without a neighbour
    _, q, rad, _ = BY_NAME["n = 2 one ulp beyond, k 3"]
    r.set_scene_arrays(*_arrays(q))
    selected, threshold, _ = r.select_statistical_outliers(rad, k=3)
    assert threshold == np.inf and selected == 2


def test_two_members_of_a_shared_scene_agree(gh, r):
    name, p, radius, k = _cluster_scene(r)
    b = gh.HIPRenderer(W, H)
    try:
        b.share_scene(r)
        want = _want(_family_key(name), p, radius, k)
        values = None
        for m in (r, b):
            values = _check(m, p, radius, k, want, what="member")
        cut = float(np.median(values["mean"][np.isfinite(values["mean"])]))
        words = []
        for m in (r, b):
            _check_select(m, values["mean"], cut, None, radius, k, "mean", what="member")
            words.append(m.selection_words().copy())
        assert np.array_equal(words[0], words[1])
    finally:
        b.dispose()


def test_every_refusal_leaves_the_selection_alone(gh, r):
    _, p, radius, k = BY_NAME["n = 65, k 8"]
    r.set_scene_arrays(*_arrays(p))
    n = p.shape[0]
    prior = np.arange(n) % 3 == 0
    r.set_selection(prior)
    L, ctx = r._L, r._ctx
    found = np.zeros(n, np.uint32)
    info = gh.GsrKnnInfo()
    sel = ctypes.c_uint32(77)
    knn = lambda radius=radius, k=k, scope=0, budget=0, stat=1, m=n: L.gsr_knn(ctx, radius, k, scope, budget, stat, found.ctypes.data, None, None, None, m, None,
                                                                               ctypes.byref(info))
    pick = lambda radius=radius, k=k, scope=0, budget=0, stat=1, lo=0.0, hi=1.0, op=0: L.gsr_select_knn(ctx, radius, k, scope, budget, stat, lo, hi, op,
                                                                                                        ctypes.byref(sel), ctypes.byref(info))
    refused = [lambda v=v: knn(radius=v) for v in (0.0, -1.0, np.nan, np.inf, 1e-200, 1e200)]
    refused += [lambda v=v: pick(radius=v) for v in (0.0, np.nan, 1e-200, 1e200)]
    refused += [lambda: knn(k=0), lambda: knn(k=33), lambda: pick(k=0), lambda: pick(k=33)]
    refused += [lambda: knn(stat=2), lambda: knn(stat=-1), lambda: pick(stat=2), lambda: knn(scope=4), lambda: pick(scope=8), lambda: pick(op=4), lambda: pick(op=-1)]
    refused += [lambda: pick(lo=np.nan), lambda: pick(hi=np.nan), lambda: pick(lo=2.0, hi=1.0), lambda: pick(lo=np.inf, hi=1.0)]
    refused += [lambda: knn(m=n - 1), lambda: knn(m=n + 1)]
    refused += [lambda: knn(budget=kr.MAX_BUDGET + 1), lambda: pick(budget=kr.MAX_BUDGET + 1)]
    for t, call in enumerate(refused):
        assert call() == GSR_ERR_ARG, t
        assert L.gsr_last_error(ctx), t
        assert sel.value == 77 and not found.any(), t
        assert r.selection_count() == int(prior.sum()), t
    assert np.array_equal(r.selection_words(), ar.pack(prior))
    assert L.gsr_knn(None, radius, k, 0, 0, 1, None, None, None, None, 0, None, None) == GSR_ERR_ARG
    assert L.gsr_select_knn(None, radius, k, 0, 0, 1, 0.0, 1.0, 0, None, None) == GSR_ERR_ARG
    # and what is NOT refused: every pointer NULL, lo == hi, both bounds +inf
    assert L.gsr_knn(ctx, radius, k, 0, 0, 1, None, None, None, None, 0, None, None) == 0
    assert pick(lo=0.25, hi=0.25, op=1) == 0 and sel.value == int(prior.sum())
    assert pick(lo=np.inf, hi=np.inf, op=2) == 0
    for bad in (0, 33):
        with pytest.raises(ValueError):
            r.knn(radius, k=bad)
    with pytest.raises(ValueError):
        r.knn(radius, stat="median")


def test_a_budget_of_one_fills_info_and_launches_no_walk(gh, r):
    name, p, radius, k = _cluster_scene(r)
    n = p.shape[0]
    prior = np.arange(n) % 5 == 0
    r.set_selection(prior)
    for call in (lambda: r.knn(radius, k=k, budget=1), lambda: r.select_knn(radius, k=k, lo=0.0, budget=1)):
        with pytest.raises(gh.GsplatError) as ei:
            call()
        assert ei.value.code == GSR_ERR_ARG
        info = ei.value.info
        assert info["budget"] == 1 and info["in_scope"] == n and info["nonfinite"] == 0 and info["pair_bound"] >= nr.pair_floor(p, radius)
        assert info["complete"] == info["finite_values"] == 0 and info["value_min"] == np.inf and info["value_max"] == -np.inf   # no walk ran
        assert str(info["pair_bound"]) in str(ei.value) and "budget of 1" in str(ei.value)
        assert r.selection_count() == int(prior.sum()) and np.array_equal(r.selection_words(), ar.pack(prior))
    info = r.knn(radius, k=k)[5]
    assert r.knn(radius, k=k, budget=info["pair_bound"])[5]["budget"] == info["pair_bound"]      # at the bound: not above it


def test_an_empty_scene_and_an_empty_scope_return_zeros(gh, r):
    _, p, radius, k = BY_NAME["n = 64, k 8"]
    r.set_scene_arrays(*_arrays(p))
    r.set_selection(None)
    found, idx, d2, values, hist, info = r.knn(radius, k=k, scope="selected", idx=True, d2=True)
    assert not found.any() and (idx == kr.NONE).all() and np.isposinf(d2).all() and np.isnan(values).all() and not hist.any()
    assert info["in_scope"] == info["nonfinite"] == info["pair_bound"] == info["complete"] == info["finite_values"] == 0
    assert info["value_min"] == np.inf and info["value_max"] == -np.inf
    assert r.select_knn(radius, k=k, scope=("selected", "visible"))[0] == 0
    e = gh.HIPRenderer(W, H)                                           # (never given a scene: the empty one)
    try:
        found, _, _, values, hist, info = e.knn(radius, k=k)
        assert found.size == 0 and values.size == 0 and not hist.any() and info["in_scope"] == 0 and info["budget"] == kr.DEFAULT_BUDGET
        assert e.select_knn(radius, k=k)[0] == 0
    finally:
        e.dispose()


def _scratch(gh, x):
    fn = x._L.gsr_debug_knn_scratch
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    out = ctypes.c_uint64(1)
    assert fn(x._ctx, ctypes.byref(out)) == 0
    return out.value


def test_a_context_that_only_renders_allocates_nothing(gh):
    cfg = gh.synth.CONFIGS["C1"]
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows("C1"))
    cam = gh.orbit_camera(3, width=cfg["width"], height=cfg["height"], fx=cfg["fx"])
    x = gh.HIPRenderer(cfg["width"], cfg["height"])
    try:
        x.render(scene, cam)
        x.neighbours(0.05)
        assert _scratch(gh, x) == 0                                    # rendering and the other walks of the index hold none of it
        n, k = cfg["n"], 5
        x.knn(0.05, k=k)
        assert _scratch(gh, x) == 32 + 12 * n                          # the info words, found and values: no lists were asked for
        x.knn(0.05, k=k, d2=True)
        assert _scratch(gh, x) == 32 + 12 * n + 12 * n * k
        x.knn(0.05, k=2, idx=True)
        assert _scratch(gh, x) == 32 + 12 * n + 12 * n * k             # it only grows
    finally:
        x.dispose()


def test_bounds_twin_counts_nothing(gh):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    x = gh.HIPRenderer(W, H, lib_path=BOUNDS_LIB)
    try:
        for name in ("n = 1, k 3", "n = 65, k 8", "n = 257, k 1", "300 coincident, k 32", "lattice beyond the clamp, k 6", "non-finite rows, k 4",
                     "clusters and floaters, k 32"):
            _, p, radius, k = BY_NAME[name]
            x.set_scene_arrays(*_arrays(p))
            values = _check(x, p, radius, k, _want(_family_key(name), p, radius, k), what="bounds twin " + name)
            after = _check_select(x, values["mean"], 0.0, 1e300, radius, k, "mean", what="bounds twin " + name)
            if 0 < after.sum():
                _check(x, p, radius, k, kr.lists(p, radius, k, after), after, 1, "bounds twin selected " + name)
        buf = (ctypes.c_uint32 * 8)()
        assert L.gsr_debug_bounds_knn(buf) == 0
        assert list(buf) == [0] * 8
    finally:
        x.dispose()

"""Normals on the GPU: gsr_normals and gsr_select_normal (k_normals.hip, gsr_normals.cpp) against tests/normal_reference.py, the
specification in numpy f64, EXACTLY: found and every info integer as integers, the normals as their 32-bit patterns, the variation
and its min / max as their 64-bit patterns, the selection's words as words.  The shapes are normal_reference.families(): the k-NN
families with k >= 2 -- one and two splats, the wave and workgroup edges, coincident splats, lattices with ties at the radius and
beyond the cell clamp, non-finite rows, 8192 splats of clusters with floaters at k 2, 8 and 32 -- a plane lattice and a sphere."""
import ctypes
import os

import numpy as np
import pytest

import attr_reference as ar
import knn_reference as kr
import neighbour_reference as nr
import normal_reference as nm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
W, H = 128, 96
GSR_ERR_ARG = -1
OPS = {"replace": 0, "add": 1, "subtract": 2, "intersect": 3}
FAMILIES = nm.families()
BY_NAME = {f[0]: f for f in FAMILIES}
CLUSTER = "clusters and floaters, k 8"
TOWARD = (0.3, -2.0, 0.7)
UP = (0.1, 1.0, -0.2)
_LISTS = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _lists(key, p, radius, k, mask=None):
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
    if n > 6:                                                          # rows the OWN source refuses a normal, and a tie in |s|
        rot[1] = 0.0
        rot[2, 3] = np.nan
        scl[3] = 0.0
        scl[4, 0] = np.inf
        scl[5] = [0.05, -0.02, 0.02]
    return data.reshape(-1), p.reshape(-1), rot.reshape(-1), scl.reshape(-1)


def _scope_names(scope):
    return tuple(name for name, bit in (("selected", 1), ("visible", 2)) if scope & bit)


def _same(got, want, p, mask, budget_floor, what):
    """one call's four outputs against the reference's three"""
    normals, variation, found, info = got
    wn, wv, wf = want
    n = wf.size
    assert normals.dtype == np.float32 and normals.shape == (n, 3) and variation.shape == (n,) and found.dtype == np.uint32 and found.shape == (n,)
    assert np.array_equal(found, wf), (what, np.nonzero(found != wf)[0][:8])
    assert np.array_equal(_bits32(normals), _bits32(wn)), (what, np.nonzero((_bits32(normals) != _bits32(wn)).any(axis=1))[0][:8])
    assert np.array_equal(_bits(variation), _bits(wv)), (what, np.nonzero(_bits(variation) != _bits(wv))[0][:8])
    winfo = nm.info(p, wv, mask)
    print(what, info)
    for key, v in winfo.items():
        assert info[key] == v, (what, key, info[key], v)
    assert _bits([info["variation_min"], info["variation_max"]]).tolist() == _bits([winfo["variation_min"], winfo["variation_max"]]).tolist()
    assert info["budget"] == nm.DEFAULT_BUDGET
    if budget_floor is None:
        assert info["pair_bound"] == 0, what
    else:
        assert budget_floor <= info["pair_bound"] <= info["budget"], what


def _check_knn(r, p, radius, k, lists, mask=None, scope=0, what=""):
    """gsr_normals' KNN source with and without a viewpoint; returns the unoriented reference outputs"""
    floor = nr.pair_floor(p, radius, mask)
    out = None
    for toward in (None, TOWARD):
        want = nm.knn_normals(p, radius, k, mask, toward, lists)
        _same(r.normals(radius, k=k, toward=toward, scope=_scope_names(scope)), want, p, mask, floor, "%s toward %r" % (what, toward))
        out = out or want
    return out


def _check_own(r, arrays, mask=None, scope=0, what=""):
    _, p, rot, scl = arrays
    out = None
    for toward in (None, TOWARD):
        want = nm.own_normals(p, rot, scl, mask, toward)
        _same(r.normals(source="own", toward=toward, scope=_scope_names(scope)), want, p, mask, None, "%s own toward %r" % (what, toward))
        out = out or want
    return out


def _check_select(r, want, stat, lo, hi, axis=None, op="replace", prior=None, what="", **options):
    got, info = r.select_normal(stat, lo=lo, hi=hi, axis=axis, op=op, **options)
    picked = nm.select(want[0], want[1], stat, lo, hi, axis)
    after = picked if prior is None else ar.fold(prior, picked, OPS[op])
    assert got == int(after.sum()) == r.selection_count(), (what, got, int(after.sum()))
    assert np.array_equal(r.selection_words(), ar.pack(after)), what
    return after


def _ranges(want, stat, axis):
    """closed ranges that cut the values in two, sit exactly on a value at both ends, and run to infinity"""
    v = nm.values(want[0], want[1], stat, axis)
    fin = np.sort(v[~np.isnan(v)])
    mid = float(fin[fin.size // 2]) if fin.size else 0.25
    low = float(fin[0]) if fin.size else 0.0
    return ((-np.inf, np.inf), (mid, np.inf), (-np.inf, mid), (mid, mid), (low, mid), (np.nextafter(mid, np.inf), np.inf))


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_normals_variation_found_info_and_selection_equal_the_reference(r, case):
    name, p, radius, k = case
    arrays = _arrays(p)
    r.set_scene_arrays(*arrays)
    n = p.shape[0]
    lists = _lists(_family_key(name), p, radius, k)
    want = _check_knn(r, p, radius, k, lists, what=name)
    own = _check_own(r, arrays, what=name)
    # the consistency guarantee: the picker is the rule on gsr_normals' own outputs
    for stat, axis in (("dot", UP), ("abs_dot", UP), ("variation", None)):
        for lo, hi in _ranges(want, stat, axis):
            after = _check_select(r, want, stat, lo, hi, axis, radius=radius, k=k, what="%s %s [%r, %r]" % (name, stat, lo, hi))
            if lo == -np.inf and hi == np.inf:
                assert int(after.sum()) == int((~np.isnan(want[1])).sum())               # every valid row and no other
    _check_select(r, own, "abs_dot", 0.0, 0.5, UP, source="own", what=name + " own")
    _check_select(r, own, "variation", 0.0, 0.1, source="own", what=name + " own")
    got = r.normals(radius, k=k)
    picked = nm.select(got[0], got[1], "dot", 0.0, np.inf, UP)                         # .. applied to what the device itself returned
    assert r.select_normal("dot", lo=0.0, axis=UP, radius=radius, k=k)[0] == int(picked.sum()) and np.array_equal(r.selection_words(), ar.pack(picked))
    # a scope: every third splat hidden, the walk sees only the others
    hid = np.arange(n) % 3 == 1
    r.set_hidden(hid)
    vis = _check_knn(r, p, radius, k, _lists(_family_key(name) + " visible", p, radius, k, ~hid), ~hid, 2, name + " visible")
    _check_select(r, vis, "variation", 0.0, np.inf, scope=("visible",), radius=radius, k=k, what=name + " visible")
    _check_own(r, arrays, ~hid, 2, name + " visible")
    r.set_hidden(None)


def test_small_cases_by_hand(r):
    p, radius, k = nm.plane_lattice()
    r.set_scene_arrays(*_arrays(p))
    normals, variation, found, info = r.normals(radius, k=k)
    assert np.array_equal(normals, np.tile(np.float32([0, 0, 1]), (25, 1))) and np.array_equal(_bits(variation), _bits(np.zeros(25)))
    assert found.reshape(5, 5)[0, 0] == 2 and found.reshape(5, 5)[2, 2] == 4 and info["valid"] == 25 and info["variation_max"] == 0.0
    assert r.normals(radius, k=k, toward=(0.5, 0.5, -3.0))[0][:, 2].tolist() == [-1.0] * 25
    g = (-1.0, 0.0, 1.0)
    cube = np.array([[x, y, z] for z in g for y in g for x in g], dtype=np.float32)
    r.set_scene_arrays(*_arrays(cube))
    normals, variation, found, _ = r.normals(1.0, k=6)
    assert found[13] == 6 and normals[13].tolist() == [1.0, 0.0, 0.0] and variation[13] == 0.3333333333333333
    r.set_scene_arrays(*_arrays(np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0]])))
    normals, variation, found, _ = r.normals(5.0, k=4)
    assert found.tolist() == [2, 2, 2] and np.array_equal(normals, np.tile(np.float32([0, 1, 0]), (3, 1))) and not variation.any()
    r.set_scene_arrays(*_arrays(np.float32([[0.5, 0.25, 2.0]] * 3)))
    normals, variation, found, info = r.normals(1.0, k=4)
    assert found.tolist() == [2, 2, 2] and (_bits32(normals) == 0x7fc00000).all() and (_bits(variation) == 0x7ff8000000000000).all() and info["valid"] == 0
    assert info["variation_min"] == np.inf and info["variation_max"] == -np.inf
    r.set_scene_arrays(*_arrays(np.float32([[0, 0, 0], [0.5, 0, 0], [9, 9, 9]])))
    normals, variation, found, info = r.normals(1.0, k=4)
    assert found.tolist() == [1, 1, 0] and np.isnan(normals).all() and np.isnan(variation).all() and info["valid"] == 0
    out = r.normals(1.0, k=4, normals=False, variation=False, found=False)
    assert out[:3] == (None, None, None) and out[3]["in_scope"] == 3


def _cluster_scene(r):
    name, p, radius, k = BY_NAME[CLUSTER]
    arrays = _arrays(p)
    r.set_scene_arrays(*arrays)
    return name, p, radius, k, arrays


def test_every_scope_after_select_box_and_hide_selected(r):
    name, p, radius, k, arrays = _cluster_scene(r)
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
        lists = _lists("%s scope %d" % (_family_key(name), scope), p, radius, k, mask)
        _check_knn(r, p, radius, k, lists, mask, scope, "%s scope %d" % (name, scope))
        _check_own(r, arrays, mask, scope, "%s scope %d" % (name, scope))
        assert np.array_equal(r.selection_words(), ar.pack(sel))       # gsr_normals reads the selection and leaves it
    r.set_hidden(None)


def test_every_stat_with_every_op_over_a_prior_selection(r):
    name, p, radius, k, arrays = _cluster_scene(r)
    n = p.shape[0]
    want = nm.knn_normals(p, radius, k, None, TOWARD, _lists(_family_key(name), p, radius, k))
    prior = np.arange(n) % 7 < 3
    for stat, axis, lo, hi in (("dot", UP, 0.2, np.inf), ("abs_dot", UP, 0.0, 0.3), ("variation", None, 0.05, 1.0)):
        for op in OPS:
            r.set_selection(prior)
            after = _check_select(r, want, stat, lo, hi, axis, op=op, prior=prior, radius=radius, k=k, toward=TOWARD, what="%s %s" % (stat, op))
            assert 0 < after.sum() < n
    # in the selected scope the pick is made among the selected, with neighbours among the selected
    r.set_selection(prior)
    sel_want = nm.knn_normals(p, radius, k, prior, None, _lists(_family_key(name) + " selected %7<3", p, radius, k, prior))
    _check_select(r, sel_want, "variation", 0.0, 0.1, op="intersect", prior=prior, radius=radius, k=k, scope=("selected",), what="selected scope")
    own = nm.own_normals(arrays[1], arrays[2], arrays[3])
    for op in OPS:
        r.set_selection(prior)
        _check_select(r, own, "abs_dot", 0.0, 0.4, UP, op=op, prior=prior, source="own", what="own " + op)


def test_two_members_of_a_shared_scene_agree(gh, r):
    name, p, radius, k, arrays = _cluster_scene(r)
    b = gh.HIPRenderer(W, H)
    try:
        b.share_scene(r)
        lists = _lists(_family_key(name), p, radius, k)
        words = []
        for m in (r, b):
            want = _check_knn(m, p, radius, k, lists, what="member")
            _check_own(m, arrays, what="member")
            _check_select(m, want, "abs_dot", 0.0, 0.25, UP, radius=radius, k=k, what="member")
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
    info = gh.GsrNormalInfo()
    sel = ctypes.c_uint32(77)
    up = np.float64([0.0, 1.0, 0.0])

    def options(source=0, k=k, radius=radius, scope=0, oriented=0, budget=0, toward=(0.0, 0.0, 0.0)):
        o = gh.GsrNormalOptions()
        o.source, o.k, o.radius, o.scope, o.oriented, o.budget = source, k, radius, scope, oriented, budget
        o.toward[:] = toward
        return o

    def normals(m=n, **kw):
        return L.gsr_normals(ctx, ctypes.byref(options(**kw)), None, None, found.ctypes.data, m, ctypes.byref(info))

    def pick(stat=1, axis=up, lo=0.0, hi=1.0, op=0, **kw):
        a = None if axis is None else np.ascontiguousarray(axis, dtype=np.float64)      # (alive until the call returns)
        return L.gsr_select_normal(ctx, ctypes.byref(options(**kw)), stat, None if a is None else a.ctypes.data, lo, hi, op, ctypes.byref(sel), ctypes.byref(info))

    refused = [lambda v=v, f=f: f(radius=v) for v in (0.0, -1.0, np.nan, np.inf, 1e-200, 1e200) for f in (normals, pick)]
    refused += [lambda v=v, f=f: f(k=v) for v in (0, 1, 33) for f in (normals, pick)]
    refused += [lambda v=v, f=f: f(source=v) for v in (2, -1) for f in (normals, pick)]
    refused += [lambda v=v, f=f, s=s: f(scope=v, source=s) for v in (4, 8) for f in (normals, pick) for s in (0, 1)]
    refused += [lambda v=v, f=f, s=s: f(oriented=1, toward=v, source=s) for v in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)) for f in (normals, pick) for s in (0, 1)]
    refused += [lambda: pick(stat=3), lambda: pick(stat=-1), lambda: pick(op=4), lambda: pick(op=-1)]
    refused += [lambda: pick(axis=None), lambda: pick(stat=0, axis=None), lambda: pick(axis=(0.0, 0.0, 0.0)), lambda: pick(axis=(0.0, np.nan, 1.0)),
                lambda: pick(stat=0, axis=(np.inf, 0.0, 1.0))]
    refused += [lambda: pick(lo=np.nan), lambda: pick(hi=np.nan), lambda: pick(lo=2.0, hi=1.0), lambda: pick(lo=np.inf, hi=1.0)]
    refused += [lambda: normals(m=n - 1), lambda: normals(m=n + 1), lambda: normals(m=n + 1, source=1)]
    refused += [lambda f=f, s=s: f(budget=nm.MAX_BUDGET + 1, source=s) for f in (normals, pick) for s in (0, 1)]
    for t, call in enumerate(refused):
        assert call() == GSR_ERR_ARG, t
        assert L.gsr_last_error(ctx), t
        assert sel.value == 77 and not found.any(), t
        assert r.selection_count() == int(prior.sum()), t
    assert np.array_equal(r.selection_words(), ar.pack(prior))
    assert L.gsr_normals(None, ctypes.byref(options()), None, None, None, 0, None) == GSR_ERR_ARG
    assert L.gsr_normals(ctx, None, None, None, None, 0, None) == GSR_ERR_ARG
    assert L.gsr_select_normal(None, ctypes.byref(options()), 2, None, 0.0, 1.0, 0, None, None) == GSR_ERR_ARG
    assert L.gsr_select_normal(ctx, None, 2, None, 0.0, 1.0, 0, None, None) == GSR_ERR_ARG
    assert np.array_equal(r.selection_words(), ar.pack(prior))
    # and what is NOT refused: every pointer NULL, lo == hi, infinite ends, a non-finite toward that is not read, OWN with any k and radius
    assert L.gsr_normals(ctx, ctypes.byref(options()), None, None, None, 0, None) == 0
    assert normals(toward=(np.nan, 0.0, 0.0)) == 0 and found.any()
    assert normals(source=1, k=0, radius=-1.0) == 0 and not found.any()
    assert pick(stat=2, axis=None, lo=0.25, hi=0.25, op=1) == 0 and sel.value >= int(prior.sum())
    assert pick(lo=-np.inf, hi=np.inf, op=3) == 0
    for bad in (0, 1, 33):
        with pytest.raises(ValueError):
            r.normals(radius, k=bad)
    with pytest.raises(ValueError):
        r.normals(radius, source="pca")
    with pytest.raises(ValueError):
        r.select_normal("median", radius=radius)
    with pytest.raises(ValueError):
        r.select_normal("dot", radius=radius)


def test_a_budget_of_one_fills_info_and_launches_no_walk(gh, r):
    name, p, radius, k, _ = _cluster_scene(r)
    n = p.shape[0]
    prior = np.arange(n) % 5 == 0
    r.set_selection(prior)
    for call in (lambda: r.normals(radius, k=k, budget=1), lambda: r.select_normal("variation", radius=radius, k=k, budget=1)):
        with pytest.raises(gh.GsplatError) as ei:
            call()
        assert ei.value.code == GSR_ERR_ARG
        info = ei.value.info
        assert info["budget"] == 1 and info["in_scope"] == n and info["nonfinite"] == 0 and info["pair_bound"] >= nr.pair_floor(p, radius)
        assert info["valid"] == 0 and info["variation_min"] == np.inf and info["variation_max"] == -np.inf   # no walk ran
        assert str(info["pair_bound"]) in str(ei.value) and "budget of 1" in str(ei.value)
        assert r.selection_count() == int(prior.sum()) and np.array_equal(r.selection_words(), ar.pack(prior))
    info = r.normals(radius, k=k)[3]
    assert r.normals(radius, k=k, budget=info["pair_bound"])[3]["budget"] == info["pair_bound"]      # at the bound: not above it
    assert r.normals(source="own", budget=1)[3]["pair_bound"] == 0                                   # OWN walks nothing: any budget does


def test_an_empty_scene_and_an_empty_scope_return_zeros(gh, r):
    _, p, radius, k = BY_NAME["n = 64, k 8"]
    r.set_scene_arrays(*_arrays(p))
    r.set_selection(None)
    for options in ({"radius": radius, "k": k}, {"source": "own"}):
        normals, variation, found, info = r.normals(scope="selected", **options)
        assert (_bits32(normals) == 0x7fc00000).all() and (_bits(variation) == 0x7ff8000000000000).all() and not found.any()
        assert info["in_scope"] == info["nonfinite"] == info["pair_bound"] == info["valid"] == 0
        assert info["variation_min"] == np.inf and info["variation_max"] == -np.inf
        assert r.select_normal("variation", scope=("selected", "visible"), **options)[0] == 0
    e = gh.HIPRenderer(W, H)                                           # (never given a scene: the empty one)
    try:
        for options in ({"radius": radius, "k": k}, {"source": "own"}):
            normals, variation, found, info = e.normals(**options)
            assert normals.shape == (0, 3) and variation.size == 0 and found.size == 0 and info["in_scope"] == 0 and info["budget"] == nm.DEFAULT_BUDGET
            assert info["variation_min"] == np.inf and info["variation_max"] == -np.inf
            assert e.select_normal("abs_dot", axis=UP, **options)[0] == 0
    finally:
        e.dispose()


def _scratch(x, name="gsr_debug_normals_scratch"):
    fn = getattr(x._L, name)
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    out = ctypes.c_uint64(1)
    assert fn(x._ctx, ctypes.byref(out)) == 0
    return out.value


def test_frame_pick_and_selection_are_untouched_and_a_context_that_never_calls_allocates_nothing(gh):
    cfg = gh.synth.CONFIGS["C1"]
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows("C1"))
    cam = gh.orbit_camera(3, width=cfg["width"], height=cfg["height"], fx=cfg["fx"])
    x = gh.HIPRenderer(cfg["width"], cfg["height"])
    try:
        n = cfg["n"]
        x.render(scene, cam)
        frame, order = x.readPixelsFloat().copy(), x.lastDepthIndex().copy()
        spot = [(cfg["width"] // 2, cfg["height"] // 2)]
        picked = x.pick(spot).copy()
        sel = np.arange(n) % 5 == 0
        x.set_selection(sel)
        x.neighbours(0.05)
        x.knn(0.05, k=5)
        assert _scratch(x) == 0                                        # rendering and the other walks of the index hold none of it
        first = x.normals(0.05, k=8, toward=(0.0, 0.0, 0.0))
        assert first[3]["in_scope"] == n and 0 < first[3]["valid"] <= n
        assert _scratch(x) == 32 + 24 * n
        with pytest.raises(gh.GsplatError) as ei:                      # a scene without rotations and scales has no axis of its own
            x.normals(source="own")
        assert ei.value.code == GSR_ERR_ARG and "gsr_set_scene_rows" in str(ei.value)
        x.normals(0.05, k=2)
        assert _scratch(x) == 32 + 24 * n                              # it only grows
        assert np.array_equal(x.selection_words(), ar.pack(sel)) and x.selection_count() == int(sel.sum())
        assert np.array_equal(x.pick(spot), picked)                    # the last frame is still valid: a pick needs it
        assert np.array_equal(x.readPixelsFloat().view(np.uint32), frame.view(np.uint32))
        again = x.normals(0.05, k=8, toward=(0.0, 0.0, 0.0))           # stateless: the same bits
        assert np.array_equal(_bits32(again[0]), _bits32(first[0])) and np.array_equal(_bits(again[1]), _bits(first[1])) and again[3] == first[3]
        x.render(scene, cam)
        assert np.array_equal(frame.view(np.uint32), x.readPixelsFloat().view(np.uint32)) and np.array_equal(order, x.lastDepthIndex())
    finally:
        x.dispose()


def test_bounds_twin_counts_nothing(gh):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    x = gh.HIPRenderer(W, H, lib_path=BOUNDS_LIB)
    try:
        for name in ("n = 1, k 3", "n = 65, k 8", "n = 257, k 8", "300 coincident, k 32", "lattice beyond the clamp, k 6", "non-finite rows, k 4",
                     "clusters and floaters, k 2", "clusters and floaters, k 32", "plane lattice, k 8"):
            _, p, radius, k = BY_NAME[name]
            arrays = _arrays(p)
            x.set_scene_arrays(*arrays)
            want = _check_knn(x, p, radius, k, _lists(_family_key(name), p, radius, k), what="bounds twin " + name)
            _check_own(x, arrays, what="bounds twin " + name)
            after = _check_select(x, want, "variation", 0.0, np.inf, radius=radius, k=k, what="bounds twin " + name)
            if 0 < after.sum():
                _check_knn(x, p, radius, k, kr.lists(p, radius, k, after), after, 1, "bounds twin selected " + name)
        buf = (ctypes.c_uint32 * 8)()
        assert L.gsr_debug_bounds_normals(buf) == 0
        assert list(buf) == [0] * 8
    finally:
        x.dispose()

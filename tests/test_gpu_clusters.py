"""Clusters on the GPU: gsr_clusters, gsr_select_clusters and gsr_select_cluster_at (k_clusters.hip, gsr_clusters.cpp) against
tests/cluster_reference.py, the blocked O(n^2) specification with a host union-find, EXACTLY: labels, sizes, info and the
selection's words bit for bit.  The shapes are cluster_reference.shapes() -- neighbour_reference.families(), a chain of 4096 splats
spaced exactly the radius apart in index order and permuted (deep trees, long hook retries), and 64 coincident groups of 65 -- at
min_pts 0, 1, 3 and 6."""
import ctypes
import os

import numpy as np
import pytest

import attr_reference as ar
import cluster_reference as cr
import neighbour_reference as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
W, H = 128, 96
GSR_ERR_ARG = -1
OPS = {"replace": 0, "add": 1, "subtract": 2, "intersect": 3}
SHAPES = cr.shapes()
BY_NAME = {s[0]: s for s in SHAPES}
NONE = cr.NONE
TOP = 2 ** 32 - 1
INFO_KEYS = ("in_scope", "nonfinite", "core", "border", "noise", "clusters", "largest_label", "largest_size")
_PAIRS, _WANT = {}, {}


def _want(name, min_pts, scope_key=None, mask=None):
    """the reference's clusters of a shape in a scope, computed once; the near pairs of the scope are shared by every min_pts"""
    key = (name, scope_key)
    _, p, radius = BY_NAME[name]
    if key not in _PAIRS:
        _PAIRS[key] = cr.pairs(p, radius, mask)
    if key + (min_pts,) not in _WANT:
        _WANT[key + (min_pts,)] = cr.Clusters(p, radius, min_pts, mask, _PAIRS[key])
    return _WANT[key + (min_pts,)]


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


def _check(r, p, radius, min_pts, want, mask=None, scope=0, what=""):
    """labels, sizes and info of one call against the reference; returns info"""
    n = np.asarray(p).reshape(-1, 3).shape[0]
    labels, sizes, info = r.clusters(radius, min_pts=min_pts, scope=_scope_names(scope))
    print(what, {k: info[k] for k in INFO_KEYS}, "pair_bound", info["pair_bound"])
    assert labels.dtype == np.uint32 and labels.shape == (n,) and sizes.dtype == np.uint32 and sizes.shape == (n,)
    assert np.array_equal(labels, want.labels), (what, np.nonzero(labels != want.labels)[0][:8])
    assert np.array_equal(sizes, want.sizes), (what, np.nonzero(sizes != want.sizes)[0][:8])
    assert {k: info[k] for k in INFO_KEYS} == want.info, what
    assert info["in_scope"] == info["core"] + info["border"] + info["noise"]
    assert info["budget"] == nr.DEFAULT_BUDGET
    assert nr.pair_floor(p, radius, mask) <= info["pair_bound"] <= info["budget"], what
    return info


def _check_select(r, want, lo, hi, radius, min_pts, mask=None, scope=0, op="replace", prior=None, what=""):
    got, _ = r.select_clusters(radius, lo=lo, hi=hi, min_pts=min_pts, scope=_scope_names(scope), op=op)
    picked = cr.select(want.sizes, lo, hi, mask)
    after = picked if prior is None else ar.fold(prior, picked, OPS[op])
    assert got == int(after.sum()) == r.selection_count(), (what, got, int(after.sum()))
    assert np.array_equal(r.selection_words(), ar.pack(after)), what
    return after


def _check_at(r, want, seed, radius, min_pts, scope=0, op="replace", prior=None, what=""):
    got, _ = r.select_cluster_at(radius, "largest" if seed == cr.LARGEST else int(seed), min_pts=min_pts, scope=_scope_names(scope), op=op)
    picked = cr.select_at(want.labels, seed, want.info["largest_label"])
    after = picked if prior is None else ar.fold(prior, picked, OPS[op])
    assert got == int(after.sum()) == r.selection_count(), (what, seed, got, int(after.sum()))
    assert np.array_equal(r.selection_words(), ar.pack(after)), (what, seed)
    return picked


def _seeds(want, mask=None):
    """one seed of every kind the shape has: core, border, noise, out of scope"""
    n = want.labels.size
    s = nr._scope(mask, n)
    kinds = (("core", want.core), ("border", want.border), ("noise", s & (want.labels == NONE)), ("out of scope", ~s))
    return [(kind, int(np.nonzero(m)[0][-1])) for kind, m in kinds if m.any()]


@pytest.mark.parametrize("min_pts", cr.MIN_PTS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_labels_sizes_info_and_selections_equal_the_reference(r, shape, min_pts):
    name, p, radius = shape
    n = p.shape[0]
    r.set_scene_arrays(*_arrays(p))
    want = _want(name, min_pts)
    _check(r, p, radius, min_pts, want, what=name)
    k = 4
    for lo, hi in ((0, 1), (0, k), (k, TOP), (2, 2)):
        after = _check_select(r, want, lo, hi, radius, min_pts, what="%s [%d, %d)" % (name, lo, hi))
        assert int(after.sum()) == int(((want.sizes >= lo) & (want.sizes.astype(np.int64) < hi)).sum())     # the consistency guarantee
    for kind, seed in _seeds(want) + [("largest", cr.LARGEST)]:
        picked = _check_at(r, want, seed, radius, min_pts, what="%s %s seed" % (name, kind))
        if kind in ("core", "border"):
            assert picked[seed] and int(picked.sum()) == int(want.sizes[seed])
        elif kind == "noise":
            assert not picked.any()
        else:
            assert int(picked.sum()) == want.info["largest_size"]
    # the scopes: every third splat hidden; then the splats the last pick left selected
    hid = np.arange(n) % 3 == 1
    r.set_hidden(hid)
    want_vis = _want(name, min_pts, "visible", ~hid)
    _check(r, p, radius, min_pts, want_vis, ~hid, 2, name + " visible")
    _check_select(r, want_vis, 0, k, radius, min_pts, mask=~hid, scope=2, what=name + " visible [0, k)")
    for kind, seed in _seeds(want_vis, ~hid) + [("largest", cr.LARGEST)]:
        picked = _check_at(r, want_vis, seed, radius, min_pts, scope=2, what="%s visible %s seed" % (name, kind))
        assert kind not in ("noise", "out of scope") or not picked.any()
    r.set_hidden(None)
    sel = np.arange(n) % 4 != 2
    r.set_selection(sel)
    want_sel = _want(name, min_pts, "selected %4!=2", sel)
    _check(r, p, radius, min_pts, want_sel, sel, 1, name + " selected")
    assert np.array_equal(r.selection_words(), ar.pack(sel))              # gsr_clusters reads the selection and leaves it
    _check_select(r, want_sel, 1, TOP, radius, min_pts, mask=sel, scope=1, op="intersect", prior=sel, what=name + " selected")


def test_small_cases_by_hand(r):
    _, p, radius = BY_NAME["n = 2 at exactly radius"]
    r.set_scene_arrays(*_arrays(p))
    for min_pts in (0, 1):
        labels, sizes, info = r.clusters(radius, min_pts=min_pts)
        assert labels.tolist() == [0, 0] and sizes.tolist() == [2, 2] and info["clusters"] == 1
    _, p, radius = BY_NAME["n = 2 one ulp beyond"]
    r.set_scene_arrays(*_arrays(p))
    labels, sizes, info = r.clusters(radius)
    assert labels.tolist() == [0, 1] and sizes.tolist() == [1, 1] and info["clusters"] == 2 and info["largest_label"] == 0
    labels, sizes, info = r.clusters(radius, min_pts=1)
    assert labels.tolist() == [NONE, NONE] and sizes.tolist() == [0, 0] and info["noise"] == 2 and info["largest_label"] == NONE
    # a non-core bridge does not merge two groups, and takes the smaller label of the two
    x = np.array([1.25, 2.2, 2.3, 2.4, 2.5, 0.0, 0.1, 0.2, 0.3])
    p = np.stack([x, np.zeros(9), np.zeros(9)], axis=1).astype(np.float32)
    r.set_scene_arrays(*_arrays(p))
    labels, sizes, info = r.clusters(1.0, min_pts=3)
    assert labels.tolist() == [1, 1, 1, 1, 1, 5, 5, 5, 5] and sizes.tolist() == [5] * 5 + [4] * 4
    assert (info["core"], info["border"], info["noise"], info["clusters"], info["largest_label"], info["largest_size"]) == (8, 1, 0, 2, 1, 5)
    assert r.clusters(1.0, min_pts=2)[0].tolist() == [0] * 9
    # ties for the largest go to the smallest label
    x = np.array([0.0, 0.1, 10.0, 20.0, 10.1, 20.1, 10.2, 20.2])
    p = np.stack([x, np.zeros(8), np.zeros(8)], axis=1).astype(np.float32)
    r.set_scene_arrays(*_arrays(p))
    labels, sizes, info = r.clusters(0.5)
    assert labels.tolist() == [0, 0, 2, 3, 2, 3, 2, 3] and sizes.tolist() == [2, 2, 3, 3, 3, 3, 3, 3]
    assert info["largest_label"] == 2 and info["largest_size"] == 3
    assert r.select_cluster_at(0.5, "largest")[0] == 3 and ar.unpack(r.selection_words(), 8).tolist() == [False, False, True, False, True, False, True, False]
    labels, sizes, info = r.clusters(0.5, labels=False, sizes=False)
    assert labels is None and sizes is None and info["clusters"] == 3


def _cluster_scene(r):
    name, p, radius = BY_NAME["clusters and floaters"]
    r.set_scene_arrays(*_arrays(p))
    return name, p, radius


def test_every_op_against_a_prior_selection(r):
    name, p, radius = _cluster_scene(r)
    n = p.shape[0]
    want = _want(name, 3)
    prior = np.arange(n) % 7 < 3
    seed = int(np.nonzero(want.core)[0][5])
    for op in OPS:
        r.set_selection(prior)
        _check_select(r, want, 0, 50, radius, 3, op=op, prior=prior, what=op)
        r.set_selection(prior)
        _check_at(r, want, seed, radius, 3, op=op, prior=prior, what=op)
        r.set_selection(prior)
        _check_at(r, want, cr.LARGEST, radius, 3, op=op, prior=prior, what=op + " largest")


def test_small_islands_erased_and_the_largest_kept(r):
    name, p, radius = _cluster_scene(r)
    want = _want(name, 0)
    small = cr.select(want.sizes, 0, 20)
    assert 200 <= small.sum() < p.shape[0] // 4                        # the floaters, one island each, and a few loose splats
    got, _ = r.select_clusters(radius, hi=20)
    assert got == int(small.sum())
    assert r.scene_erase_selected() == p.shape[0] - got
    left = r.read_scene()[1].reshape(-1, 3)
    assert np.array_equal(left.view(np.uint32), p[~small].view(np.uint32))
    # stateless: the same call now describes the scene that is left; keep its largest island
    want_left = cr.Clusters(left, radius, 0)
    _check(r, left, radius, 0, want_left, what="after the erase")
    assert want_left.info["largest_size"] >= 20 and int(want_left.sizes.min()) >= 20
    r.select_cluster_at(radius, "largest")
    r.invert_selection()
    assert r.scene_erase_selected() == want_left.info["largest_size"]
    kept = r.read_scene()[1].reshape(-1, 3)
    assert np.array_equal(kept.view(np.uint32), left[want_left.labels == want_left.info["largest_label"]].view(np.uint32))


def test_two_members_of_a_shared_scene_give_the_same_words(gh, r):
    name, p, radius = _cluster_scene(r)
    b = gh.HIPRenderer(W, H)
    try:
        b.share_scene(r)
        want = _want(name, 3)
        for m in (r, b):
            _check(m, p, radius, 3, want, what="member")
        assert b.select_clusters(radius, hi=10, min_pts=3)[0] == r.selection_count() == int(cr.select(want.sizes, 0, 10).sum())
        words = r.selection_words().copy()
        assert r.select_clusters(radius, hi=10, min_pts=3)[0] == b.selection_count() and np.array_equal(b.selection_words(), words)
    finally:
        b.dispose()


def test_two_runs_give_identical_words(r):
    name, p, radius = BY_NAME["chain of 4096 permuted"]
    r.set_scene_arrays(*_arrays(p))
    first = r.clusters(radius)
    for _ in range(2):
        again = r.clusters(radius)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]
    name, p, radius = _cluster_scene(r)
    first = r.clusters(radius, min_pts=6)
    again = r.clusters(radius, min_pts=6)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]


def test_frames_and_neighbour_counts_are_untouched_by_a_cluster_call(gh):
    cfg = gh.synth.CONFIGS["C1"]
    rows = gh.synth.config_rows("C1")
    scene = gh.Scene()
    scene.setData(rows)
    cam = gh.orbit_camera(3, width=cfg["width"], height=cfg["height"], fx=cfg["fx"])
    x = gh.HIPRenderer(cfg["width"], cfg["height"])
    try:
        x.render(scene, cam)
        frame, order = x.readPixelsFloat().copy(), x.lastDepthIndex().copy()
        counts, hist, info = x.neighbours(0.05, cap=16)
        labels, sizes, cinfo = x.clusters(0.05, min_pts=3)
        assert cinfo["in_scope"] == cfg["n"] == cinfo["core"] + cinfo["border"] + cinfo["noise"] and labels.shape == sizes.shape == (cfg["n"],)
        x.select_cluster_at(0.05, "largest", min_pts=3)
        again = x.neighbours(0.05, cap=16)
        assert np.array_equal(counts, again[0]) and np.array_equal(hist, again[1]) and info == again[2]
        x.render(scene, cam)
        assert np.array_equal(frame.view(np.uint32), x.readPixelsFloat().view(np.uint32)) and np.array_equal(order, x.lastDepthIndex())
    finally:
        x.dispose()


def test_every_refusal_touches_nothing(gh, r):
    _, p, radius = BY_NAME["n = 65"]
    r.set_scene_arrays(*_arrays(p))
    n = p.shape[0]
    prior = np.arange(n) % 3 == 0
    r.set_selection(prior)
    L, ctx = r._L, r._ctx
    labels, sizes = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    info = gh.GsrClusterInfo()
    sel = ctypes.c_uint32(77)
    cl = lambda radius=radius, min_pts=2, scope=0, budget=0, m=n, lab=True, siz=True: L.gsr_clusters(
        ctx, radius, min_pts, scope, budget, labels.ctypes.data if lab else None, sizes.ctypes.data if siz else None, m, ctypes.byref(info))
    pick = lambda radius=radius, min_pts=2, scope=0, budget=0, lo=0, hi=1, op=0: L.gsr_select_clusters(ctx, radius, min_pts, scope, budget, lo, hi, op,
                                                                                                     ctypes.byref(sel), ctypes.byref(info))
    at = lambda radius=radius, min_pts=2, scope=0, budget=0, seed=0, op=0: L.gsr_select_cluster_at(ctx, radius, min_pts, scope, budget, seed, op,
                                                                                                 ctypes.byref(sel), ctypes.byref(info))
    tiny, huge = 1e-200, 1e200                                         # radius * radius underflows; overflows
    refused = [lambda v=v, f=f: f(radius=v) for v in (0.0, -1.0, np.nan, np.inf, tiny, huge) for f in (cl, pick, at)]
    refused += [lambda f=f: f(min_pts=4096) for f in (cl, pick, at)]
    refused += [lambda f=f: f(scope=4) for f in (cl, pick, at)]
    refused += [lambda f=f: f(budget=nr.MAX_BUDGET + 1) for f in (cl, pick, at)]
    refused += [lambda: pick(op=4), lambda: pick(op=-1), lambda: at(op=4), lambda: pick(lo=2, hi=1), lambda: pick(lo=TOP, hi=0)]
    refused += [lambda: at(seed=n), lambda: at(seed=TOP - 1)]
    refused += [lambda: cl(m=n - 1), lambda: cl(m=n + 1), lambda: cl(m=0, siz=False), lambda: cl(m=n + 1, lab=False)]
    for k, call in enumerate(refused):
        assert call() == GSR_ERR_ARG, k
        assert L.gsr_last_error(ctx), k
        assert sel.value == 77 and not labels.any() and not sizes.any(), k
        assert r.selection_count() == int(prior.sum()), k
    assert np.array_equal(r.selection_words(), ar.pack(prior))
    assert L.gsr_clusters(None, radius, 0, 0, 0, None, None, 0, None) == GSR_ERR_ARG
    assert L.gsr_select_clusters(None, radius, 0, 0, 0, 0, 1, 0, None, None) == GSR_ERR_ARG
    assert L.gsr_select_cluster_at(None, radius, 0, 0, 0, 0, 0, None, None) == GSR_ERR_ARG
    # and what is NOT refused: every pointer NULL, lo == hi, min_pts 0 and 4095, the last splat as the seed
    assert L.gsr_clusters(ctx, radius, 0, 0, 0, None, None, 0, None) == 0
    assert L.gsr_clusters(ctx, radius, nr.MAX_CAP, 0, 0, None, None, 0, ctypes.byref(info)) == 0 and info.noise == n and info.largest_label == NONE
    assert pick(lo=5, hi=5, op=1) == 0 and sel.value == int(prior.sum())
    assert np.array_equal(r.selection_words(), ar.pack(prior))
    assert at(seed=n - 1, min_pts=0, op=1) == 0 and sel.value >= int(prior.sum())


def test_a_bound_above_the_budget_is_refused_before_any_walk(gh, r):
    p = np.tile(np.array([[0.5, 0.5, 0.5]], np.float32), (512, 1))
    r.set_scene_arrays(*_arrays(p))
    radius = 0.01
    floor = nr.pair_floor(p, radius)
    assert floor == 512 * 512
    prior = np.arange(512) % 5 == 0
    r.set_selection(prior)
    for call in (lambda: r.clusters(radius, min_pts=2, budget=1), lambda: r.select_clusters(radius, hi=2, min_pts=2, budget=1),
                 lambda: r.select_cluster_at(radius, 3, min_pts=2, budget=1)):
        with pytest.raises(gh.GsplatError) as ei:
            call()
        assert ei.value.code == GSR_ERR_ARG
        info = ei.value.info
        assert info["budget"] == 1 and info["in_scope"] == 512 and info["nonfinite"] == 0 and info["pair_bound"] >= floor
        assert info["core"] == info["border"] == info["noise"] == info["clusters"] == 0          # no walk was launched: nothing was counted
        assert str(info["pair_bound"]) in str(ei.value) and "budget of 1" in str(ei.value)       # the message names both numbers
        assert r.selection_count() == int(prior.sum()) and np.array_equal(r.selection_words(), ar.pack(prior))
    labels, sizes, info = r.clusters(radius, min_pts=2)                # the default budget passes
    assert not labels.any() and (sizes == 512).all() and info["budget"] == nr.DEFAULT_BUDGET and floor <= info["pair_bound"]
    assert r.clusters(radius, budget=info["pair_bound"])[2]["budget"] == info["pair_bound"]      # at the bound: not above it


def test_an_empty_scene_and_an_empty_scope_return_zeros(gh, r):
    _, p, radius = BY_NAME["n = 64"]
    r.set_scene_arrays(*_arrays(p))
    r.set_selection(None)
    zeros = {"in_scope": 0, "nonfinite": 0, "pair_bound": 0, "budget": nr.DEFAULT_BUDGET, "core": 0, "border": 0, "noise": 0, "clusters": 0,
             "largest_label": NONE, "largest_size": 0}
    labels, sizes, info = r.clusters(radius, scope="selected")
    assert (labels == NONE).all() and not sizes.any() and info == zeros
    assert r.select_clusters(radius, scope=("selected", "visible"))[0] == 0
    assert r.select_cluster_at(radius, "largest", scope="selected")[0] == 0 and r.select_cluster_at(radius, 5, scope="selected")[0] == 0
    e = gh.HIPRenderer(W, H)                                           # (never given a scene: the empty one)
    try:
        labels, sizes, info = e.clusters(radius)
        assert labels.size == 0 and sizes.size == 0 and info == zeros
        assert e.select_clusters(radius)[0] == 0 and e.select_cluster_at(radius, "largest")[0] == 0
    finally:
        e.dispose()


def test_bounds_twin_counts_nothing(gh):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    x = gh.HIPRenderer(W, H, lib_path=BOUNDS_LIB)
    try:
        for name in ("n = 1", "n = 65", "n = 257", "300 coincident", "lattice beyond the clamp", "non-finite rows", "chain of 4096 permuted",
                     "64 coincident groups of 65", "clusters and floaters"):
            _, p, radius = BY_NAME[name]
            x.set_scene_arrays(*_arrays(p))
            for min_pts in (0, 3):
                want = _want(name, min_pts)
                _check(x, p, radius, min_pts, want, what="bounds twin " + name)
                _check_select(x, want, 0, 4, radius, min_pts, what="bounds twin " + name)
                _check_at(x, want, cr.LARGEST, radius, min_pts, what="bounds twin " + name)
        buf = (ctypes.c_uint32 * 8)()
        assert L.gsr_debug_bounds_clusters(buf) == 0
        assert list(buf) == [0] * 8
        assert L.gsr_debug_bounds_neighbours(buf) == 0                 # the index and the core test are k_neighbours.hip's
        assert list(buf) == [0] * 8
    finally:
        x.dispose()

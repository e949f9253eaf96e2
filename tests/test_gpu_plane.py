"""Planes on the GPU: gsr_fit_plane, gsr_plane_inliers and gsr_select_plane (k_plane.hip, gsr_plane.cpp) against
tests/plane_reference.py, the specification in numpy f64, EXACTLY: all H scores, every integer of info, the plane by its bits and
the selection's words.  The shapes are plane_reference.families(): the smallest that can still go wrong -- one to three splats,
coincident and colinear ones, the wave, workgroup and chunk edges, every hypothesis count at which the grid changes, the tie
rule, rows at exactly the threshold and one ulp beyond, huge and tiny coordinates, non-finite rows, a candidate count past the
score grid's last chunk group, and 8192 splats of a tilted floor, a wall and clutter."""
import ctypes
import os

import numpy as np
import pytest

import attr_reference as ar
import plane_reference as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
W, H = 128, 96
GSR_ERR_ARG = -1
OPS = {"replace": 0, "add": 1, "subtract": 2, "intersect": 3}
FAMILIES = pr.families()
BY_NAME = {f[0]: f for f in FAMILIES}
FLOOR = "floor, wall and clutter"
_WANT = {}


def _want(name, scope_key=None, mask=None):
    """the reference's (info, scores) of a family in a scope, computed once"""
    key = (name, scope_key)
    if key not in _WANT:
        _, p, t, h, seed = BY_NAME[name]
        info, sc = pr.fit(p, t, h, seed, mask)
        sc.setflags(write=False)
        _WANT[key] = (info, sc)
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


def _same_info(got, want, what):
    for k, v in want.items():
        if k == "plane":
            assert np.array_equal(got[k].view(np.uint64), v.view(np.uint64)), (what, k, got[k], v)   # by its bits: -0.0 is not 0.0
        else:
            assert got[k] == v, (what, k, got[k], v)
    assert set(got) == set(want)


def _check(r, case, want, scope=(), what=""):
    """scores, info and plane of one fit against the reference, and plane_inliers of the reference's planes; returns info"""
    name, p, t, h, seed = case
    winfo, wsc = want
    plane, info, sc = r.fit_plane(t, hypotheses=h, seed=seed, scope=scope, scores=True)
    print(what, {k: v for k, v in info.items() if k != "plane"}, info["plane"])
    assert sc.dtype == np.uint32 and sc.shape == (h,)
    assert np.array_equal(sc, wsc), (what, np.nonzero(sc != wsc)[0][:8])
    _same_info(info, winfo, what)
    assert (plane is None) == (not winfo["found"])
    if plane is not None:
        assert np.array_equal(plane.view(np.uint64), winfo["plane"].view(np.uint64))
    return info


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_scores_info_plane_and_selection_equal_the_reference(r, case):
    name, p, t, h, seed = case
    n = p.shape[0]
    r.set_scene_arrays(*_arrays(p))
    want = _want(name)
    info = _check(r, case, want, what=name)
    # the scoring pass alone over the reference's planes: the same scores
    cand, _, _ = pr.candidates(p)
    planes, _, deg = pr.hypotheses(p, cand, h, seed)
    if (~deg).any():
        got, pinfo = r.plane_inliers(planes[~deg], t, info=True)
        assert np.array_equal(got, want[1][~deg]), name
        assert (pinfo["in_scope"], pinfo["nonfinite"], pinfo["hypotheses"], pinfo["tests"], pinfo["budget"]) == \
               (info["in_scope"], info["nonfinite"], int((~deg).sum()), int((~deg).sum()) * cand.size, pr.DEFAULT_BUDGET)
    # the picker under all four ops, and the consistency guarantee
    if info["found"]:
        picked = pr.select(p, info["plane"], -t, t)
        prior = np.arange(n) % 7 < 3
        for op in OPS:
            r.set_selection(prior)
            got = r.select_plane(info["plane"], within=t, op=op)
            after = ar.fold(prior, picked, OPS[op])
            assert got == int(after.sum()) == r.selection_count(), (name, op)
            assert np.array_equal(r.selection_words(), ar.pack(after)), (name, op)
        assert r.select_plane(info["plane"], within=t) == info["inliers"], name
    # visible: every third splat hidden
    hid = np.arange(n) % 3 == 1
    r.set_hidden(hid)
    _check(r, case, _want(name, "visible", ~hid), scope="visible", what=name + " visible")
    r.set_hidden(None)
    # selected: the fit sees the selection only, and leaves it alone
    sel = np.arange(n) % 5 != 2
    r.set_selection(sel)
    sinfo = _check(r, case, _want(name, "selected", sel), scope="selected", what=name + " selected")
    assert np.array_equal(r.selection_words(), ar.pack(sel))
    if sinfo["found"]:
        assert r.select_plane(sinfo["plane"], within=t, op="intersect") == sinfo["inliers"], name
        assert np.array_equal(r.selection_words(), ar.pack(sel & pr.select(p, sinfo["plane"], -t, t)))


def test_the_closed_interval_by_hand(r):
    up, down = np.nextafter(np.float32(0.75), np.float32(np.inf)), np.nextafter(np.float32(0.25), np.float32(-np.inf))
    z = np.array([0.25, 0.5, 0.75, up, down, np.nan, np.inf], np.float32)
    p = np.stack([np.arange(7, dtype=np.float32), np.zeros(7, np.float32), z], axis=1)
    r.set_scene_arrays(*_arrays(p))
    plane = (0.0, 0.0, 1.0, -0.5)
    got, info = r.plane_inliers([plane], 0.25, info=True)
    assert got.tolist() == [3] and info["in_scope"] == 7 and info["nonfinite"] == 2 and info["tests"] == 5
    assert r.select_plane(plane, within=0.25) == 3
    assert ar.unpack(r.selection_words(), 7).tolist() == [True, True, True, False, False, False, False]
    assert r.select_plane(plane, lo=0.25) == 3                         # exactly 0.25, one ulp beyond, and +inf; never the NaN
    assert ar.unpack(r.selection_words(), 7).tolist() == [False, False, True, True, False, False, True]
    assert r.select_plane(plane, hi=-0.25) == 2
    assert r.select_plane(plane) == 6                                  # (-inf, +inf): everything but the NaN
    assert r.plane_inliers([(0.0, 0.0, 2.0, -1.0)], 0.5).tolist() == [3]   # used as given, not normalised


def test_under_the_floor_and_alignment(gh, r):
    name, p, t, h, seed = BY_NAME[FLOOR]
    r.set_scene_arrays(*_arrays(p))
    plane, info = r.fit_plane(t, hypotheses=h, seed=seed)
    _same_info(info, _want(name)[0], name)
    under = pr.select(p, plane, -np.inf, -t)
    assert r.select_plane(plane, hi=-t) == int(under.sum()) and 0 < under.sum() < p.shape[0]
    assert np.array_equal(r.selection_words(), ar.pack(under))
    # fit, plane_alignment, scene_rotate, scene_translate: the floor lies at y = 0.  After the two edits every coordinate lies
    # below 16, so each of the two f32 stores moves a coordinate by at most 2^-21 (half an ulp of a value below 16); a unit normal
    # turns the two into at most sqrt(3) * 2^-20 < 2^-19 of distance.
    q, tr = gh.plane_alignment(plane, (0, 1, 0))
    wq, wt = pr.alignment(plane, (0, 1, 0))
    assert np.array_equal(q.view(np.uint64), wq.view(np.uint64)) and np.array_equal(tr.view(np.uint64), wt.view(np.uint64))
    r.scene_rotate(q)
    r.scene_translate(tr)
    now = r.read_scene()[1].reshape(-1, 3)
    assert np.abs(now).max() < 16.0
    got = r.plane_inliers([(0.0, 1.0, 0.0, 0.0)], t + 2.0 ** -19)
    print("inliers before", info["inliers"], "after", int(got[0]))
    assert int(got[0]) >= info["inliers"]


def test_two_members_of_a_shared_scene_agree(gh, r):
    case = BY_NAME["n = 257"]
    r.set_scene_arrays(*_arrays(case[1]))
    b = gh.HIPRenderer(W, H)
    try:
        b.share_scene(r)
        for m in (r, b):
            _check(m, case, _want(case[0]), what="member")
    finally:
        b.dispose()


def test_the_budget(gh, r):
    case = BY_NAME["n = 257"]
    name, p, t, h, seed = case
    r.set_scene_arrays(*_arrays(p))
    prior = np.arange(257) % 5 == 0
    r.set_selection(prior)
    for call in (lambda: r.fit_plane(t, hypotheses=h, seed=seed, budget=h * 257 - 1), lambda: r.plane_inliers(np.tile([0.0, 0.0, 1.0, 0.0], (h, 1)), t, budget=h * 257 - 1)):
        with pytest.raises(gh.GsplatError) as ei:
            call()
        assert ei.value.code == GSR_ERR_ARG
        info = ei.value.info
        assert info["budget"] == h * 257 - 1 and info["tests"] == h * 257 and info["in_scope"] == 257 and info["nonfinite"] == 0
        assert info["found"] == 0 and info["inliers"] == 0 and not info["plane"].any()
        assert str(h * 257) in str(ei.value) and "budget of %d" % (h * 257 - 1) in str(ei.value)   # the message names both numbers
        assert np.array_equal(r.selection_words(), ar.pack(prior))
    _, info = r.fit_plane(t, hypotheses=h, seed=seed, budget=h * 257)   # at the budget: not above it
    assert info["budget"] == h * 257 and info["found"] == 1
    with pytest.raises(gh.GsplatError) as ei:
        r.fit_plane(t, budget=pr.MAX_BUDGET + 1)
    assert ei.value.code == GSR_ERR_ARG and "GSR_NEIGHBOUR_MAX_BUDGET" in str(ei.value)
    assert r.fit_plane(t, hypotheses=h, budget=pr.MAX_BUDGET)[1]["budget"] == pr.MAX_BUDGET


def test_every_refusal_leaves_the_selection_alone(gh, r):
    _, p, t, h, seed = BY_NAME["n = 65"]
    r.set_scene_arrays(*_arrays(p))
    n = p.shape[0]
    prior = np.arange(n) % 3 == 0
    r.set_selection(prior)
    L, ctx = r._L, r._ctx
    info = gh.GsrPlaneInfo()
    sel = ctypes.c_uint32(77)
    sc = np.full(8, 77, np.uint32)
    good = np.array([0.0, 0.0, 1.0, 0.0], np.float64)
    planes = lambda *rows: np.ascontiguousarray(rows, dtype=np.float64)
    fit = lambda t=t, h=8, scope=0, budget=0, i=info: L.gsr_fit_plane(ctx, t, h, 0, scope, budget, sc.ctypes.data, ctypes.byref(i) if i is not None else None)
    inl = lambda pl=good, k=1, t=t, scope=0, budget=0, out=sc: L.gsr_plane_inliers(ctx, None if pl is None else pl.ctypes.data, k, t, scope, budget,
                                                                                    None if out is None else out.ctypes.data, ctypes.byref(info))
    pick = lambda pl=good, lo=-1.0, hi=1.0, op=0: L.gsr_select_plane(ctx, None if pl is None else pl.ctypes.data, lo, hi, op, ctypes.byref(sel))
    refused = [lambda v=v: fit(t=v) for v in (-1.0, np.nan, np.inf, -np.inf)] + [lambda v=v: inl(t=v) for v in (-1e-300, np.nan, np.inf)]
    refused += [lambda: fit(h=0), lambda: fit(h=4097), lambda: inl(k=0), lambda: inl(pl=np.tile(good, (4097, 1)), k=4097)]
    refused += [lambda: fit(scope=4), lambda: inl(scope=8), lambda: pick(op=4), lambda: pick(op=-1)]
    refused += [lambda: fit(i=None), lambda: inl(pl=None), lambda: inl(out=None), lambda: pick(pl=None)]
    refused += [lambda v=v: inl(pl=planes([0.0, v, 1.0, 0.0])) for v in (np.nan, np.inf)] + [lambda: inl(pl=planes([0.0, 0.0, 0.0, 1.0]))]
    refused += [lambda: inl(pl=planes(good, [0.0, 0.0, 0.0, 0.0]), k=2), lambda: pick(pl=planes([0.0, 0.0, 1.0, np.nan])), lambda: pick(pl=planes([0.0, 0.0, 0.0, 1.0]))]
    refused += [lambda: pick(lo=np.nan), lambda: pick(hi=np.nan), lambda: pick(lo=1.0, hi=0.5)]
    refused += [lambda: fit(budget=pr.MAX_BUDGET + 1), lambda: inl(budget=pr.MAX_BUDGET + 1)]
    for k, call in enumerate(refused):
        assert call() == GSR_ERR_ARG, k
        assert L.gsr_last_error(ctx), k
        assert sel.value == 77 and (sc == 77).all(), k
        assert r.selection_count() == int(prior.sum()), k
    assert np.array_equal(r.selection_words(), ar.pack(prior))
    assert L.gsr_fit_plane(None, t, 8, 0, 0, 0, None, ctypes.byref(info)) == GSR_ERR_ARG
    assert L.gsr_plane_inliers(None, good.ctypes.data, 1, t, 0, 0, sc.ctypes.data, None) == GSR_ERR_ARG
    assert L.gsr_select_plane(None, good.ctypes.data, -1.0, 1.0, 0, None) == GSR_ERR_ARG
    # and what is NOT refused: no scores, no info for the inliers, no count for the picker, lo == hi, a threshold of 0
    assert L.gsr_fit_plane(ctx, 0.0, 8, 0, 0, 0, None, ctypes.byref(info)) == 0
    assert L.gsr_plane_inliers(ctx, good.ctypes.data, 1, 0.0, 0, 0, sc.ctypes.data, None) == 0
    assert np.array_equal(r.selection_words(), ar.pack(prior))         # neither touches the selection
    assert L.gsr_select_plane(ctx, good.ctypes.data, 0.5, 0.5, 1, None) == 0


def test_an_empty_scene_and_an_empty_scope_return_zeros(gh, r):
    _, p, t, h, seed = BY_NAME["n = 64"]
    r.set_scene_arrays(*_arrays(p))
    r.set_selection(None)
    zeros = pr.fit(p, t, h, seed, np.zeros(64, bool))[0]
    assert zeros["hypotheses"] == zeros["found"] == zeros["tests"] == 0
    plane, info, sc = r.fit_plane(t, hypotheses=h, seed=seed, scope="selected", scores=True)
    assert plane is None and not sc.any()
    _same_info(info, zeros, "empty scope")
    assert not r.plane_inliers([(0, 0, 1, 0)], t, scope=("selected", "visible")).any()
    e = gh.HIPRenderer(W, H)                                           # (never given a scene: the empty one)
    try:
        plane, info = e.fit_plane(t)
        assert plane is None
        _same_info(info, zeros, "empty scene")
        assert not e.plane_inliers([(0, 0, 1, 0)], t).any() and e.select_plane((0, 0, 1, 0)) == 0
    finally:
        e.dispose()


def test_bounds_twin_counts_nothing(gh):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    x = gh.HIPRenderer(W, H, lib_path=BOUNDS_LIB)
    try:
        for name in ("n = 1", "n = 3", "n = 65", "n = 257", "n = 1025 (chunk)", "H = 4096", "non-finite rows", FLOOR):
            case = BY_NAME[name]
            _, p, t, h, seed = case
            x.set_scene_arrays(*_arrays(p))
            info = _check(x, case, _want(name), what="bounds twin " + name)
            hid = np.arange(p.shape[0]) % 3 == 1
            x.set_hidden(hid)
            _check(x, case, _want(name, "visible", ~hid), scope="visible", what="bounds twin visible " + name)
            x.set_hidden(None)
            if info["found"]:
                assert x.select_plane(info["plane"], within=t) == info["inliers"]
                assert x.plane_inliers([info["plane"]], t).tolist() == [info["inliers"]]
        buf = (ctypes.c_uint32 * 8)()
        assert L.gsr_debug_bounds_plane(buf) == 0
        assert list(buf) == [0] * 8
    finally:
        x.dispose()

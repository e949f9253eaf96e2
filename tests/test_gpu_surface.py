"""Point-to-plane registration on the GPU: gsr_match_surface and gsr_register_surface (gsr_match.cpp over k_match.hip's
k_match_surface_rows and the 29-wide tree, the target's normals by gsr_normals' own device path) against tests/surface_reference.py
bit for bit -- every family's counts and 29 sums; on the box corner the transform, the status, the number of steps and every step's
values, with OWN and with KNN normals; the two early ends; the same bits twice; the context as its own target and members of
shared scenes; the target left as it was; the scratch; the refusals; and the bounds-checked twin counting nothing."""
import ctypes
import math
import os

import numpy as np
import pytest

import normal_reference as nref
import register_reference as rr
import surface_reference as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
W, H = 128, 96
GSR_ERR_ARG = -1
STATUS = {sr.CONVERGED: "converged", sr.MAX_ITERATIONS: "max_iterations", sr.TOO_FEW: "too_few", sr.DEGENERATE: "degenerate"}
OWN = {"source": "own"}
KNN = {"source": "knn", "k": 8, "radius": 0.15}
FAMILIES = sr.families()
BY_NAME = {f[0]: f for f in FAMILIES}
SMALL = ("1 x 1", "65 x 300", "257 x 300", "non-finite rows", "no normal at all")
_WANT = {}


def _want(name):
    """(pairs, surface_pairs, sum29, match info) of a family, computed once"""
    if name not in _WANT:
        _, src, tgt, radius, M, _, _, nrm = BY_NAME[name]
        idx, d2, info = rr.match(src, tgt, radius, M)
        _WANT[name] = sr.sums(src, tgt, nrm, idx, d2, M) + (info,)
    return _WANT[name]


def _want_corner(which, max_iterations=16):
    """(normals, (M, info)) of the corner under OWN or KNN normals, computed once"""
    if (which, max_iterations) not in _WANT:
        c = sr.corner_scenario()
        nrm = c["target_normals"] if which == "own" else nref.knn_normals(c["target"], KNN["radius"], KNN["k"])[0]
        _WANT[(which, max_iterations)] = (nrm, sr.register_surface(c["source"], c["target"], nrm, sr.RADIUS, max_iterations=max_iterations, tolerance=2.0 ** -30))
    return _WANT[(which, max_iterations)]


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


@pytest.fixture(scope="module")
def pair(gh):
    a, b = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    yield a, b
    a.dispose()
    b.dispose()


def _arrays(p, rot=None, scl=None, seed=1):
    """(data, positions, rotations, scales) around the positions p; seeded rotations and scales where none are given"""
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    data[:, 0:3] = p.view(np.uint32)
    rot = rng.normal(0, 1, (n, 4)).astype(np.float32) if rot is None else np.ascontiguousarray(rot, dtype=np.float32)
    scl = rng.uniform(0.01, 0.1, (n, 3)).astype(np.float32) if scl is None else np.ascontiguousarray(scl, dtype=np.float32)
    return data.reshape(-1), p.reshape(-1), rot.reshape(-1), scl.reshape(-1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def _load_corner(a, b, faces=(0, 1, 2)):
    c = sr.corner_scenario()
    tgt, rot, scl, _ = sr.corner_faces(faces)
    a.set_scene_arrays(*_arrays(c["source"], c["source_rotations"], c["source_scales"]))
    b.set_scene_arrays(*_arrays(tgt, rot, scl, seed=2))
    return c


def _same_sums(got, info, want, what):
    pairs, surface_pairs, s29, winfo = want
    print(what, got["pairs"], got["surface_pairs"], info)
    assert got["pairs"] == pairs and got["surface_pairs"] == surface_pairs, (what, got, pairs, surface_pairs)
    assert np.array_equal(_bits(got["sum"]), _bits(s29)), (what, got["sum"], s29)
    for k in ("in_scope", "nonfinite", "target_indexed", "matched", "pair_bound"):
        assert info[k] == winfo[k], (what, k, info, winfo)


def _same_register(M, info, want, what):
    wM, winfo = want
    print(what, info)
    assert info["status"] == STATUS[winfo["status"]] and info["iterations"] == winfo["iterations"], (what, info, winfo)
    assert info["pairs"] == winfo["pairs"] and info["surface_pairs"] == winfo["surface_pairs"], (what, info, winfo)
    assert np.array_equal(_bits(M), _bits(wM)), (what, M, wM)
    for k in ("rms", "surface_rms", "delta"):
        assert _bits([info[k]])[0] == _bits([winfo[k]])[0], (what, k, info, winfo)
    if "step_pairs" in info:
        assert info["step_pairs"].tolist() == winfo["step_pairs"] and info["step_surface_pairs"].tolist() == winfo["step_surface_pairs"], what
        assert np.array_equal(_bits(info["step_rms"]), _bits(winfo["step_rms"])), what
        assert np.array_equal(_bits(info["step_surface_rms"]), _bits(winfo["step_surface_rms"])), what


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_match_surface_equals_the_reference_bit_for_bit(pair, case):
    a, b = pair
    name, src, tgt, radius, M, rot, scl, nrm = case
    a.set_scene_arrays(*_arrays(src))
    b.set_scene_arrays(*_arrays(tgt, rot, scl, seed=2))
    got = b.normals(source="own", variation=False, found=False)[0]
    assert np.array_equal(got.view(np.uint32), nrm.view(np.uint32)), name    # the device's normals are the family's
    sums, info = a.match_surface(b, radius, normals=OWN, transform=M)
    _same_sums(sums, info, _want(name), name)
    if name == "no normal at all":
        assert sums["surface_pairs"] == 0 and sums["pairs"] > 0 and not _bits(sums["sum"]).any()   # every sum +0.0
    elif name.endswith((" x 300", " x 512")):
        assert 0 < sums["surface_pairs"] < sums["pairs"]                # matches with and without a normal
    # gsr_match with the same arguments gives idx and d2 for a host that wants them: the same rows, the same sums
    idx, d2, _, _ = a.match(b, radius, transform=M)
    assert np.array_equal(_bits(sr.tree(sr.rows(src, tgt, nrm, idx, M, d2))), _bits(sums["sum"])), name


@pytest.mark.parametrize("which", ["own", "knn"])
def test_register_surface_on_the_corner_equals_the_reference_bit_for_bit(gh, pair, which):
    a, b = pair
    c = _load_corner(a, b)
    options = OWN if which == "own" else KNN
    nrm, want = _want_corner(which)
    assert np.array_equal(b.normals(options.get("radius"), k=options.get("k", 8), source=which)[0].view(np.uint32), nrm.view(np.uint32))
    M, info = a.register_surface(b, sr.RADIUS, normals=options, max_iterations=16, tolerance=2.0 ** -30, history=True)
    _same_register(M, info, want, which + ", history")
    assert info["status"] == "converged" and info["valid"] == int((~np.isnan(nrm[:, 0])).sum())
    again, info2 = a.register_surface(b, sr.RADIUS, normals=options, max_iterations=16, tolerance=2.0 ** -30)       # the same call twice: the same bits
    assert "step_pairs" not in info2 and np.array_equal(_bits(again), _bits(M))
    _same_register(again, info2, want, which + ", again")
    # one step as data, and the pure solve on it: the loop's first step
    sums, _ = a.match_surface(b, sr.RADIUS, normals=options)
    wsp, ws29 = want[1]["step_sums"][0]
    assert sums["surface_pairs"] == wsp and np.array_equal(_bits(sums["sum"]), _bits(ws29))
    D, rms, degenerate = gh.surface_solve(sums)
    wD, wrms, wdeg = sr.surface_solve(wsp, ws29)
    assert degenerate == wdeg == 0 and np.array_equal(_bits(D), _bits(wD)) and _bits([rms])[0] == _bits([wrms])[0]
    # from the result: one more step changes nothing worth a step
    M2, info3 = a.register_surface(b, sr.RADIUS, normals=options, transform=M, max_iterations=3, tolerance=2.0 ** -30)
    _same_register(M2, info3, sr.register_surface(c["source"], c["target"], nrm, sr.RADIUS, M, max_iterations=3, tolerance=2.0 ** -30), which + ", restart")
    assert np.array_equal(a.read_scene()[1], c["source"].reshape(-1))  # the scene was never written


def test_one_face_is_degenerate_and_a_target_without_normals_too_few(pair):
    a, b = pair
    c = _load_corner(a, b, faces=(2,))
    tgt, _, _, nrm = sr.corner_faces((2,))
    M, info = a.register_surface(b, sr.RADIUS, normals=OWN, max_iterations=8, tolerance=2.0 ** -30, history=True)
    want = sr.register_surface(c["source"], tgt, nrm, sr.RADIUS, max_iterations=8, tolerance=2.0 ** -30)
    _same_register(M, info, want, "one face")
    assert info["status"] == "degenerate" and info["iterations"] == 1 and info["delta"] == math.inf and np.array_equal(_bits(M), _bits(rr.IDENTITY))
    # every rotation zero: no splat of the target has a normal, every match is a pair and none a surface pair
    b.set_scene_arrays(*_arrays(tgt, np.zeros((tgt.shape[0], 4), np.float32), np.tile(sr.FACE_SCALES, (tgt.shape[0], 1)), seed=2))
    M, info = a.register_surface(b, sr.RADIUS, normals=OWN, max_iterations=8, history=True)
    want = sr.register_surface(c["source"], tgt, np.full_like(nrm, np.nan), sr.RADIUS, max_iterations=8)
    _same_register(M, info, want, "no normals")
    assert info["status"] == "too_few" and info["iterations"] == 1 and info["pairs"] > 0 and info["surface_pairs"] == 0 and info["valid"] == 0
    assert info["surface_rms"] == math.inf and info["step_surface_pairs"].tolist() == [0]
    # max_iterations, and a tolerance of zero
    _load_corner(a, b)
    M, info = a.register_surface(b, sr.RADIUS, normals=OWN, max_iterations=2, tolerance=0.0, history=True)
    _same_register(M, info, sr.register_surface(c["source"], c["target"], c["target_normals"], sr.RADIUS, max_iterations=2, tolerance=0.0), "two steps")
    assert info["status"] == "max_iterations" and info["iterations"] == 2


def test_target_is_the_context_itself_and_members_of_shared_scenes(gh, pair):
    a, b = pair
    case = BY_NAME["257 x 300"]
    name, src, tgt, radius, M, rot, scl, nrm = case
    # the context as its own target: every finite splat matches itself, e = T - Q under M
    b.set_scene_arrays(*_arrays(tgt, rot, scl, seed=2))
    sums, info = b.match_surface(b, radius, normals=OWN, transform=M)
    idx, d2, winfo = rr.match(tgt, tgt, radius, M)
    _same_sums(sums, info, sr.sums(tgt, tgt, nrm, idx, d2, M) + (winfo,), "self")
    sums, info = b.match_surface(b, radius, normals={"source": "knn", "k": 6, "radius": 0.3}, transform=M)
    knn = nref.knn_normals(tgt, 0.3, 6)[0]
    _same_sums(sums, info, sr.sums(tgt, tgt, knn, idx, d2, M) + (winfo,), "self, knn")
    a.set_scene_arrays(*_arrays(src))
    a2, b2 = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    try:
        a2.share_scene(a)
        b2.share_scene(b)
        for s in (a, a2):
            for t in (b, b2):
                got, info = s.match_surface(t, radius, normals=OWN, transform=M)
                _same_sums(got, info, _want(name), "members")
        # a member of the target's own scene as the source
        got, info = b2.match_surface(b, radius, normals=OWN, transform=M)
        _same_sums(got, info, sr.sums(tgt, tgt, nrm, idx, d2, M) + (winfo,), "member of the target's scene")
    finally:
        a2.dispose()
        b2.dispose()


def test_the_target_renders_the_same_frame_and_reads_the_same_selection(gh, pair):
    a, b = pair
    c = _load_corner(a, b)
    cam = gh.orbit_camera(3, width=W, height=H, fx=120.0)
    sel = np.arange(1200) % 4 == 1
    hid = np.arange(1200) % 9 == 2
    b.set_selection(sel)
    b.set_hidden(hid)

    def frame():
        b.set_camera(cam)
        b._check(b._L.gsr_render(b._ctx))
        return b.lastDepthIndex().copy(), b.readPixelsFloat().copy()

    before = frame()
    a.register_surface(b, sr.RADIUS, normals=OWN, max_iterations=3)
    a.register_surface(b, sr.RADIUS, normals=KNN, max_iterations=2)
    sums, _ = a.match_surface(b, sr.RADIUS, normals=OWN, target_scope="visible")
    idx, d2, _ = rr.match(c["source"], c["target"], sr.RADIUS, None, None, ~hid)
    want = sr.sums(c["source"], c["target"], nref.own_normals(c["target"], c["target_rotations"], c["target_scales"], ~hid)[0], idx, d2)
    assert (sums["pairs"], sums["surface_pairs"]) == want[:2] and np.array_equal(_bits(sums["sum"]), _bits(want[2]))
    assert np.array_equal(b.readPixelsFloat().view(np.uint32), before[1].view(np.uint32))   # the last frame is still there
    after = frame()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1].view(np.uint32), before[1].view(np.uint32))
    assert np.array_equal(b.selection(), sel) and np.array_equal(b.hidden(), hid)
    assert np.array_equal(b.read_scene()[1], c["target"].reshape(-1)) and np.array_equal(a.read_scene()[1], c["source"].reshape(-1))
    b.set_hidden(None)
    b.set_selection(None)


def _scratch(r, name):
    fn = getattr(r._L, name)
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    out = ctypes.c_uint64(99)
    assert fn(r._ctx, ctypes.byref(out)) == 0
    return out.value


def test_no_scratch_before_the_first_call_and_the_documented_bytes_after(gh):
    x, y = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    try:
        name, src, tgt, radius, M, rot, scl, nrm = BY_NAME["257 x 300"]
        x.set_scene_arrays(*_arrays(src))
        y.set_scene_arrays(*_arrays(tgt, rot, scl, seed=2))
        for c in (x, y):
            assert _scratch(c, "gsr_debug_match_scratch") == 0 and _scratch(c, "gsr_debug_normals_scratch") == 0
        x.match_surface(y, radius, normals=OWN, transform=M)
        # ctx: the info words, idx and d2, and three 29-wide rows (two groups and their sum); no 16-wide tree.  target: what
        # gsr_normals would hold, 32 bytes of info words and 12 + 8 + 4 per splat
        assert _scratch(x, "gsr_debug_match_scratch") == 48 + 257 * 12 + 3 * 232
        assert _scratch(y, "gsr_debug_normals_scratch") == 32 + 24 * 300
        assert _scratch(y, "gsr_debug_match_scratch") == 0 and _scratch(x, "gsr_debug_normals_scratch") == 0
        x.register_surface(y, radius, normals=OWN, transform=M, max_iterations=2)
        y.normals(source="own")
        assert _scratch(x, "gsr_debug_match_scratch") == 48 + 257 * 12 + 3 * 232 and _scratch(y, "gsr_debug_normals_scratch") == 32 + 24 * 300
        x.match(y, radius, transform=M, sums=True)                     # the 16-wide rows are their own
        assert _scratch(x, "gsr_debug_match_scratch") == 48 + 257 * 12 + 3 * 232 + 3 * 128
    finally:
        x.dispose()
        y.dispose()


def test_refusals(gh, pair):
    a, b = pair
    name, src, tgt, radius, M, rot, scl, nrm = BY_NAME["65 x 300"]
    a.set_scene_arrays(*_arrays(src))
    b.set_scene_arrays(*_arrays(tgt, rot, scl, seed=2))
    L, ctx, tctx = a._L, a._ctx, b._ctx
    out = np.full(12, 77.0)
    sums, info, rinfo = gh.GsrSurfaceSums(), gh.GsrMatchInfo(), gh.GsrRegisterSurfaceInfo()
    sums.pairs = 77

    def options(source=1, scope=0, k=8, radius=0.3, budget=0, oriented=0, toward=(0.0, 0.0, 0.0)):
        o = gh.GsrNormalOptions()
        o.source, o.scope, o.k, o.radius, o.budget, o.oriented = source, scope, k, radius, budget, oriented
        o.toward[:] = toward
        return ctypes.byref(o)

    good = np.ascontiguousarray(M, dtype=np.float64)
    ptr = lambda m: None if m is None else m.ctypes.data
    mat = lambda t=tctx, m=good, r=radius, scope=0, ts=0, budget=0, o=None: L.gsr_match_surface(ctx, t, ptr(m), r, scope, ts, budget, o or options(), ctypes.byref(sums),
                                                                                               ctypes.byref(info))
    reg = lambda t=tctx, m=good, r=radius, scope=0, ts=0, budget=0, o=None, it=4, tol=0.0, ri=rinfo: L.gsr_register_surface(
        ctx, t, ptr(m), r, scope, ts, budget, o or options(), it, tol, out.ctypes.data, ctypes.byref(ri))
    bad = good.copy()
    bad[5] = np.nan
    short = gh.GsrRegisterSurfaceInfo()
    steps = np.zeros(3, np.float64)
    short.step_surface_rms, short.step_rows = steps.ctypes.data, 3
    refused = []
    for f in (mat, reg):
        refused += [lambda f=f: f(t=None), lambda f=f: f(m=bad), lambda f=f: f(scope=4), lambda f=f: f(ts=8), lambda f=f: f(budget=rr.MAX_BUDGET + 1)]
        refused += [lambda f=f, v=v: f(r=v) for v in (0.0, -1.0, np.nan, np.inf)]
        refused += [lambda f=f: f(ts=1, o=options(scope=0)), lambda f=f: f(ts=0, o=options(scope=2))]          # options->scope is not target_scope
        refused += [lambda f=f: f(o=options(source=2)), lambda f=f: f(o=options(source=0, k=1)), lambda f=f: f(o=options(source=0, k=33)),
                    lambda f=f: f(o=options(source=0, radius=0.0)), lambda f=f: f(o=options(budget=rr.MAX_BUDGET + 1)),
                    lambda f=f: f(o=options(oriented=1, toward=(np.nan, 0.0, 0.0)))]
    refused += [lambda: L.gsr_match_surface(ctx, tctx, None, radius, 0, 0, 0, None, None, None), lambda: L.gsr_register_surface(ctx, tctx, None, radius, 0, 0, 0, None, 4, 0.0, None, None)]
    refused += [lambda: reg(it=0), lambda: reg(it=257), lambda: reg(tol=-1.0), lambda: reg(tol=np.nan), lambda: reg(ri=short)]
    for k, call in enumerate(refused):
        assert call() == GSR_ERR_ARG, k
        assert L.gsr_last_error(ctx), k
        assert sums.pairs == 77 and (out == 77.0).all(), k
    assert L.gsr_match_surface(None, tctx, None, radius, 0, 0, 0, options(), None, None) == GSR_ERR_ARG
    assert L.gsr_register_surface(None, tctx, None, radius, 0, 0, 0, options(), 4, 0.0, None, None) == GSR_ERR_ARG
    # OWN on a target without rotations and scales: gsr_normals' refusal, and the message reaches ctx
    data, pos, _, _ = _arrays(tgt, seed=2)
    b.set_raw_scene(data, pos)
    for f in (mat, reg):
        assert f() == GSR_ERR_ARG and b"gsr_set_scene_rows" in L.gsr_last_error(ctx)
    assert mat(o=options(source=0)) == 0                                # KNN needs no rows
    with pytest.raises(ValueError):
        a.register_surface(b, radius, normals={"source": "knn"})        # the host: KNN without a radius
    with pytest.raises(ValueError):
        a.match_surface(b, radius, normals={"sauce": "own"})
    # the budget: the walk's bound above it is refused with both numbers, and the info filled
    b.set_scene_arrays(*_arrays(tgt, rot, scl, seed=2))
    bound = rr.match(src, tgt, radius, M)[2]["pair_bound"]
    with pytest.raises(gh.GsplatError) as ei:
        a.match_surface(b, radius, normals=OWN, transform=M, budget=bound - 1)
    assert ei.value.code == GSR_ERR_ARG and str(bound) in str(ei.value) and ei.value.info["pair_bound"] == bound
    with pytest.raises(gh.GsplatError) as ei:
        a.register_surface(b, radius, normals=OWN, transform=M, budget=bound - 1)
    assert ei.value.code == GSR_ERR_ARG and "budget of %d" % (bound - 1) in str(ei.value)
    # and what is NOT refused: no out pointer at all, a NULL transform, oriented normals (the sign cannot matter)
    assert L.gsr_match_surface(ctx, tctx, None, radius, 0, 0, 0, options(), None, None) == 0
    assert L.gsr_register_surface(ctx, tctx, None, radius, 0, 0, 0, options(), 1, np.inf, None, None) == 0
    plain, _ = a.match_surface(b, radius, normals=OWN, transform=M)
    assert mat(o=options(oriented=1, toward=(5.0, -3.0, 2.0))) == 0
    assert sums.surface_pairs == plain["surface_pairs"] and np.array_equal(_bits(np.array(sums.sum)), _bits(plain["sum"]))


def test_empty_scene_and_empty_target(gh, pair):
    a, b = pair
    name, src, tgt, radius, M, rot, scl, nrm = BY_NAME["64 x 300"]
    a.set_scene_arrays(*_arrays(src))
    e = gh.HIPRenderer(W, H)                                           # (never given a scene: the empty one)
    try:
        sums, info = a.match_surface(e, radius, normals=OWN, transform=M)
        assert sums["pairs"] == 0 and sums["surface_pairs"] == 0 and not _bits(sums["sum"]).any() and info["in_scope"] == 64 and info["target_indexed"] == 0
        Mr, rinfo = a.register_surface(e, radius, normals=OWN, transform=M, history=True)
        assert rinfo["status"] == "too_few" and rinfo["iterations"] == 1 and rinfo["pairs"] == 0 and rinfo["rms"] == math.inf and rinfo["valid"] == 0
        assert np.array_equal(_bits(Mr), _bits(M))
        sums, info = e.match_surface(a, radius, normals=OWN)
        assert sums["pairs"] == 0 and not _bits(sums["sum"]).any() and info["in_scope"] == 0
        assert e.register_surface(a, radius, normals=OWN)[1]["status"] == "too_few"
    finally:
        e.dispose()


def test_bounds_twin_counts_nothing(gh):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    x, y = gh.HIPRenderer(W, H, lib_path=BOUNDS_LIB), gh.HIPRenderer(W, H, lib_path=BOUNDS_LIB)
    try:
        for name in SMALL:
            _, src, tgt, radius, M, rot, scl, nrm = BY_NAME[name]
            x.set_scene_arrays(*_arrays(src))
            y.set_scene_arrays(*_arrays(tgt, rot, scl, seed=2))
            sums, info = x.match_surface(y, radius, normals=OWN, transform=M)
            _same_sums(sums, info, _want(name), "bounds twin " + name)
            x.register_surface(y, radius, normals=OWN, transform=M, max_iterations=2)
            if tgt.shape[0] > 8:
                x.match_surface(y, radius, normals={"source": "knn", "k": 4, "radius": radius}, transform=M)
        for fn in (L.gsr_debug_bounds_match, L.gsr_debug_bounds_match_surface, L.gsr_debug_bounds_neighbours, L.gsr_debug_bounds_normals):
            buf = (ctypes.c_uint32 * 8)()
            assert fn(buf) == 0
            assert list(buf) == [0] * 8
    finally:
        x.dispose()
        y.dispose()

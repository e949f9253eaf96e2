"""Splat data on the GPU: gsr_attr_stats, gsr_attr_histogram and gsr_select_attr (k_attr.hip, gsr_attr.cpp) against
tests/attr_reference.py, the specification in numpy f64, EXACTLY: counts as integers, selection words bit for bit, min / max
with ==.  Scene sizes sit on the word, half-wave, wave and workgroup edges, and one lies above a single pass of the grid-stride
loop: the reductions run on at most ATTR_MAX_GRID = 1024 workgroups of ATTR_THREADS = 256 (attr_grid, k_attr.hip: four per
compute unit for k_attr_stats, two for k_attr_hist), so one pass covers at most 262144 splats on any device and
BIG = 262144 + 333 needs a second one of k_attr_stats and a third of k_attr_hist on 256 compute units."""
import ctypes
import os

import numpy as np
import pytest

import attr_reference as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
W, H = 128, 96
BIG = 1024 * 256 + 333
SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, BIG)
BINS = (1, 2, 64, 256, 257, 4096)
SCOPES = (0, 1, 2, 3)
SCENE_ATTRS = tuple(a for a in ar.ATTRS if not a.startswith("contrib"))
ORIGIN = (0.1, -0.2, 0.3)          # no component is an f32: every dx is inexact in f32, exact in f64, and dx * dx rounds
RANGES = {"x": (-1.5, 2.25), "y": (0.1, 1.3), "z": (-4.0, 4.0), "distance": (0.3, 3.1), "red": (0.0, 256.0), "green": (16.0, 200.0),
          "blue": (0.0, 255.0), "opacity": (0.0, 256.0), "scale_x": (0.0, 1.0), "scale_y": (0.01, 0.77), "scale_z": (-1.0, 1.0),
          "scale_min": (0.0, 0.5), "scale_max": (0.2, 1.3)}
PATTERNS = ("empty", "full", "first and last", "every 64th word zero", "last word partial", "random 1 %")
GSR_ERR_ARG = -1


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


def _scene(n, seed=3, plant=True):
    """(data, positions, rotations, scales) of n splats: seeded, with NaN, +-inf and -0.0 planted in positions and scales"""
    rng = np.random.default_rng(seed * 100003 + n)
    pos = rng.normal(0.4, 1.1, (n, 3)).astype(np.float32)
    scl = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    rgba = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if plant:
        for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0)):
            for axis in range(3):
                i = (7 * k + 11 * axis + 2) % n
                pos[i, axis] = v
                scl[(i + 3) % n, (axis + 1) % 3] = v
    data = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    data[:, 0:3] = pos.view(np.uint32)
    data[:, 7] = rgba
    rot = rng.normal(0, 1, (n, 4)).astype(np.float32)
    return data.reshape(-1), pos.reshape(-1), rot.reshape(-1), scl.reshape(-1)


def _pattern(kind, n, seed=0):
    i = np.arange(n)
    if kind == "empty":
        return np.zeros(n, dtype=bool)
    if kind == "full":
        return np.ones(n, dtype=bool)
    if kind == "first and last":
        return (i == 0) | (i == n - 1)
    if kind == "every 64th word zero":      # whole waves out of scope between waves in scope
        return (i >> 5) % 64 != 0
    if kind == "last word partial":         # the bits of the last word that name a splat, and nothing else
        return i >= (n - 1) // 32 * 32
    return np.random.default_rng(99 + n + seed).random(n) < 0.01


def _load(r, scene, sel=None, hid=None):
    r.set_scene_arrays(*scene)
    n = scene[1].size // 3
    sw = hw = None
    if sel is not None:
        r.set_selection(sel)
        sw = ar.pack(sel)
    if hid is not None:
        r.set_hidden(hid)
        hw = ar.pack(hid)
    return n, sw, hw


def _values(attr, scene, contrib=None):
    data, pos, _, scl = scene
    return ar.attr_value(attr, data=data, positions=pos, scales=scl, origin=ORIGIN, contrib=contrib)


def _check_stats(r, attr, v, scope, mask, what):
    got = r.attr_stats(attr, origin=ORIGIN, selected=bool(scope & 1), visible=bool(scope & 2))
    want = ar.stats(v, mask)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3] == want[3], (what, got, want)
    return got


def _check_hist(r, attr, v, lo, hi, bins, scope, mask, what):
    counts, outside, edges = r.attr_histogram(attr, lo, hi, bins, origin=ORIGIN, selected=bool(scope & 1), visible=bool(scope & 2))
    wc, wo = ar.histogram(v, lo, hi, bins, mask)
    assert np.array_equal(edges, ar.edges(lo, hi, bins)), what
    assert counts.dtype == np.uint32 and np.array_equal(counts, wc), (what, np.nonzero(counts != wc)[0][:8])
    assert tuple(outside) == wo, (what, outside, wo)
    return counts, outside, edges


def _check_select(r, attr, v, lo, hi, what, op="replace", prior=None):
    got = r.select_attr(attr, lo, hi, origin=ORIGIN, op=op)
    want = ar.select(v, lo, hi)
    if prior is not None:
        want = ar.fold(prior, want, {"replace": 0, "add": 1, "subtract": 2, "intersect": 3}[op])
    assert got == int(want.sum()) == r.selection_count(), (what, got, int(want.sum()))
    assert np.array_equal(r.selection_words(), ar.pack(want)), what
    return want


@pytest.mark.parametrize("n", SIZES)
def test_every_attribute_in_every_scope(r, n):
    scene = _scene(n)
    sel, hid = _pattern("random 1 %", n) | (np.arange(n) % 5 == 0), np.arange(n) % 3 == 1
    n, sw, hw = _load(r, scene, sel, hid)
    for k, attr in enumerate(SCENE_ATTRS):
        v = _values(attr, scene)
        lo, hi = RANGES[attr]
        for scope in SCOPES:
            mask = ar.in_scope(n, scope, sw, hw)
            what = "n %d %s scope %d" % (n, attr, scope)
            count = _check_stats(r, attr, v, scope, mask, what)[0]
            bins = BINS[(k + scope) % len(BINS)]
            counts, outside, _ = _check_hist(r, attr, v, lo, hi, bins, scope, mask, what + " bins %d" % bins)
            assert int(counts.sum()) + sum(outside) == count, what
    # (the selection is still the one the scopes read: no call above changed it)
    assert np.array_equal(r.selection_words(), sw) and np.array_equal(r.hidden_words(), hw)
    for attr in SCENE_ATTRS:
        _check_select(r, attr, _values(attr, scene), *RANGES[attr], "n %d select %s" % (n, attr))
    assert np.array_equal(r.hidden_words(), hw)


@pytest.mark.parametrize("bins", BINS)
def test_every_bin_count_at_two_sizes(r, bins):
    for n in (257, 1000):
        scene = _scene(n, seed=5)
        _load(r, scene)
        for attr in ("y", "opacity", "scale_max", "distance"):
            _check_hist(r, attr, _values(attr, scene), *RANGES[attr], bins, 0, None, "n %d %s bins %d" % (n, attr, bins))


@pytest.mark.parametrize("kind", PATTERNS)
def test_set_patterns(r, kind):
    for n in (1000, 64 * 32 * 3 + 17):     # the second: more than one run of 64 words, a partial last word
        scene = _scene(n, seed=7)
        for which in ("selection", "hidden", "both"):
            sel = _pattern(kind, n) if which != "hidden" else None
            hid = _pattern(kind, n, seed=1) if which != "selection" else None
            _, sw, hw = _load(r, scene, sel, hid)
            for scope in SCOPES:
                mask = ar.in_scope(n, scope, sw, hw)
                for attr in ("opacity", "scale_max", "x"):
                    what = "%s as %s, n %d %s scope %d" % (kind, which, n, attr, scope)
                    v = _values(attr, scene)
                    _check_stats(r, attr, v, scope, mask, what)
                    _check_hist(r, attr, v, *RANGES[attr], 64, scope, mask, what)


def test_a_scene_never_selected_in_and_an_empty_scene(r):
    scene = _scene(300)
    _load(r, scene)
    v = _values("opacity", scene)
    assert r.attr_stats("opacity", selected=True) == (0, 0, np.inf, -np.inf)
    assert r.attr_stats("opacity", visible=True) == ar.stats(v)
    counts, outside, _ = r.attr_histogram("opacity", 0, 256, 16, selected=True)
    assert not counts.any() and outside == (0, 0, 0)
    r.set_scene_arrays(*[a[:0] for a in scene])
    assert r.attr_stats("x") == (0, 0, np.inf, -np.inf)
    counts, outside, _ = r.attr_histogram("x", 0, 1, 7)
    assert counts.size == 7 and not counts.any() and outside == (0, 0, 0)
    assert r.select_attr("x", 0, 1) == 0


def _edge_scene(n, attr_axis, lo, hi, bins, seed=11):
    """positions whose `attr_axis` component holds, for every edge, the f32 values around it: the edge rounded to f32 and its two
    f32 neighbours (an edge that is an f32 is hit exactly, with one f32 ulp to either side)"""
    data, pos, rot, scl = _scene(n, seed, plant=False)
    e = ar.edges(lo, hi, bins).astype(np.float32)
    planted = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))])
    assert planted.size <= n
    p = pos.reshape(-1, 3)
    p[:planted.size, attr_axis] = planted
    d = data.reshape(-1, 8)
    d[:, 0:3] = p.view(np.uint32)
    return d.reshape(-1), p.reshape(-1), rot, scl


@pytest.mark.parametrize("lo,hi,bins", ((0.0, 1.0, 64), (0.0, 1.0, 4096), (-2.0, 2.0, 256), (0.1, 1.3, 257), (0.1, 1.3, 7), (-3.7, 11.9, 4096), (0.25, 0.75, 2)))
def test_values_on_the_edges_and_beside_them(r, lo, hi, bins):
    n = 3 * (bins + 1) + 500
    scene = _edge_scene(n, 0, lo, hi, bins)
    _load(r, scene)
    v = _values("x", scene)
    e = ar.edges(lo, hi, bins)
    if (lo, hi) == (0.0, 1.0) or (lo, hi) == (-2.0, 2.0):
        assert np.isin(e, v).all()               # dyadic edges are f32s: every edge itself is a value of the scene
    counts, _, edges = _check_hist(r, "x", v, lo, hi, bins, 0, None, "edges %r" % ((lo, hi, bins),))
    # what the histogram shows is what the range selects, through the device
    rng = np.random.default_rng(bins)
    pairs = {(0, bins), (0, 1), (bins - 1, bins)} | {tuple(sorted(rng.choice(bins + 1, 2, replace=False))) for _ in range(5)}
    for a, b in sorted(pairs):
        assert r.select_attr("x", edges[a], edges[b]) == int(counts[a:b].sum()), (lo, hi, bins, a, b)
        assert np.array_equal(r.selection_words(), ar.pack(ar.select(v, edges[a], edges[b])))


def test_every_splat_in_one_bin_and_every_splat_outside(r):
    n = 70001
    data, pos, rot, scl = _scene(n, plant=False)
    data.reshape(-1, 8)[:, 7] |= np.uint32(0xff000000)      # opacity 255 everywhere: every lane of every wave meets in one counter
    scl[:] = np.float32(0.5)
    scene = (data, pos, rot, scl)
    hid = np.arange(n) % 7 == 0
    _, _, hw = _load(r, scene, None, hid)
    for scope in (0, 2):
        mask = ar.in_scope(n, scope, None, hw)
        for attr, lo, hi in (("opacity", 0.0, 256.0), ("scale_max", 0.0, 1.0), ("scale_min", 0.5, 0.75)):
            v = _values(attr, scene)
            for bins in (1, 256, 4096):
                counts, outside, _ = _check_hist(r, attr, v, lo, hi, bins, scope, mask, "one bin: %s %d" % (attr, bins))
                assert counts.max() == int(mask.sum()) and outside == (0, 0, 0)
        for lo, hi, where in ((300.0, 400.0, 0), (-5.0, 255.0, 1)):
            counts, outside, _ = _check_hist(r, "opacity", _values("opacity", scene), lo, hi, 64, scope, mask, "all outside")
            assert not counts.any() and outside[where] == int(mask.sum())
    nan_pos = pos.copy()
    nan_pos[0::3] = np.nan
    data.reshape(-1, 8)[:, 0] = nan_pos[0::3].view(np.uint32)
    _load(r, (data, nan_pos, rot, scl))
    assert r.attr_stats("x") == (n, n, np.inf, -np.inf) and r.attr_stats("distance", origin=ORIGIN)[1] == n
    counts, outside, _ = r.attr_histogram("x", 0, 1, 64)
    assert not counts.any() and outside == (0, 0, n)
    assert r.select_attr("x") == 0                            # NaN is never picked, whatever the bounds


def test_distance_is_the_correctly_rounded_f64_expression(r):
    n = 5000
    scene = _scene(n, seed=13, plant=False)
    _load(r, scene)
    p = scene[1].reshape(-1, 3).astype(np.float64)
    dx = p[:, 0] - ORIGIN[0]
    v = _values("distance", scene)
    from fractions import Fraction
    assert any(Fraction(float(d)) ** 2 != Fraction(float(d * d)) for d in dx[:16]), "no dx * dx rounds: the origin does not test the order of operations"
    got = _check_stats(r, "distance", v, 0, None, "distance")
    assert got[2] == v.min() and got[3] == v.max()
    # every value, not only the extremes: the range [v_i, nextafter(v_i)) selects exactly the splats whose distance is v_i bit for bit
    for i in np.random.default_rng(1).choice(n, 24, replace=False):
        want = v == v[i]
        assert r.select_attr("distance", v[i], np.nextafter(v[i], np.inf), origin=ORIGIN) == int(want.sum())
        assert np.array_equal(r.selection_words(), ar.pack(want))
    # and all of them at once: a histogram whose bins are far finer than the values' spacing, compared with the reference bin by bin
    _check_hist(r, "distance", v, 0.3, 3.1, 4096, 0, None, "distance")
    other = (1e6 + 0.1, -1e6, 3.0)
    w = ar.attr_value("distance", positions=scene[1], origin=other)
    got = r.attr_stats("distance", origin=other)
    assert got == ar.stats(w)


def test_all_four_ops_against_a_prior_selection(r):
    n = 1000
    scene = _scene(n)
    v = _values("y", scene)
    prior = _pattern("every 64th word zero", n) & (np.arange(n) % 2 == 0)
    for op in ("replace", "add", "subtract", "intersect"):
        for lo, hi in ((-np.inf, 0.4), (0.4, np.inf), (-np.inf, np.inf), (0.4, 0.4)):
            _load(r, scene, prior)
            _check_select(r, "y", v, lo, hi, "%s [%g, %g)" % (op, lo, hi), op=op, prior=prior)


def test_refusals_leave_the_selection_alone(gh, r):
    n = 500
    scene = _scene(n)
    sel = _pattern("every 64th word zero", n)
    _, sw, _ = _load(r, scene, sel)
    L, ctx, u32 = r._L, r._ctx, ctypes.c_uint32
    o = (ctypes.c_double * 3)(*ORIGIN)
    bad = (ctypes.c_double * 3)(0.0, np.inf, 0.0)
    nan = (ctypes.c_double * 3)(np.nan, 0.0, 0.0)
    counts, outside, cnt = (u32 * 4099)(), (u32 * 3)(), u32(77)

    def refused(rc, what):
        assert rc == GSR_ERR_ARG, (what, rc)
        assert L.gsr_last_error(ctx), what
        assert r.selection_count() == int(sel.sum()) and np.array_equal(r.selection_words(), sw), what

    for code in (-1, 16, 1000):
        refused(L.gsr_attr_stats(ctx, code, o, 0, None, None, None, None), "stats attr %d" % code)
        refused(L.gsr_attr_histogram(ctx, code, o, 0, 0.0, 1.0, 8, counts, outside), "histogram attr %d" % code)
        refused(L.gsr_select_attr(ctx, code, o, 0.0, 1.0, 0, ctypes.byref(cnt)), "select attr %d" % code)
    for org, what in ((None, "NULL origin"), (bad, "inf origin"), (nan, "NaN origin")):
        refused(L.gsr_attr_stats(ctx, 3, org, 0, None, None, None, None), what)
        refused(L.gsr_attr_histogram(ctx, 3, org, 0, 0.0, 1.0, 8, counts, outside), what)
        refused(L.gsr_select_attr(ctx, 3, org, 0.0, 1.0, 0, ctypes.byref(cnt)), what)
    assert r.attr_stats("x", origin=None)[0] == n and L.gsr_attr_stats(ctx, 0, bad, 0, None, None, None, None) == 0   # origin is ignored elsewhere
    for stat in ("contrib_weight", "contrib_peak", "contrib_pixels"):                                               # never reset
        refused(L.gsr_attr_stats(ctx, ar.ATTRS[stat], None, 0, None, None, None, None), stat)
        refused(L.gsr_select_attr(ctx, ar.ATTRS[stat], None, 0.0, 1.0, 0, ctypes.byref(cnt)), stat)
    for bins, lo, hi, what in ((0, 0.0, 1.0, "bins 0"), (4097, 0.0, 1.0, "bins 4097"), (8, 1.0, 1.0, "lo == hi"), (8, 2.0, 1.0, "lo > hi"),
                               (8, -np.inf, 1.0, "lo -inf"), (8, 0.0, np.inf, "hi inf"), (8, np.nan, 1.0, "lo NaN"), (8, -1e308, 1e308, "hi - lo overflows")):
        refused(L.gsr_attr_histogram(ctx, 0, None, 0, lo, hi, bins, counts, outside), what)
    for lo, hi, op, what in ((np.nan, 1.0, 0, "lo NaN"), (0.0, np.nan, 0, "hi NaN"), (2.0, 1.0, 0, "lo > hi"), (0.0, 1.0, 4, "op 4"), (0.0, 1.0, -1, "op -1")):
        refused(L.gsr_select_attr(ctx, 0, None, lo, hi, op, ctypes.byref(cnt)), what)
    refused(L.gsr_attr_stats(ctx, 0, None, 4, None, None, None, None), "scope 4")
    assert cnt.value == 77
    # frames == 0: accumulators exist, no pass has contributed
    r.contrib_reset()
    for stat in ("contrib_weight", "contrib_peak", "contrib_pixels"):
        refused(L.gsr_attr_histogram(ctx, ar.ATTRS[stat], None, 0, 0.0, 1.0, 8, counts, outside), stat + ", frames == 0")
        refused(L.gsr_select_attr(ctx, ar.ATTRS[stat], None, 0.0, 1.0, 0, ctypes.byref(cnt)), stat + ", frames == 0")
    # a scene without rotations / scales: the scale attributes are refused as gsr_scene_scale_selected refuses, the others work
    r.set_raw_scene(scene[0], scene[1])
    r.set_selection(sel)
    for attr in ("scale_x", "scale_y", "scale_z", "scale_min", "scale_max"):
        refused(L.gsr_attr_stats(ctx, ar.ATTRS[attr], None, 0, None, None, None, None), attr)
        refused(L.gsr_attr_histogram(ctx, ar.ATTRS[attr], None, 0, 0.0, 1.0, 8, counts, outside), attr)
        refused(L.gsr_select_attr(ctx, ar.ATTRS[attr], None, 0.0, 1.0, 0, ctypes.byref(cnt)), attr)
    assert r.attr_stats("opacity") == ar.stats(_values("opacity", scene))
    with pytest.raises(ValueError):
        r.attr_stats("mass")


def _tour(gh, x, poses=(3, 40)):
    x.contrib_reset()
    for k in poses:
        x.set_camera(gh.orbit_camera(k, width=W, height=H, fx=gh.synth.CONFIGS["C1"]["fx"] * W / 640))
        x.render_async()
        x.sync()
        x.contrib_accumulate()
    return x.read_contrib()


def test_contribution_attributes_after_a_tour(gh, scenes):
    x = gh.HIPRenderer(W, H)
    try:
        rows = scenes(3000, 21)[0]
        x.set_scene_rows(rows)
        weight, peak, pixels, frames = _tour(gh, x)
        assert frames == 2 and pixels.any()
        contrib = (weight, peak, pixels)
        for stat, t in (("weight", 0.75), ("peak", 0.05), ("pixels", 3.0), ("pixels", 1.0)):
            attr = "contrib_" + stat
            v = ar.attr_value(attr, contrib=contrib)
            count = x.select_contrib(stat, below=t)
            words = x.selection_words()
            x.set_selection(None)
            assert x.select_attr(attr, hi=t) == count == int((v < t).sum())
            assert np.array_equal(x.selection_words(), words), stat          # bit for bit what gsr_select_contrib picks
            assert x.attr_stats(attr) == ar.stats(v)
            hi = float(v.max()) + 1.0
            for bins in (1, 64, 4096):
                _check_hist(x, attr, v, 0.0, hi, bins, 0, None, "%s bins %d" % (attr, bins))
        # pixels == 0 for most of a scene after a short tour on a small frame: the one-counter case on real data
        counts, outside, _ = x.attr_histogram("contrib_pixels", 0, 4096, 4096)
        assert counts[0] == int((pixels == 0).sum())
    finally:
        x.dispose()


def test_either_member_of_a_shared_scene_and_a_frame_in_flight(gh, scenes):
    a, b = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    try:
        a.set_scene_rows(scenes(3000, 21)[0])
        b.share_scene(a)
        n = a.scene_count()
        sel = _pattern("every 64th word zero", n)
        a.set_selection(sel)
        b.set_hidden(np.arange(n) % 4 == 0)
        cam = gh.orbit_camera(3, width=W, height=H, fx=gh.synth.CONFIGS["C1"]["fx"] * W / 640)
        b.set_camera(cam)
        b.render_async()
        b.sync()
        frame = b.readPixelsFloat().copy()
        scene = a.read_scene()
        b.render_async()                     # in flight on b while a asks
        got = {}
        for m in (a, b):
            got[m] = [(m.attr_stats(attr, origin=ORIGIN, selected=s, visible=v), m.attr_histogram(attr, *RANGES[attr], 64, origin=ORIGIN, selected=s, visible=v)[:2])
                      for attr in ("opacity", "distance", "scale_min") for s in (False, True) for v in (False, True)]
        for (sa, ha), (sb, hb) in zip(got[a], got[b]):
            assert sa == sb and np.array_equal(ha[0], hb[0]) and ha[1] == hb[1]
        k = 0
        for attr in ("opacity", "distance", "scale_min"):
            v = _values(attr, scene)
            for s in (False, True):
                for vis in (False, True):
                    mask = ar.in_scope(n, s | 2 * vis, a.selection_words(), a.hidden_words())
                    assert got[a][k][0] == ar.stats(v, mask), (attr, s, vis)
                    wc, wo = ar.histogram(v, *RANGES[attr], 64, mask)
                    assert np.array_equal(got[a][k][1][0], wc) and got[a][k][1][1] == wo
                    k += 1
        assert b.select_attr("opacity", 0, 128) == a.selection_count() == int(ar.select(_values("opacity", scene), 0, 128).sum())
        b.sync()
        assert np.array_equal(b.readPixelsFloat(), frame)    # the frame that was in flight is the frame it would have been
    finally:
        b.dispose()
        a.dispose()


def test_the_histogram_describes_the_rows_after_duplicate_and_erase(r):
    n = 777
    scene = _scene(n, seed=17)
    sel = np.arange(n) % 6 == 1
    _load(r, scene, sel)
    first, count = r.scene_duplicate_selected()
    assert (first, count) == (n, int(sel.sum())) and r.scene_count() == n + count
    for step in ("duplicate", "erase"):
        if step == "erase":
            r.select_attr("opacity", 0, 100)
            r.scene_erase_selected()
        now = r.read_scene()
        m = now[1].size // 3
        assert m == r.scene_count()
        for attr in ("opacity", "scale_max", "z", "distance"):
            v = _values(attr, now)
            assert r.attr_stats(attr, origin=ORIGIN) == ar.stats(v), (step, attr)
            _check_hist(r, attr, v, *RANGES[attr], 257, 0, None, "%s %s" % (step, attr))
            mask = ar.in_scope(m, 1, r.selection_words(), None)
            _check_hist(r, attr, v, *RANGES[attr], 64, 1, mask, "%s %s selected" % (step, attr))
    assert (_values("opacity", r.read_scene()) >= 100).all()


def test_bounds_twin_counts_nothing(gh):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    x = gh.HIPRenderer(W, H, lib_path=BOUNDS_LIB)
    try:
        for n in (1, 33, 65, 257, 1000, BIG):
            scene = _scene(n)
            sel, hid = _pattern("every 64th word zero", n), np.arange(n) % 3 == 1
            _, sw, hw = _load(x, scene, sel, hid)
            for attr in ("x", "distance", "opacity", "scale_max"):
                v = _values(attr, scene)
                for scope in SCOPES:
                    mask = ar.in_scope(n, scope, sw, hw)
                    _check_stats(x, attr, v, scope, mask, "bounds twin")
                    _check_hist(x, attr, v, *RANGES[attr], (1, 257, 4096, 64)[scope], scope, mask, "bounds twin")
                _check_select(x, attr, v, *RANGES[attr], "bounds twin")
                x.set_selection(sel)
        buf = (ctypes.c_uint32 * 8)()
        assert L.gsr_debug_bounds_attr(buf) == 0
        assert list(buf) == [0] * 8
    finally:
        x.dispose()

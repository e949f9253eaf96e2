"""Hidden splats on the GPU (gsr_hidden.cpp, k_project_key's test of the hidden bit, k_box_compact_bits) against
tests/hide_reference.py: the masks word for word, and the hidden FRAME against every specification the project already has, fed
with the oracle's boxes made invisible at the members of H (hide_bbox) and the unchanged depth order -- never with anything the
device wrote.  H is a seeded random half of C1 united with the splats inside tests/test_gpu_select.py's BOX; that it removes
between a quarter and three quarters of the listed splats, empties whole bins and mixes others is asserted on the CPU
(tests/test_hide_reference.py) and again here.

How the depth reference is applied: as tests/test_gpu_depth.py applies it -- the index plane equal outside the reference's knife-edge
mask, hit the bits of z[index], mean (an f64 sum in the reference) within that file's tolerance."""
import ctypes
import os

import numpy as np
import pytest

import bin_reference as B
import blend_reference as BR
import contrib_reference as CR
import depth_reference as DR
import hide_reference as HR
import overlay_reference as OR
import select_reference as SR
import sh_follow_reference as SF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
KNOBS = ("GSR_BIN_TWO_LEVEL", "GSR_LONG_ITEMS", "GSR_DEPTH_SKIP", "GSR_NO_GRAPH")
GSR_ERR_ARG = -1
NONE = 0xFFFFFFFF
NAME, POSES = "C1", (3, 40)
W, H = 640, 480
TINY = (1, 31, 32, 33, 1023, 1024, 1025)          # word, wave and BOX_THREADS block edges
BOX = (-1.0, 2.5, -0.75, 3.0, -2.0, 1.0)          # tests/test_gpu_select.py's: about half of C1
SEED = 5                                          # fixed by tests/test_hide_reference.py
RECT = (200, 150, 330, 270)
BAND = (192, 416)                                 # starts at bin column 6, inside the image: the projection's pack path
TINT, MIX = (1.0, 0.5, 0.0), 0.5
KINDS = {"default": {}, "throughput": {"throughput": True}, "two level": {"env": {"GSR_BIN_TWO_LEVEL": "1"}}, "band": {"band": BAND}}


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    cfg = gsplat_hip.synth.CONFIGS[NAME]
    assert (cfg["width"], cfg["height"]) == (W, H) and cfg["n"] % 32 == 16
    return gsplat_hip


def _cam(gh, k):
    return gh.orbit_camera(k, width=W, height=H, fx=gh.synth.CONFIGS[NAME]["fx"])


class C1:
    """the oracle's views of C1 at both poses, H, the hidden boxes, and the references of the hidden frame: computed once, shared, never changed"""

    def __init__(self, oracle, scenes, gh):
        self.oracle, self.gh = oracle, gh
        self.rows, self.data, self.pos = scenes(NAME)
        self.n = gh.synth.CONFIGS[NAME]["n"]
        self.H = HR.test_set(self.n, self.pos, BOX, SEED)
        self.H.flags.writeable = False
        self.views, self._cache = {}, {}
        for k in POSES:
            cam = _cam(gh, k)
            v, p, vp = cam.f32()
            rec, bbox, raw = oracle.project(self.data, v, p, cam.fx, cam.fy, W, H)
            order = oracle.sort(vp, self.pos)[0]
            hb = HR.hide_bbox(bbox, self.H)
            for a in (rec, bbox, raw, order, hb):
                a.flags.writeable = False
            self.views[k] = {"rec": rec, "bbox": bbox, "raw": raw, "order": order, "hbbox": hb}
            listed = SR.listed(bbox)
            gone = int((listed & self.H).sum())
            assert 0.25 * listed.sum() <= gone <= 0.75 * listed.sum(), (k, gone, int(listed.sum()))   # neither side is vacuous

    def ref(self, what, k):
        if (what, k) not in self._cache:
            v = self.views[k]
            if what == "blend":
                out = BR.blend_reference(v["rec"], v["hbbox"], v["raw"], v["order"], W, H)
            elif what == "depth":
                out = DR.depth_planes_reference(v["rec"], v["hbbox"], np.ascontiguousarray(v["raw"][:, 10]), v["order"], W, H, None, 0.5)
            elif what == "contrib":
                out = CR.contrib_reference([(v["rec"], v["hbbox"], v["order"], W, H)], self.n)
            else:
                sel = self.H | SR.centre_pick(v["rec"], v["bbox"], RECT)
                out = (sel, OR.overlay_reference(v["rec"], v["hbbox"], v["raw"], v["order"], sel, W, H))
            self._cache[(what, k)] = out
        return self._cache[(what, k)]


@pytest.fixture(scope="module")
def c1(oracle, scenes, gh):
    return C1(oracle, scenes, gh)


def _context(gh, monkeypatch, scenes, env=None, name=NAME, seed=None, rows=True, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    r = gh.HIPRenderer(W, H, **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)
    if rows:
        r.set_scene_rows(scenes(name, seed)[0])
    return r


def _frame(gh, r, k):
    r.set_camera(_cam(gh, k))
    r.render_async()
    r.sync()
    assert r.stats()["overflow_frames"] == 0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _words_are(words, want, what):
    ref = HR.pack(want)
    assert words.dtype == np.uint32 and words.shape == ref.shape, what
    bad = np.nonzero(words != ref)[0]
    assert not bad.size, (what, bad[:4].tolist(), [hex(int(v)) for v in words[bad[:4]]], [hex(int(v)) for v in ref[bad[:4]]])


def _hidden_is(r, want, what):
    """the device's hidden set is `want` (bool[n]): word for word (the tail included), and the count"""
    _words_are(r.hidden_words(), want, what)
    assert r.hidden_count() == int(np.sum(want)), what
    assert np.array_equal(r.hidden(), want), what


def _selection_is(r, want, what):
    _words_are(r.selection_words(), want, what)
    assert r.selection_count() == int(np.sum(want)), what


def _bounds_zero(r, what):
    for name in ("gsr_debug_bounds_scene", "gsr_debug_bounds_scene_sh", "gsr_debug_bounds_select", "gsr_debug_bounds_bin", "gsr_debug_bounds_sort",
                 "gsr_debug_bounds_blend"):
        buf = (ctypes.c_uint32 * 8)()
        assert getattr(r._L, name)(buf) == 0
        assert not any(buf), (what, name, list(buf))


# 1 masks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [NAME] + list(TINY), ids=str)
def test_masks_against_numpy(gh, monkeypatch, scenes, count):
    r = _context(gh, monkeypatch, scenes, name=count, seed=None if count == NAME else 7)
    n = r.scene_count()
    nw = -(-n // 32)
    rng = np.random.default_rng(n + 100)
    bytes0 = r.scene_sharing()[1]
    assert r.hidden_count() == 0 and not r.hidden().any() and r.hidden().shape == (n,) and r.hidden_words().shape == (nw,)   # never hid: all zeros
    assert r.scene_sharing()[1] == bytes0                     # ... and reading allocates nothing
    Hs = np.zeros(n, bool)
    for step, op in enumerate(("replace", "add", "subtract", "intersect", "add", "replace")):      # gsr_hidden_set
        P = rng.random(n) < (0.5, 0.2, 0.3, 0.7, 0.1, 0.4)[step]
        Hs = HR.hidden_set(Hs, P, op)
        assert r.set_hidden(P, op=op) == int(Hs.sum())
        _hidden_is(r, Hs, (n, "set", step, op))
    _selection_is(r, np.zeros(n, bool), (n, "the selection is untouched"))
    for step, op in enumerate(("add", "subtract", "intersect", "replace")):                        # gsr_hide_selected
        S = rng.random(n) < (0.3, 0.4, 0.6, 0.5)[step]
        r.set_selection(S)
        Hs = HR.hide_selected(Hs, S, op)
        assert r.hide_selected(op=op) == int(Hs.sum())
        _hidden_is(r, Hs, (n, "hide", op))
        _selection_is(r, S, (n, "hide leaves the selection", op))
    assert r.hide_selected() == int((Hs | S).sum())           # the default op hides
    Hs = Hs | S
    for step, op in enumerate(("replace", "add", "subtract", "intersect")):                        # gsr_select_hidden
        S = rng.random(n) < 0.5
        r.set_selection(S)
        S = HR.select_hidden(S, Hs, op)
        assert r.select_hidden(op=op) == int(S.sum())
        _selection_is(r, S, (n, "select hidden", op))
        _hidden_is(r, Hs, (n, "select hidden leaves H", op))
    ones = np.full(nw + 3, 0xFFFFFFFF, dtype=np.uint32)       # more words than needed, every bit set: bits at and above n are dropped
    assert r.set_hidden(words=ones, op="intersect") == int(Hs.sum())
    _hidden_is(r, Hs, (n, "intersect with everything"))
    assert r.set_hidden(words=ones) == n
    _hidden_is(r, np.ones(n, bool), (n, "all ones"))
    assert r.set_hidden(None, op="intersect") == 0            # NULL words: the empty set
    _hidden_is(r, np.zeros(n, bool), (n, "intersect with nothing"))
    Hs = rng.random(n) < 0.5
    r.set_hidden(Hs)
    # refusals change nothing
    S = r.selection()
    L, ctx = r._L, r._ctx
    words = np.zeros(nw, np.uint32)
    out = ctypes.c_uint32(12345)
    for op in (4, -1):
        assert L.gsr_hide_selected(ctx, op, ctypes.byref(out)) == GSR_ERR_ARG and b"op" in L.gsr_last_error(ctx)
        assert L.gsr_hidden_set(ctx, words.ctypes.data, nw, op, ctypes.byref(out)) == GSR_ERR_ARG and b"op" in L.gsr_last_error(ctx)
        assert L.gsr_select_hidden(ctx, op, ctypes.byref(out)) == GSR_ERR_ARG and b"op" in L.gsr_last_error(ctx)
    assert L.gsr_hidden_set(ctx, words.ctypes.data, nw - 1, 0, ctypes.byref(out)) == GSR_ERR_ARG and b"nwords" in L.gsr_last_error(ctx)
    assert L.gsr_read_hidden(ctx, words.ctypes.data, nw - 1, ctypes.byref(out)) == GSR_ERR_ARG and b"nwords" in L.gsr_last_error(ctx)
    for call in (lambda: L.gsr_hide_selected(None, 1, None), lambda: L.gsr_hidden_set(None, None, 0, 0, None), lambda: L.gsr_read_hidden(None, None, 0, None),
                 lambda: L.gsr_select_hidden(None, 0, None)):
        assert call() == GSR_ERR_ARG
    assert out.value == 12345 and not words.any()
    _hidden_is(r, Hs, (n, "after every refusal"))
    _selection_is(r, S, (n, "after every refusal"))
    assert L.gsr_read_hidden(ctx, None, 0, None) == 0         # every output may be NULL
    r.dispose()


# 2 lists -------------------------------------------------------------------------------------------------------------
def _lists_equal_the_reference(gh, r, c1, band, what, records=False):
    for k in POSES:
        v = c1.views[k]
        r.set_hidden(None)
        _frame(gh, r, k)
        s0, l0 = r.bin_lists()
        full = B.bin_lists_reference(v["bbox"], v["order"], W, H, band)
        assert B.first_difference(s0, l0, full[0], full[1], v["bbox"]) is None, (what, k, "the unhidden frame")
        bb0 = r.read_records()[1] if records else None
        di0 = r.lastDepthIndex()
        assert r.set_hidden(c1.H) == int(c1.H.sum())
        _frame(gh, r, k)
        starts, lst = r.bin_lists()
        want = B.bin_lists_reference(v["hbbox"], v["order"], W, H, band)
        diff = B.first_difference(starts, lst, want[0], want[1], v["hbbox"])
        assert diff is None, (what, k, diff)
        filt = HR.filter_lists(s0, l0, c1.H)
        assert np.array_equal(starts, filt[0]) and np.array_equal(lst, filt[1]), (what, k, "not the unhidden lists filtered by H")
        assert 0 < lst.size < l0.size and not c1.H[lst].any(), (what, k)
        assert np.array_equal(r.bin_totals().reshape(-1), np.diff(want[0].astype(np.int64))), (what, k)
        st = r.stats()
        print("hide lists", what, k, "entries", l0.size, "->", lst.size, "visible", st["visible"], "tiles", st["tile_entries"])
        assert st["bin_entries"] == int(want[0][-1]), (what, k, st["bin_entries"])
        assert st["visible"] == B.visible_reference(v["hbbox"], W, H, band), (what, k, st["visible"])
        assert st["tile_entries"] == HR.tile_entries(v["hbbox"], W, H, band), (what, k, st["tile_entries"])
        assert not r.overflow_pending() and st["dropped_frames"] == 0, (what, k)
        if records:                                           # a hidden splat reads as a culled one
            bb = r.read_records()[1]
            assert (bb[c1.H, 0] > bb[c1.H, 2]).all() and np.array_equal(bb, HR.hide_bbox(bb0, c1.H)), (what, k)
            assert np.array_equal(SR.listed(bb), SR.listed(v["hbbox"])), (what, k)
        di = r.lastDepthIndex()                               # still sorted: bit for bit the unhidden frame's order, the oracle's
        assert np.array_equal(di, di0) and np.array_equal(di, v["order"]), (what, k, "depthIndex")


@pytest.mark.parametrize("kind", list(KINDS))
def test_lists_equal_the_reference(gh, monkeypatch, scenes, c1, kind):
    r = _context(gh, monkeypatch, scenes, **KINDS[kind])
    _lists_equal_the_reference(gh, r, c1, KINDS[kind].get("band"), kind, records=kind == "default")
    r.dispose()


# 3 colour ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "throughput"])
def test_colour_within_the_derived_bound(gh, monkeypatch, scenes, c1, kind):
    r = _context(gh, monkeypatch, scenes, **KINDS[kind])
    r.set_hidden(c1.H)
    for k in POSES:
        _frame(gh, r, k)
        ref = c1.ref("blend", k)
        got = r.readPixelsFloat().astype(np.float64)
        lit, kept = got[..., 3] > 0.0, ref["kept"] > 0
        assert np.array_equal(lit, kept), (kind, k, "covered pixels differ", int((lit != kept).sum()), np.argwhere(lit != kept)[:4].tolist())
        ratio = np.abs(got - ref["rgba"]) / ref["bound"]
        print("hide colour", kind, k, "max |gpu - ref| / bound %.3f" % float(ratio.max()), "covered", int(kept.sum()))
        assert not (ratio > 1.0).any(), (kind, k, int((ratio > 1.0).sum()), float(ratio.max()), np.argwhere(ratio > 1.0)[:4].tolist())
        assert 0 < kept.sum() < W * H
    r.dispose()


# 4 downstream passes see through -------------------------------------------------------------------------------------
def test_downstream_passes_see_through(gh, monkeypatch, scenes, c1):
    r = _context(gh, monkeypatch, scenes)
    r.set_hidden(c1.H)
    r.set_overlay(TINT, MIX)
    n = c1.n
    for k in POSES:
        v = c1.views[k]
        _frame(gh, r, k)
        # depth planes
        mean, hit, index = r.read_depth()
        pl = c1.ref("depth", k)
        z = np.ascontiguousarray(v["raw"][:, 10])
        ok = ~pl["mask"]
        assert pl["mask"].mean() < 0.01 and (pl["index"] != NONE).any()
        bad = ok & (index != pl["index"])
        assert not bad.any(), (k, "index plane", int(bad.sum()), np.argwhere(bad)[:4].tolist())
        some = index != NONE
        assert not c1.H[index[some]].any(), (k, "the index plane names a hidden splat")
        assert np.array_equal(_bits(hit[some]), _bits(z[index[some]])) and np.all(np.isinf(hit[~some])), (k, "hit is not z of index, bit for bit")
        vis = SR.listed(v["hbbox"])
        err = np.abs(mean.astype(np.float64) - pl["mean"])[ok].max()
        assert err <= 2e-4 * max(1.0, float(z[vis].max())), (k, err)
        pk = r.pick([(320, 240), (317, 243), (100, 100)])
        assert np.array_equal(pk["index"], index[[240, 243, 100], [320, 317, 100]])
        # select_region, both modes
        drect, dmask = SR.disc(317, 243, 70)
        for rid, rect, mask in (("rect", RECT, None), ("disc", drect, dmask), ("whole", (0, 0, W, H), None)):
            want = SR.centre_pick(v["rec"], v["hbbox"], rect, mask)
            assert r.select_region(rect, mask, mode="centre") == int(want.sum()) > 0
            _selection_is(r, want, (k, "centre", rid))
            want = SR.hit_pick(index, n, rect, mask)
            assert r.select_region(rect, mask, mode="hit") == int(want.sum()) > 0
            _selection_is(r, want, (k, "hit", rid))
            assert not (want & c1.H).any()
        # one contribution pass
        r.contrib_reset()
        r.contrib_accumulate()
        got = r.read_contrib()
        weight, peak, pixels = got[:3]
        assert not weight[c1.H].any() and not pixels[c1.H].any() and not _bits(peak[c1.H]).any(), (k, "a hidden splat contributed")
        ref = c1.ref("contrib", k)
        bad = np.nonzero(pixels != ref["pixels"])[0]
        assert not bad.size, (k, "pixels", bad[:4].tolist())
        ratios = CR.excess(got, ref)
        print("hide contrib", k, "max |gpu - ref| / bound: weight %.3f peak %.3f" % ratios)
        assert ratios[0] <= 1.0 and ratios[1] <= 1.0 and pixels.any(), (k, ratios)
        # the overlay with S = H + a rectangle's pick: the hidden part of S draws nothing
        sel, oref = c1.ref("overlay", k)
        r.set_selection(sel)
        rgba, cover = r.read_overlay()
        fb = r.readPixelsFloat()
        none = ~oref["maybe"]
        assert not cover[none].any() and np.array_equal(_bits(rgba[none]), _bits(fb[none])), (k, "pixels without a selected fragment")
        lit = cover > 0
        assert not (lit & none).any() and not (oref["surely"] & ~lit).any() and lit.any(), (k, "covered pixels differ")
        oratios = OR.excess(cover, rgba, fb, oref, TINT, MIX)
        print("hide overlay", k, "max |gpu - ref| / bound: cover %.3f overlay - fb %.3f" % oratios)
        assert oratios[0] <= 1.0 and oratios[1] <= 1.0, (k, oratios)
    r.dispose()


# 5 round trip and state ----------------------------------------------------------------------------------------------
def test_round_trip_and_state(gh, monkeypatch, scenes, c1):
    never = _context(gh, monkeypatch, scenes)
    r = _context(gh, monkeypatch, scenes)
    bytes0 = r.scene_sharing()[1]
    k = POSES[0]
    state = lambda c: (c.readPixelsFloat(), c.bin_lists(), c.work_items(), {s: c.stats()[s] for s in ("visible", "bin_entries", "tile_entries", "n")})

    def same(a, b, what):
        assert np.array_equal(_bits(a[0]), _bits(b[0])), (what, "framebuffer")
        assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1]), (what, "lists")
        assert a[2] == b[2] and a[3] == b[3], (what, a[2], b[2], a[3], b[3])

    _frame(gh, r, k)
    A = state(r)
    ys, xs = np.nonzero(r.read_depth()[2] != NONE)           # pixels with a hit in the unhidden frame
    pts = [(int(xs[j]), int(ys[j])) for j in range(0, xs.size, max(1, xs.size // 64))]
    assert (r.pick(pts)["index"] != NONE).all()
    r.set_selection(c1.H)
    assert r.hide_selected() == int(c1.H.sum())
    for call in (lambda: r.pick(pts), r.depth_async, lambda: r.select_region(RECT)):          # an edit since the frame, as after a translate
        with pytest.raises(gh.GsplatError, match="no frame") as ei:
            call()
        assert ei.value.code == GSR_ERR_ARG
    _frame(gh, r, k)
    B1 = state(r)
    hits = r.pick(pts)["index"]                                                               # answers again, and sees through
    assert (hits != NONE).any() and not c1.H[hits[hits != NONE]].any()
    assert not np.array_equal(_bits(A[0]), _bits(B1[0])) and B1[3]["bin_entries"] < A[3]["bin_entries"]
    _frame(gh, r, k)
    same(state(r), B1, "the hidden frame once more (replayed)")
    assert r.hide_selected() == int(c1.H.sum())              # changes no bit: an edit all the same
    with pytest.raises(gh.GsplatError, match="no frame"):
        r.pick(pts)
    assert r.set_hidden(None) == 0                            # show all; the buffers stay
    assert r.scene_sharing()[1] > bytes0
    _frame(gh, r, k)
    same(state(r), A, "frame C is frame A")
    _frame(gh, never, k)
    same(state(never), A, "a context that never hid")
    assert never.scene_sharing()[1] == bytes0                 # ... holds what it always held
    fresh = _context(gh, monkeypatch, scenes)
    assert fresh.set_hidden(words=HR.pack(c1.H)) == int(c1.H.sum())
    _frame(gh, fresh, k)
    same(state(fresh), B1, "a fresh context given the words")
    flat = _context(gh, monkeypatch, scenes, rows=False)     # a scene without rotations and scales can hide
    flat.set_raw_scene(c1.data, c1.pos)
    assert flat.set_hidden(c1.H) == int(c1.H.sum())
    _frame(gh, flat, k)
    same(state(flat), B1, "a scene from gsr_set_scene")
    r.set_hidden(c1.H)
    r.set_scene_rows(c1.rows)                                 # a new scene leaves nothing hidden and frees the buffers
    assert r.hidden_count() == 0 and not r.hidden_words().any() and r.scene_sharing()[1] == bytes0
    _frame(gh, r, k)
    same(state(r), A, "after a new scene")
    for c in (never, r, fresh, flat):
        c.dispose()


# 6 compaction --------------------------------------------------------------------------------------------------------
def _box_of_half(pos):
    xs = np.sort(np.asarray(pos).reshape(-1, 3)[:, 0].astype(np.float64))
    return (float(xs[xs.size // 2]), 99.0, -99.0, 99.0, -99.0, 99.0)


def _compaction(gh, monkeypatch, scenes, oracle, count, lib_path=None):
    made = []
    for how in ("erase", "limit_box"):
        r = _context(gh, monkeypatch, scenes, name=count, seed=None if count == NAME else 7, lib_path=lib_path)
        n = r.scene_count()
        before = r.read_scene()
        pos = before[1]
        box = _box_of_half(pos)
        Bx = SR.box_pick(pos, box)
        Hs = HR.test_set(n, pos, BOX, SEED + n)
        assert n < 32 or (not np.array_equal(Hs, Bx) and 0 < Bx.sum())
        assert r.set_hidden(Hs) == int(Hs.sum())
        if how == "erase":
            r.select_box(box)
            keep = ~Bx
            assert r.scene_erase_selected() == int(keep.sum())
            assert r.selection_count() == 0                   # the selection is still dropped there
        else:
            keep = Bx
            assert r.scene_limit_box(box) == int(keep.sum())
        want = HR.compact(Hs, keep)
        _hidden_is(r, want, (count, how))
        after = r.read_scene()
        for a, b, per in zip(after, before, (8, 3, 4, 3)):
            assert np.array_equal(_bits(a), _bits(b.reshape(n, per)[keep].reshape(-1))), (count, how, per)
        if count == NAME:                                     # the next frame: the compacted scene with the compacted H
            for k in POSES:
                cam = _cam(gh, k)
                v, p, vp = cam.f32()
                _, bbox, _ = oracle.project(after[0], v, p, cam.fx, cam.fy, W, H)
                order = oracle.sort(vp, after[1])[0]
                _frame(gh, r, k)
                starts, lst = r.bin_lists()
                ws, wl = B.bin_lists_reference(HR.hide_bbox(bbox, want), order, W, H)
                diff = B.first_difference(starts, lst, ws, wl)
                assert diff is None and 0 < lst.size, (how, k, diff)
                assert np.array_equal(r.lastDepthIndex(), order)
        made.append(r)
    # erasing the hidden splats for good
    r = made[0]
    n, Hc, before = r.scene_count(), r.hidden(), r.read_scene()
    assert r.select_hidden("replace") == int(Hc.sum())
    assert r.scene_erase_selected() == n - int(Hc.sum()) == r.scene_count()
    assert r.hidden_count() == 0 and not r.hidden_words().any() and r.hidden_words().size == -(-(n - int(Hc.sum())) // 32)
    for a, b, per in zip(r.read_scene(), before, (8, 3, 4, 3)):
        assert np.array_equal(_bits(a), _bits(b.reshape(n, per)[~Hc].reshape(-1))), (count, "erase hidden", per)
    return made


@pytest.mark.parametrize("count", [NAME] + list(TINY), ids=str)
def test_compaction_carries_the_hidden_set(gh, monkeypatch, scenes, oracle, count):
    for r in _compaction(gh, monkeypatch, scenes, oracle, count):
        r.dispose()


def test_compaction_with_sh_that_follows(gh, monkeypatch, scenes, c1):
    n = c1.n
    rng = np.random.default_rng(11)
    band = np.array([999, 4000, 7000], dtype=np.int32)
    tex = [rng.integers(0, 1 << 32, 8 * (n - 1000), dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    r = _context(gh, monkeypatch, scenes)
    r.set_sh_follow(True)
    r.set_sh(tex, band)
    r.set_hidden(c1.H)
    _frame(gh, r, POSES[0])
    col = r.read_sh_colors()
    listed = SR.listed(c1.views[POSES[0]]["hbbox"])
    assert not _bits(col[c1.H]).any(), "a hidden SH splat wrote its colour"
    assert _bits(col[listed & (np.arange(n) > 999)]).any()
    box = _box_of_half(c1.pos)
    Bx = SR.box_pick(c1.pos, box)
    r.select_box(box)
    assert r.scene_erase_selected() == int((~Bx).sum())
    wt, wb, wc = SF.compact_sh(tex, band, ~Bx)
    gt, gb = r.read_scene_sh()
    assert wc > 0 and np.array_equal(gb, wb) and all(np.array_equal(a, b) for a, b in zip(gt, wt))
    _hidden_is(r, HR.compact(c1.H, ~Bx), "sh follows")
    _frame(gh, r, POSES[0])                                   # and the compacted scene renders with the compacted H
    assert not _bits(r.read_sh_colors()[HR.compact(c1.H, ~Bx)]).any()
    r.dispose()


# 7 shared scene ------------------------------------------------------------------------------------------------------
def test_shared_scene_has_one_hidden_set(gh, monkeypatch, scenes, c1):
    k = POSES[0]
    singles = []
    for hide in (False, True):
        s = _context(gh, monkeypatch, scenes)
        if hide:
            s.set_hidden(c1.H)
        _frame(gh, s, k)
        singles.append(s.readPixels().reshape(H, W, 4).copy())
        s.dispose()
    assert not np.array_equal(singles[0], singles[1])
    a = _context(gh, monkeypatch, scenes)
    b, c = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    b.share_scene(a)
    c.share_scene(a)
    a.open_delivery(3)
    a.set_camera(_cam(gh, k))
    a.render_async()                                          # member 1 enqueues a frame (and its delivery: the framebuffer is reused) ...
    first = a.deliver()
    assert b.set_hidden(c1.H) == int(c1.H.sum())              # ... member 2 hides ...
    with pytest.raises(gh.GsplatError, match="no frame"):     # (every member's frame state is marked as edited: no wait, a host check)
        a.pick([(320, 240)])
    a.render_async()                                          # ... and member 1 enqueues another
    second = a.deliver()
    for serial, want, what in ((first, singles[0], "enqueued before the hide"), (second, singles[1], "enqueued behind the hide")):
        got_serial, px = a.acquire(serial)
        assert got_serial == serial and np.array_equal(px, want), what
        a.release(serial)
    a.sync()
    _hidden_is(a, c1.H, "read through member 1")
    _hidden_is(c, c1.H, "read through a member that never rendered")
    assert a.scene_sharing() == b.scene_sharing() and a.scene_sharing()[0] == 3
    c.set_scene_rows(c1.rows)                                 # a member that leaves starts with nothing hidden; the others keep theirs
    assert c.hidden_count() == 0 and not c.hidden_words().any()
    _hidden_is(b, c1.H, "after a member left")
    d = gh.HIPRenderer(W, H)
    d.share_scene(b)                                          # and a new member takes H over with the scene
    _hidden_is(d, c1.H, "taken over with the scene")
    _frame(gh, d, k)
    assert np.array_equal(d.readPixels().reshape(H, W, 4), singles[1])
    for x in (a, b, c, d):
        x.dispose()


# 8 bounds build ------------------------------------------------------------------------------------------------------
def _bounds_lib():
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    return BOUNDS_LIB


@pytest.mark.parametrize("kind", list(KINDS))
def test_bounds_twin_lists(gh, monkeypatch, scenes, c1, kind):
    r = _context(gh, monkeypatch, scenes, lib_path=_bounds_lib(), **KINDS[kind])
    _lists_equal_the_reference(gh, r, c1, KINDS[kind].get("band"), ("bounds", kind), records=kind == "default")
    _bounds_zero(r, ("lists", kind))
    r.dispose()


@pytest.mark.parametrize("count", [NAME] + list(TINY), ids=str)
def test_bounds_twin_compaction(gh, monkeypatch, scenes, oracle, count):
    made = _compaction(gh, monkeypatch, scenes, oracle, count, lib_path=_bounds_lib())
    _bounds_zero(made[0], ("compaction", count))
    for r in made:
        r.dispose()

"""Splat selection on the GPU (k_select.hip, gsr_select.cpp) against tests/select_reference.py -- the specification in numpy, fed
by the oracle's projection, the planes tests/test_gpu_depth.py pins and the arrays read back BEFORE an edit, never by anything the
selection kernels wrote -- and against the pinned gsr_scene_limit_box where the two run the same compaction.  The frame must not
notice a selection, and a context that never selects is what it always was."""
import ctypes
import os

import numpy as np
import pytest

import select_reference as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
KNOBS = ("GSR_BIN_TWO_LEVEL", "GSR_LONG_ITEMS", "GSR_DEPTH_SKIP")
GSR_ERR_ARG = -1
NAME, POSES = "C1", (3, 40)
W, H = 640, 480
TINY = (1, 31, 32, 33, 1023, 1024, 1025)          # word, wave and BOX_THREADS block edges
RECT = (200, 150, 330, 270)
DISC = (317, 243, 70)
BOX = (-1.0, 2.5, -0.75, 3.0, -2.0, 1.0)          # about half of C1


def _regions():
    """(id, rect, mask): the rectangles, the whole image, the disc as bytes, the disc again with rows longer than it is wide"""
    drect, dmask = SR.disc(*DISC)
    _, dwide = SR.disc(*DISC, stride_pad=13)
    return [("rect", RECT, None), ("corner", (608, 448, 640, 480), None), ("four bins", (31, 31, 33, 33), None),
            ("one pixel", (300, 220, 301, 221), None), ("disc rect", drect, None), ("whole", (0, 0, W, H), None),
            ("disc", drect, dmask), ("disc wide", drect, dwide)]


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    cfg = gsplat_hip.synth.CONFIGS[NAME]
    assert (cfg["width"], cfg["height"]) == (W, H) and cfg["n"] % 32 == 16
    return gsplat_hip


def _cam(gh, k):
    cfg = gh.synth.CONFIGS[NAME]
    return gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"])


@pytest.fixture(scope="module")
def proj(oracle, scenes, gh):
    """pose -> (rec, bbox) of the oracle's projection of C1: computed once, shared, never changed"""
    _, data, _ = scenes(NAME)
    out = {}
    for k in POSES:
        cam = _cam(gh, k)
        v, p, _ = cam.f32()
        rec, bbox, _ = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
        rec.flags.writeable = False; bbox.flags.writeable = False
        out[k] = (rec, bbox)
    return out


def _context(gh, monkeypatch, scenes, env=None, name=NAME, seed=None, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    r = gh.HIPRenderer(W, H, **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)
    r.set_scene_rows(scenes(name, seed)[0])
    return r


def _frame(gh, r, k):
    r.set_camera(_cam(gh, k))
    r.render_async()
    r.sync()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _is(r, want, what):
    """the device's selection is `want` (bool[n]): word for word, and the count"""
    words = r.selection_words()
    ref = SR.pack(want)
    assert words.dtype == np.uint32 and words.shape == ref.shape, what
    bad = np.nonzero(words != ref)[0]
    assert not bad.size, (what, bad[:4].tolist(), [hex(int(v)) for v in words[bad[:4]]], [hex(int(v)) for v in ref[bad[:4]]])
    assert r.selection_count() == int(np.sum(want)), what


def _bounds_zero(r, what):
    for name in ("gsr_debug_bounds_select", "gsr_debug_bounds_scene_sh", "gsr_debug_bounds_depth"):
        buf = (ctypes.c_uint32 * 8)()
        assert getattr(r._L, name)(buf) == 0
        assert not any(buf), (what, name, list(buf))


# 1 -------------------------------------------------------------------------------------------------------------------
def _centre_equals_the_reference(gh, r, proj, what):
    n = r.scene_count()
    for k in POSES:
        rec, bbox = proj[k]
        _frame(gh, r, k)
        for rid, rect, mask in _regions():
            want = SR.centre_pick(rec, bbox, rect, mask)
            print("centre", what, k, rid, int(want.sum()))
            got = r.select_region(rect, mask, mode="centre", op="replace")
            _is(r, want, (what, k, rid))
            assert got == int(want.sum())
            if rid in ("rect", "whole", "disc", "disc wide"):
                assert 0 < got < n, (what, k, rid)       # neither nothing nor everything


@pytest.mark.parametrize("kind", ["default", "throughput", "two level"])
def test_centre_equals_the_reference(gh, monkeypatch, scenes, proj, kind):
    env = {"GSR_BIN_TWO_LEVEL": "1"} if kind == "two level" else None
    r = _context(gh, monkeypatch, scenes, env=env, throughput=kind == "throughput")
    _centre_equals_the_reference(gh, r, proj, kind)
    r.dispose()


# 2 -------------------------------------------------------------------------------------------------------------------
def _hit_equals_the_plane(gh, r, what):
    n = r.scene_count()
    _frame(gh, r, POSES[0])
    drect, dmask = SR.disc(*DISC)
    sets = {}
    for alpha in (0.5, 0.9):
        r.set_hit_alpha(alpha)
        for rid, rect, mask in (("rect", RECT, None), ("disc", drect, dmask), ("whole", (0, 0, W, H), None)):
            got = r.select_region(rect, mask, mode="hit")      # (runs the planes pass itself: they are not this frame's / this alpha's)
            index = r.read_depth()[2]
            want = SR.hit_pick(index, n, rect, mask)
            print("hit", what, alpha, rid, int(want.sum()))
            _is(r, want, (what, alpha, rid))
            assert 0 < got == int(want.sum()) < n
            sets[(alpha, rid)] = want
    assert not np.array_equal(sets[(0.5, "whole")], sets[(0.9, "whole")])   # the selection follows the new plane
    r.set_hit_alpha(0.5)


def test_hit_equals_the_index_plane(gh, monkeypatch, scenes):
    r = _context(gh, monkeypatch, scenes)
    _hit_equals_the_plane(gh, r, "default")
    r.dispose()


# 3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [NAME] + list(TINY), ids=str)
def test_ops_against_numpy(gh, monkeypatch, scenes, count):
    r = _context(gh, monkeypatch, scenes, name=count, seed=None if count == NAME else 7)
    n = r.scene_count()
    nw = -(-n // 32)
    rng = np.random.default_rng(n)
    assert r.selection_count() == 0 and not r.selection().any() and r.selection().shape == (n,)   # never selected in: all zeros
    S = np.zeros(n, bool)
    for step, op in enumerate(("replace", "add", "subtract", "intersect", "add", "replace")):
        P = rng.random(n) < (0.5, 0.2, 0.3, 0.7, 0.1, 0.4)[step]
        S = SR.apply_op(S, P, op)
        assert r.set_selection(P, op=op) == int(S.sum())
        _is(r, S, (n, step, op))
    assert r.invert_selection() == n - int(S.sum())
    S = ~S
    _is(r, S, (n, "invert"))                                  # (word for word: the tail stays 0)
    ones = np.full(nw + 3, 0xFFFFFFFF, dtype=np.uint32)       # more words than needed, every bit set: bits at and above n are dropped
    assert r.set_selection(words=ones, op="intersect") == int(S.sum())
    _is(r, S, (n, "intersect with everything"))
    assert r.set_selection(words=ones) == n
    _is(r, np.ones(n, bool), (n, "all ones"))
    assert r.invert_selection() == 0
    _is(r, np.zeros(n, bool), (n, "invert of everything"))
    assert r.invert_selection() == n and r.set_selection(None, op="intersect") == 0               # NULL words: the empty set
    _is(r, np.zeros(n, bool), (n, "intersect with nothing"))
    # the ops with a picker's set for P
    _, pos, _, _ = r.read_scene()
    xs = np.sort(pos.reshape(-1, 3)[:, 0].astype(np.float64))
    lo, hi = float(xs[n // 4]), float(xs[-1]) + 1.0
    P = SR.box_pick(pos, (lo, hi, -1e9, 1e9, -1e9, 1e9))
    S = rng.random(n) < 0.5
    r.set_selection(S)
    for op in ("subtract", "add", "intersect", "replace"):
        S = SR.apply_op(S, P, op)
        assert r.select_box((lo, hi, -1e9, 1e9, -1e9, 1e9), op=op) == int(S.sum())
        _is(r, S, (n, "box", op))
    if nw > 1:
        with pytest.raises(gh.GsplatError, match="nwords") as ei:
            r.set_selection(words=np.zeros(nw - 1, np.uint32))
        assert ei.value.code == GSR_ERR_ARG
        _is(r, S, (n, "after a refused set"))
    r.dispose()


# 4 -------------------------------------------------------------------------------------------------------------------
def test_select_box_is_the_f64_predicate(gh, monkeypatch, scenes):
    r = _context(gh, monkeypatch, scenes)
    n = r.scene_count()
    _, pos, _, _ = r.read_scene()
    p = pos.reshape(-1, 3)
    edge = float(p[1234, 0])                                  # a bound that IS a splat's coordinate: both comparisons are inclusive
    for box in (BOX, (edge, 9.0, -9.0, 9.0, -9.0, 9.0), (-9.0, edge, -9.0, 9.0, -9.0, 9.0), (-1e-3, 1e-3, -9, 9, -9, 9), (-99, 99, -99, 99, -99, 99)):
        want = SR.box_pick(pos, box)
        assert r.select_box(box) == int(want.sum())
        _is(r, want, box)
    assert want.all()
    want = SR.box_pick(pos, BOX)
    assert 0 < r.select_box(BOX) == int(want.sum()) < n
    for bad, word in (((1, 1, 0, 1, 0, 1), "xMin"), ((0, 1, 2, 1, 0, 1), "yMin"), ((0, 1, 0, 1, 3, 3), "zMin")):
        with pytest.raises(gh.GsplatError, match=word + ".*must be smaller") as ei:
            r.select_box(bad)
        assert ei.value.code == GSR_ERR_ARG
        with pytest.raises(gh.GsplatError, match=word + ".*must be smaller"):
            r.scene_limit_box(bad)                            # limitBox refuses the same boxes
    _is(r, want, "after the refusals")
    r.dispose()


# 5 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("follow", [False, True], ids=["sh dropped", "sh follows"])
def test_erase_equals_the_pinned_limit_box(gh, monkeypatch, scenes, follow):
    n = gh.synth.CONFIGS[NAME]["n"]
    rng = np.random.default_rng(11)
    band = np.array([999, 4000, 7000], dtype=np.int32)
    tex = [rng.integers(0, 1 << 32, 8 * (n - 1000), dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    got = []
    for how in ("erase", "limit_box"):
        r = _context(gh, monkeypatch, scenes)
        r.set_sh_follow(follow)
        r.set_sh(tex, band)
        if how == "erase":
            picked = r.select_box(BOX)
            kept = r.scene_erase_selected(keep=True)
            assert kept == picked and 0 < kept < n
            assert r.selection_count() == 0 and not r.selection_words().any() and r.selection_words().size == -(-kept // 32)
        else:
            kept = r.scene_limit_box(BOX)
        assert r.scene_count() == kept
        got.append((kept, r.read_scene(), r.read_scene_sh()))
        r.dispose()
    (ka, sa, (ta, ba)), (kb, sb, (tb, bb)) = got
    assert ka == kb
    for a, b in zip(sa, sb):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(ba, bb) and all(np.array_equal(a, b) for a, b in zip(ta, tb))
    assert (ta[0].size > 0) == follow                         # compacted with the scene, or dropped


# 6 -------------------------------------------------------------------------------------------------------------------
def _erase_of_a_region_selection(gh, monkeypatch, scenes, proj, lib_path=None):
    r = _context(gh, monkeypatch, scenes, lib_path=lib_path)
    n = r.scene_count()
    _frame(gh, r, POSES[0])
    before = r.read_scene()
    picked = r.select_region(RECT, mode="centre")
    sel = r.selection()
    assert np.array_equal(sel, SR.centre_pick(*proj[POSES[0]], RECT)) and 0 < picked < n
    assert r.scene_erase_selected() == n - picked == r.scene_count()
    after = r.read_scene()
    for a, b, per in zip(after, before, (8, 3, 4, 3)):
        assert np.array_equal(_bits(a), _bits(b.reshape(n, per)[~sel].reshape(-1))), per     # numpy indexing: order is kept
    assert r.selection_count() == 0 and not r.selection_words().any()
    fresh = gh.HIPRenderer(W, H, lib_path=lib_path)
    fresh.set_scene_arrays(*after)
    for c in (r, fresh):
        _frame(gh, c, POSES[1])
    assert np.array_equal(_bits(r.readPixelsFloat()), _bits(fresh.readPixelsFloat()))
    assert np.array_equal(r.lastDepthIndex(), fresh.lastDepthIndex())
    fresh.dispose()
    return r


def test_erase_of_a_region_selection(gh, monkeypatch, scenes, proj):
    _erase_of_a_region_selection(gh, monkeypatch, scenes, proj).dispose()


# 7 -------------------------------------------------------------------------------------------------------------------
def test_nothing_to_remove_changes_nothing(gh, monkeypatch, scenes):
    r = _context(gh, monkeypatch, scenes)
    n = r.scene_count()
    _frame(gh, r, POSES[0])
    pts = [(320, 240), (100, 100), (317, 243)]
    before = (r.pick(pts), r.read_scene(), r.stats(), r.scene_sharing())
    assert (before[0]["index"] != SR.NONE).any()
    assert r.scene_erase_selected() == n                      # nothing selected (and nothing allocated for it)
    assert r.scene_sharing() == before[3]
    r.set_selection(None)
    assert r.scene_erase_selected() == n
    assert r.invert_selection() == n
    assert r.scene_erase_selected(keep=True) == n             # everything selected and kept
    after = (r.pick(pts), r.read_scene(), r.stats())          # pick still answers: the last frame is valid, nothing was rendered
    assert np.array_equal(after[0], before[0]) and after[2] == before[2]
    for a, b in zip(after[1], before[1]):
        assert np.array_equal(_bits(a), _bits(b))
    assert r.selection_count() == n and r.scene_count() == n  # the selection stays too
    r.dispose()


# 8 -------------------------------------------------------------------------------------------------------------------
def test_the_frame_does_not_notice(gh, monkeypatch, scenes):
    plain = _context(gh, monkeypatch, scenes)
    r = _context(gh, monkeypatch, scenes)
    bytes0 = r.scene_sharing()[1]
    for c in (plain, r):
        _frame(gh, c, POSES[0])
    state = lambda c: (c.readPixelsFloat(), c.lastDepthIndex(), c.work_items(), c.stats())
    before = state(r)
    drect, dmask = SR.disc(*DISC)
    calls = [lambda: r.select_region(RECT), lambda: r.select_region(drect, dmask, op="add"), lambda: r.select_region(RECT, mode="hit", op="subtract"),
             lambda: r.select_box(BOX, op="intersect"), lambda: r.set_selection(np.arange(r.scene_count()) % 3 == 0, op="add"),
             lambda: r.invert_selection(), lambda: r.selection(), lambda: r.selection_count()]
    for k, call in enumerate(calls):
        call()
        after = state(r)
        assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(after[1], before[1]), k
        assert after[2] == before[2] and after[3] == before[3], k
    assert r.scene_sharing()[1] > bytes0 == plain.scene_sharing()[1]      # the selection's buffers are counted once they exist
    for c in (plain, r):
        _frame(gh, c, POSES[1])
    a, b = state(r), state(plain)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    plain.dispose(); r.dispose()


# 9 -------------------------------------------------------------------------------------------------------------------
def test_band_context(gh, monkeypatch, scenes, proj):
    band = (192, 416)
    r = _context(gh, monkeypatch, scenes, band=band)
    n = r.scene_count()
    drect, dmask = SR.disc(*DISC)
    for k in POSES:
        rec, bbox = proj[k]
        _frame(gh, r, k)
        for rid, rect, mask in (("rect", RECT, None), ("the band", (band[0], 0, band[1], H), None), ("disc", drect, dmask),
                                ("first column", (band[0], 0, band[0] + 1, H), None), ("last column", (band[1] - 1, 0, band[1], H), None)):
            want = SR.centre_pick(rec, bbox, rect, mask, band=band)
            got = r.select_region(rect, mask)
            _is(r, want, ("band", k, rid))
            if rid in ("rect", "the band", "disc"):
                assert 0 < got < n
        index = r.read_depth()[2]
        r.select_region(RECT, mode="hit")
        _is(r, SR.hit_pick(index, n, RECT), ("band", k, "hit"))
    want = r.selection()
    for rect in ((band[0] - 1, 150, 330, 270), (200, 150, band[1] + 1, 270), (0, 0, W, H), (0, 0, 32, 32)):
        for mode in ("centre", "hit"):
            with pytest.raises(gh.GsplatError, match="band") as ei:
                r.select_region(rect, mode=mode)
            assert ei.value.code == GSR_ERR_ARG
    _is(r, want, "after the refusals")
    r.dispose()


# 10 ------------------------------------------------------------------------------------------------------------------
def test_shared_scene_has_one_selection(gh, monkeypatch, scenes, proj):
    a = _context(gh, monkeypatch, scenes)
    b, c = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H, throughput=True)
    n = a.scene_count()
    a.select_box(BOX)                                         # a selection made before the share goes with the scene
    b.share_scene(a)
    c.share_scene(a)
    _is(b, SR.box_pick(scenes(NAME)[2], BOX), "taken over with the scene")
    _frame(gh, a, POSES[0])
    _frame(gh, b, POSES[1])
    want = SR.centre_pick(*proj[POSES[0]], RECT)
    assert a.select_region(RECT) == int(want.sum())           # A's camera
    _is(b, want, "read through another member")
    both = want | SR.centre_pick(*proj[POSES[1]], RECT)
    assert b.select_region(RECT, op="add") == int(both.sum()) # B's camera into the same bits, no events in between
    _is(a, both, "added through another member")
    assert a.scene_sharing()[1] == b.scene_sharing()[1] and a.scene_sharing()[0] == 3
    c.set_scene_rows(scenes(NAME)[0])                         # a member that leaves starts empty; the others keep theirs
    assert c.selection_count() == 0 and not c.selection_words().any()
    _is(a, both, "after a member left")
    before = a.read_scene()
    assert b.scene_erase_selected() == n - int(both.sum())
    after = a.read_scene()
    for x, y, per in zip(after, before, (8, 3, 4, 3)):
        assert np.array_equal(_bits(x), _bits(y.reshape(n, per)[~both].reshape(-1)))
    assert a.selection_count() == 0 and b.selection_count() == 0
    with pytest.raises(gh.GsplatError, match="no frame"):     # every member's frame state went with the old numbering
        a.select_region(RECT)
    fresh = gh.HIPRenderer(W, H)
    fresh.set_scene_arrays(*after)
    for m, k in ((a, POSES[0]), (b, POSES[1])):
        _frame(gh, m, k)
        _frame(gh, fresh, k)
        assert np.array_equal(_bits(m.readPixelsFloat()), _bits(fresh.readPixelsFloat())) and np.array_equal(m.lastDepthIndex(), fresh.lastDepthIndex())
    for x in (a, b, c, fresh):
        x.dispose()


# 11 ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_selection_alone(gh, monkeypatch, scenes):
    r = _context(gh, monkeypatch, scenes)
    n = r.scene_count()
    S = np.arange(n) % 5 == 1
    r.set_selection(S)

    def refused(match, call):
        with pytest.raises(gh.GsplatError, match=match) as ei:
            call()
        assert ei.value.code == GSR_ERR_ARG, match
        _is(r, S, match)

    for mode in ("centre", "hit"):
        refused("no frame", lambda: r.select_region(RECT, mode=mode))
    _frame(gh, r, POSES[0])
    r.sort()
    refused("sort-only", lambda: r.select_region(RECT))
    _frame(gh, r, POSES[0])
    r.scene_translate((0.0, 0.0, 0.0))                        # an edit since the frame: its lists are of another scene
    for mode in ("centre", "hit"):
        refused("no frame", lambda: r.select_region(RECT, mode=mode))
    S = SR.apply_op(S, SR.box_pick(r.read_scene()[1], BOX), "add")
    assert r.select_box(BOX, op="add") == int(S.sum())        # the box needs no frame
    _frame(gh, r, POSES[0])
    for rect in ((-1, 0, 10, 10), (0, -1, 10, 10), (10, 10, 10, 20), (10, 10, 20, 10), (20, 10, 10, 20), (0, 0, W + 1, 10), (0, 0, 10, H + 1)):
        refused("rectangle", lambda: r.select_region(rect))
    refused("mask_stride", lambda: r.select_region((10, 10, 20, 20), np.ones((10, 9), np.uint8)))
    refused("mode", lambda: r.select_region(RECT, mode=2))
    refused("mode", lambda: r.select_region(RECT, mode=-1))
    for op in (4, -1):
        refused("op", lambda: r.select_region(RECT, op=op))
        refused("op", lambda: r.select_box(BOX, op=op))
        refused("op", lambda: r.set_selection(S, op=op))
    reg = gh.GsrRegion(10, 10, 20, 20, None, 0, 1)
    assert r._L.gsr_select_region(r._ctx, ctypes.byref(reg), 0, 0, None) == GSR_ERR_ARG and b"reserved" in r._L.gsr_last_error(r._ctx)
    assert r._L.gsr_select_region(r._ctx, None, 0, 0, None) == GSR_ERR_ARG
    words = np.zeros(-(-n // 32), np.uint32)
    assert r._L.gsr_read_selection(r._ctx, words.ctypes.data, words.size - 1, None) == GSR_ERR_ARG and b"nwords" in r._L.gsr_last_error(r._ctx)
    assert r._L.gsr_selection_set(r._ctx, words.ctypes.data, words.size - 1, 0, None) == GSR_ERR_ARG
    _is(r, S, "after every refusal")
    assert r.select_region(RECT) > 0                          # and the frame is still good for a selection
    r.dispose()
    flat = gh.HIPRenderer(W, H)                               # a scene without rotations and scales: limitBox's own error
    _, data, pos = scenes(NAME)
    flat.set_raw_scene(data, pos)
    assert flat.select_box(BOX) > 0
    for call in (lambda: flat.scene_erase_selected(), lambda: flat.scene_limit_box(BOX)):
        with pytest.raises(gh.GsplatError, match="gsr_set_scene_rows") as ei:
            call()
        assert ei.value.code == GSR_ERR_ARG
    assert flat.selection_count() > 0
    flat.dispose()


# 12 ------------------------------------------------------------------------------------------------------------------
def test_a_frame_that_did_not_fit_is_repaired_first(gh, monkeypatch, scenes, proj):
    r = _context(gh, monkeypatch, scenes)
    n = r.scene_count()
    _frame(gh, r, POSES[0])
    assert r.stats()["bin_entries"] > 4096
    for frames, mode in ((1, "centre"), (2, "hit")):
        r.set_list_capacity(1024)                             # far too small for the next frame (the handled regrowth path)
        r.set_camera(_cam(gh, POSES[1]))
        r.render_async()
        got = r.select_region(RECT, mode=mode)                # renders the frame again with regrown lists, then selects
        assert r.stats()["overflow_frames"] == frames and r.stats()["dropped_frames"] == 0
        want = SR.centre_pick(*proj[POSES[1]], RECT) if mode == "centre" else SR.hit_pick(r.read_depth()[2], n, RECT)
        _is(r, want, ("overflow", mode))
        assert 0 < got == int(want.sum())
    r.dispose()


# 13 ------------------------------------------------------------------------------------------------------------------
def test_bounds_twin(gh, monkeypatch, scenes, proj):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    for throughput in (False, True):
        r = _context(gh, monkeypatch, scenes, throughput=throughput, lib_path=BOUNDS_LIB)
        _centre_equals_the_reference(gh, r, proj, ("bounds", throughput))
        _hit_equals_the_plane(gh, r, ("bounds", throughput))
        _bounds_zero(r, ("bounds", throughput))
        r.dispose()
    r = _erase_of_a_region_selection(gh, monkeypatch, scenes, proj, lib_path=BOUNDS_LIB)
    _bounds_zero(r, "erase")
    r.dispose()
    r = _context(gh, monkeypatch, scenes, name=1025, seed=7, lib_path=BOUNDS_LIB)      # the box picker and the followed SH compaction
    n = r.scene_count()
    r.set_sh_follow(True)
    r.set_sh([np.arange(8 * (n - 100), dtype=np.uint32)] * 3, np.array([99, 400, 700], dtype=np.int32))
    pos = r.read_scene()[1]
    mid = float(np.median(pos.reshape(-1, 3)[:, 0]))
    want = SR.box_pick(pos, (mid, 99, -99, 99, -99, 99))
    assert r.select_box((mid, 99, -99, 99, -99, 99)) == int(want.sum())
    _is(r, want, "bounds box")
    assert r.scene_erase_selected(keep=True) == int(want.sum())
    tex, band = r.read_scene_sh()
    keep_sh = want[100:]
    assert np.array_equal(tex[0], np.arange(8 * (n - 100), dtype=np.uint32).reshape(-1, 8)[keep_sh].reshape(-1))
    assert band.tolist() == [int(want[:100].sum()) - 1, int(want[:401].sum()) - 1, int(want[:701].sum()) - 1]
    _bounds_zero(r, "box and SH")
    r.dispose()


# 14 ------------------------------------------------------------------------------------------------------------------
# The contract every picker's kernel shares (mask_store_ballot, k_splat_ops.h): EVERY word of the scratch mask is written, so no
# picker zeroes it first.  n = 33: one wave, the second word partial; 65: the second wave stores one word and must not store a
# second; 257: a second workgroup.  Each picker first takes everything -- behind the previous picker's empty mask, so every word
# must have been written with its bits -- then nothing, behind its own full mask, so every word must have been written with zeros.
# (The two masks k_merge.hip stores the same way are test_gpu_merge.py's, on both builds.)
EVERY = (-1e9, 1e9, -1e9, 1e9, -1e9, 1e9)
FAR = (1e8, 1e9, 1e8, 1e9, 1e8, 1e9)
LINK = 32.0                                       # synth positions lie in [-6, 6]^3: every splat is within LINK of every other


def _pickers(r):
    """(name, take everything, take nothing): each returns the selected count of a REPLACE"""
    return [("gsr_select_attr", lambda: r.select_attr("x"), lambda: r.select_attr("x", lo=0.0, hi=0.0)),
            ("gsr_select_neighbours", lambda: r.select_neighbours(LINK)[0], lambda: r.select_neighbours(LINK, lo=0, hi=0)[0]),
            ("gsr_select_knn", lambda: r.select_knn(LINK)[0], lambda: r.select_knn(LINK, lo=0.0, hi=0.0)[0]),
            ("gsr_select_clusters", lambda: r.select_clusters(LINK)[0], lambda: r.select_clusters(LINK, lo=0, hi=0)[0]),
            # one island at LINK; at a radius nobody has a neighbour within and min_pts = 1 the seed is noise: the empty set
            ("gsr_select_cluster_at", lambda: r.select_cluster_at(LINK, "largest")[0], lambda: r.select_cluster_at(1e-6, 0, min_pts=1)[0]),
            ("gsr_select_contrib", lambda: r.select_contrib("pixels", below=np.inf), lambda: r.select_contrib("pixels", below=0.0)),
            ("gsr_select_box", lambda: r.select_box(EVERY), lambda: r.select_box(FAR))]


@pytest.mark.parametrize("build", ["shipped", "bounds twin"])
@pytest.mark.parametrize("n", [33, 65, 257])
def test_every_picker_stores_every_word(gh, monkeypatch, scenes, n, build):
    if build != "shipped":
        assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    r = _context(gh, monkeypatch, scenes, name=n, seed=7, **({} if build == "shipped" else {"lib_path": BOUNDS_LIB}))
    assert r.scene_count() == n
    _frame(gh, r, POSES[0])                       # the contribution picker needs a pass
    r.contrib_reset()
    r.contrib_accumulate()
    r.sync()
    everything, nothing = np.ones(n, bool), np.zeros(n, bool)
    for name, take_all, take_none in _pickers(r):
        assert take_all() == n, (n, name)
        _is(r, everything, (n, name, "everything"))
        assert take_none() == 0, (n, name)
        _is(r, nothing, (n, name, "nothing"))
        assert not r.selection_words().any(), (n, name)
    if build != "shipped":
        for unit in ("attr", "neighbours", "knn", "clusters", "contrib", "select"):
            buf = (ctypes.c_uint32 * 8)()
            assert getattr(r._L, "gsr_debug_bounds_" + unit)(buf) == 0
            assert not any(buf), (n, unit, list(buf))
    r.dispose()

"""The traces of tests/history_trace.py, checked without a GPU: the builders are deterministic, the tour holds every operation,
read-back, refusal and risky pair, every random walk the GPU tests use holds every kind of operation, and the State a trace ends
in is the fold of its operations.  The same for the editing layer's tour and walks -- and, through the oracle on the CPU, that none of
their steps is vacuous (a hide hides something that shows, a region picks some but not all listed splats, an erase removes some but
not all), that duplicates fall on both sides of the capacity, and that `materialise` is the references' chain.  And the same once
more for the analysis layer -- neighbour counts, clusters, k nearest neighbours, merge cells: its tour and its walks over all three
sets of kinds, with the conditions under which a picker, a seed or a merge checks something."""
import hashlib
from dataclasses import replace

import numpy as np
import pytest

import append_reference
import history_trace as ht

WALKS = [(seed, kind) for seed in (101, 202, 303) for kind in ("default", "throughput")]   # tests/test_gpu_history.py::test_random_walks
WALK_STEPS = 60


def _start(kind, seed=0):
    return ht.State(kind=kind, timing=bool(seed & 1))


def test_builders_are_deterministic():
    assert ht.tour() == ht.tour() and ht.tour(True) == ht.tour(True)
    for seed, kind in WALKS:
        a, b = ht.walk(seed, WALK_STEPS, _start(kind, seed)), ht.walk(seed, WALK_STEPS, _start(kind, seed))
        assert a == b and len(a) == WALK_STEPS
        assert ht.walk(seed, 17, _start(kind, seed)) == a[:17]          # a failure at step 16 replays as walk(seed, 17)
    assert ht.walk(101, WALK_STEPS) != ht.walk(202, WALK_STEPS)


@pytest.mark.parametrize("band_context", [False, True])
def test_the_tour_holds_every_operation_and_every_risky_pair(band_context):
    start = ht.State(band=(192, 448) if band_context else None)
    t = ht.tour(band_context)
    kinds = {st.op[0] for st in t}
    assert kinds == set(ht.KINDS), set(ht.KINDS) ^ kinds
    assert {st.op[1] for st in t if st.op[0] == "readback"} == set(ht.READBACKS)
    assert {st.op[1] for st in t if st.op[0] == "refused"} == set(ht.REFUSALS)
    seen = ht.pairs_in(start, t)
    for a, b, why in ht.RISKY_PAIRS:
        assert why
        if band_context and a.startswith("resize"):
            continue      # (a band context sets its band again behind every resize: that operation is the resize's neighbour)
        assert (a, b) in seen, (a, b)
    # the sizes cross the 4096-bin boundary (two-level binning, waves per tile) in both directions, the scenes every
    # keys-per-block step (3 << 20 splats) and the sizes the issue names
    bins, s = [], start
    for st in t:
        s = ht.fold(s, st.op)
        bins.append(ht.bins_of(s.W, s.H))
    ups = [1 for x, y in zip(bins, bins[1:]) if x <= 4096 < y]
    downs = [1 for x, y in zip(bins, bins[1:]) if y <= 4096 < x]
    assert ups and downs and 4096 in bins
    ns = [ht.scene_n(st.op[1]) for st in t if st.op[0] == "scene"]
    assert {0, 1, 63, 2049, 70000, 300000, 10000} <= set(ns) and max(ns) > (3 << 20)
    assert any(x > (3 << 20) >= y for x, y in zip(ns, ns[1:])) and any(y > (3 << 20) >= x for x, y in zip(ns, ns[1:]))
    assert any(st.op[0] == "resize" and (st.op[1] % 2 or st.op[2] % 2) for st in t)
    # unchecked steps are only those that keep the last frame readable
    assert all(st.check or st.op[0] in ht.KEEPS_FRAME for st in t)


@pytest.mark.parametrize("seed,kind", WALKS)
def test_every_walk_holds_every_kind_and_stays_cheap(seed, kind):
    t = ht.walk(seed, WALK_STEPS, _start(kind, seed))
    assert {st.op[0] for st in t} == set(ht.KINDS), set(ht.KINDS) - {st.op[0] for st in t}
    s = _start(kind, seed)
    for st in t:
        assert st.check or st.op[0] in ht.KEEPS_FRAME
        if st.op[0] in ("rotate", "translate", "scale", "limit_box"):
            assert ht.scene_form(s.scene) == "rows"          # transforms need a scene built from rows
        if st.op[0] == "ring_open":
            assert s.ring is None
        if st.op[0] in ("ring_close", "deliver"):
            assert s.ring is not None
        s = ht.fold(s, st.op)
        assert ht.scene_n(s.scene) <= 20000 and s.W <= 900 and s.H <= 700
        assert s.band is None or (s.band[0] % 32 == 0 and s.band[0] < s.band[1] <= s.W)


def _digest(trace):
    return hashlib.sha256(ht.describe(trace).encode()).hexdigest()[:16]


def test_the_old_traces_are_unchanged():
    """describe() of tour() and of the walks over KINDS, digested on the commit before the editing layer joined the module"""
    assert (_digest(ht.tour()), _digest(ht.tour(True))) == ("3adedddaafc32c89", "b067c35df2a4aac9")
    want = {101: "d419ffae3778d0f8", 202: "5ae363d8e129a2d3", 303: "11d8bc4105fe7223"}
    for seed, kind in WALKS:
        assert _digest(ht.walk(seed, WALK_STEPS, _start(kind, seed))) == want[seed], (seed, kind)
        assert ht.walk(seed, WALK_STEPS, _start(kind, seed), kinds=ht.KINDS) == ht.walk(seed, WALK_STEPS, _start(kind, seed))
    assert ht.KINDS[0] == "camera" and ht.KINDS[-1] == "refused" and len(ht.KINDS) == 23 and len(ht.REFUSALS) == 4
    assert not set(ht.KINDS) & set(ht.EDIT_KINDS) and not set(ht.REFUSALS) & set(ht.EDIT_REFUSALS)


def test_the_editing_traces_are_unchanged(oracle):
    """describe() of editing_tour() and of the walks over KINDS + EDIT_KINDS, digested on the commit before the analysis layer joined
    the module"""
    assert (_digest(ht.editing_tour()), _digest(ht.editing_tour(True))) == ("b4d3b8a0008e0de6", "1f6632c6227cec5d")
    want = {11: "6a1fa6bba10e2eae", 22: "b38d1852bbcf5ffa", 33: "49c03ba32febef5e"}
    for seed, kind in EDIT_WALKS:
        assert _digest(_edit_walk(oracle, seed, kind)) == want[seed], (seed, kind)
    assert len(ht.EDIT_KINDS) == 18 and len(ht.EDIT_REFUSALS) == 5 and len(ht.SELECT_KINDS) == 7
    assert not set(ht.KINDS + ht.EDIT_KINDS) & set(ht.ANALYSIS_KINDS) and not set(ht.REFUSALS + ht.EDIT_REFUSALS) & set(ht.ANALYSIS_REFUSALS)


# ---------------------------------------------------------------------------------------------------------------------------
# the editing layer
# ---------------------------------------------------------------------------------------------------------------------------
EDIT_WALKS = [(seed, kind) for seed in (11, 22, 33) for kind in ("default", "throughput")]   # tests/test_gpu_history.py::test_editing_walks
EDIT_WALK_STEPS = 150
ALL_KINDS = ht.KINDS + ht.EDIT_KINDS
_edit_walks = {}


def _edit_walk(oracle, seed, kind):
    if (seed, kind) not in _edit_walks:
        _edit_walks[seed, kind] = ht.walk(seed, EDIT_WALK_STEPS, _start(kind, seed), kinds=ALL_KINDS, oracle=oracle)
    return _edit_walks[seed, kind]


def _capacities(start, trace, oracle):
    """[(step, n before, capacity before, n after)] of the trace's duplicates, by the capacity rule of append_reference:
    a scene's capacity is its count when it is set, the old count after a compaction, never shrinks otherwise"""
    out, s, cap = [], start, None
    for i, st in enumerate(trace):
        n0 = ht.materialise(s, oracle).n
        cap = n0 if cap is None else cap
        s = ht.fold(s, st.op)
        n1 = ht.materialise(s, oracle).n
        kind = st.op[0]
        if kind == "duplicate":
            out.append((i, n0, cap, n1))
        if kind == "scene":
            cap = n1
        elif kind in ("limit_box", "erase", "merge_cells"):      # (a merge removes its rows by the same compaction)
            cap = n0 if n1 < n0 else cap
        elif kind == "reserve":
            cap = max(cap, st.op[1])
        elif kind in ("duplicate", "append_arrays"):
            cap = append_reference.capacity_after(cap, n1)
    return out


def _assert_nothing_vacuous(start, trace, oracle):
    s = start
    for i, st in enumerate(trace):
        why = ht.vacuous(s, st.op, oracle)
        assert why is None, "step %d (%s) %s" % (i, " ".join(str(v) for v in st.op), why)
        s = ht.fold(s, st.op)
        if s.contrib:      # live accumulators: nothing moved the splats they describe
            assert st.op[0] not in ht.MOVES_GEOMETRY, i
        assert ht.materialise(s, oracle).n <= ht.MAX_GROWN
        if s.edits and ht.scene_form(s.scene) == "raw":      # a raw scene takes pickers and hides only
            assert {e[0] for e in s.edits} <= set(ht.SELECT_KINDS) | {"hide", "set_hidden"} | set(ht.ANALYSIS_PICKERS)
        if s.ring_overlay:
            assert s.ring is not None
        if st.op[0] in ("duplicate", "append_arrays", "reserve"):
            assert s.sh is None and ht.scene_form(s.scene) == "rows"


def test_the_editing_builders_are_deterministic(oracle):
    assert ht.editing_tour() == ht.editing_tour() and ht.editing_tour(True) == ht.editing_tour(True)
    for seed, kind in EDIT_WALKS[:2]:
        a = _edit_walk(oracle, seed, kind)
        assert len(a) == EDIT_WALK_STEPS and a == ht.walk(seed, EDIT_WALK_STEPS, _start(kind, seed), kinds=ALL_KINDS, oracle=oracle)
        assert ht.walk(seed, 41, _start(kind, seed), kinds=ALL_KINDS, oracle=oracle) == a[:41]
    assert _edit_walk(oracle, 11, "default") != _edit_walk(oracle, 22, "default")


@pytest.mark.parametrize("band_context", [False, True])
def test_the_editing_tour_holds_every_kind_refusal_and_pair(oracle, band_context):
    start = ht.State(band=(192, 448) if band_context else None)
    t = ht.editing_tour(band_context)
    kinds = {st.op[0] for st in t}
    assert set(ht.EDIT_KINDS) <= kinds <= set(ALL_KINDS), set(ht.EDIT_KINDS) - kinds
    assert {st.op[1] for st in t if st.op[0] == "refused"} == set(ht.EDIT_REFUSALS)
    seen = ht.pairs_in(start, t)
    for a, b, why in ht.EDIT_RISKY_PAIRS:
        assert why
        assert (a, b) in seen, (a, b)     # (on a band context too: the band is set again BEHIND a resize, which stays the neighbour)
    # what the issue asks of the operations: both keep values, all four fold ops on a rectangle and on a byte mask, every kind of
    # edit with and without a pivot, show-all, overlay on / other options / outline on and off / off
    assert {st.op[1] for st in t if st.op[0] == "erase"} == {False, True}
    regions = {(st.op[2] is not None, st.op[3]) for st in t if st.op[0] == "select_region"}
    assert {op for _, op in regions} == set(ht.SELOPS) and {m for m, _ in regions} == {False, True}
    edits = {(st.op[1], st.op[3] is not None) for st in t if st.op[0] == "edit"}
    assert edits >= {("translate", False), ("rotate", False), ("rotate", True), ("scale", False), ("scale", True), ("rgba", False)}
    assert {st.op[1] for st in t if st.op[0] == "hide"} >= {"add", "subtract"}
    assert ("set_hidden", None, "replace") in [st.op for st in t]
    overlays = [st.op for st in t if st.op[0] == "overlay"]
    assert ("overlay", None) in overlays and {o[3] is not None for o in overlays if o[1] is not None} == {False, True}
    assert len({o[1:3] for o in overlays if o[1] is not None}) > 1
    # sizes and scenes stay small: four scene sizes from rows, at most 900 x 700 and one size above 4096 bins
    ns = {ht.scene_n(st.op[1]) for st in t if st.op[0] == "scene"}
    assert ns == {1, 33, 2049, 20000} and all(ht.scene_form(st.op[1]) == "rows" for st in t if st.op[0] == "scene")
    sizes = {(st.op[1], st.op[2]) for st in t if st.op[0] == "resize"}
    big = {z for z in sizes if z[0] > 900 or z[1] > 700}
    assert len(big) == 1 and ht.bins_of(*next(iter(big))) > 4096
    # unchecked steps keep the frame
    assert all(st.check or st.op[0] in ht.KEEPS_FRAME + ht.EDIT_KEEPS_FRAME for st in t)
    _assert_nothing_vacuous(start, t, oracle)
    # the one delivery that is refused by design is asked for, and one behind it is delivered again
    s, refused = start, []
    for st in t:
        if st.op[0] == "deliver":
            refused.append(ht.overlay_ring_refuses(s))
        s = ht.fold(s, st.op)
    assert True in refused and refused[refused.index(True) + 1] is False
    # duplicates on both sides of the capacity, and each on the side the trace says
    dups = _capacities(start, t, oracle)
    said = {i: st.op[1] for i, st in enumerate(t) if st.op[0] == "duplicate"}
    for i, n0, cap, n1 in dups:
        assert n1 > n0 and said[i] == ("fit" if n1 <= cap else "grow"), (i, n0, cap, n1, said[i])
    assert {"fit", "grow"} <= set(said.values())
    # past sort.rows (the largest count since the scene was set) and past a multiple of the 2048 keys of a radix block
    i = next(i for i, st in enumerate(t) if st.op[0] == "duplicate" and t[i + 1].op[0] == "sort_only")
    _, n0, _, n1 = next(d for d in dups if d[0] == i)
    assert n1 > n0 and n1 // 2048 > n0 // 2048 and n0 % 2048 and n1 % 2048


@pytest.mark.parametrize("seed,kind", EDIT_WALKS)
def test_every_editing_walk_holds_every_kind_and_stays_cheap(oracle, seed, kind):
    start = _start(kind, seed)
    t = _edit_walk(oracle, seed, kind)
    assert {st.op[0] for st in t} == set(ALL_KINDS), set(ALL_KINDS) ^ {st.op[0] for st in t}
    assert {st.op[1] for st in t if st.op[0] == "refused"} & set(ht.EDIT_REFUSALS)
    s = start
    for st in t:
        assert st.check or st.op[0] in ht.KEEPS_FRAME + ht.EDIT_KEEPS_FRAME
        if st.op[0] == "ring_overlay" and st.op[1]:
            assert s.ring is not None and s.overlay is not None
        if st.op[0] == "select_contrib":
            assert s.contrib                       # only where a pass has contributed
        s = ht.fold(s, st.op)
        assert s.W <= 900 and s.H <= 700
    _assert_nothing_vacuous(start, t, oracle)


def test_fold_is_pure_and_the_editing_tour_ends_where_it_says():
    s0 = ht.State(kind="throughput")
    t = ht.editing_tour()
    s = ht.fold_all(s0, t)
    assert ht.fold_all(s0, t) == s and s0 == ht.State(kind="throughput") and hash(s) == hash(ht.fold_all(s0, t))
    # by hand, for the tail: the last scene, a selection set on it, SH on and off again, three refusals and their cameras
    assert s.scene == ("synth", 2049, 6, "rows") and s.transforms == () and s.sh is None and s.pose == 70
    assert s.edits == (("set_selection", (15, 0.5), "replace"),)
    assert s.contrib is None and s.overlay is None and s.ring is None and s.ring_overlay is False and (s.W, s.H) == (640, 480)
    # the rules of the fold, one by one
    e = ("select_box", ht.BOX, "add")
    assert ht.fold(s, e).edits == s.edits + (e,)
    r = ht.fold(s, ("select_region", ht.RECT, None, "replace"))
    assert r.edits[-1] == ("select_region", ht.RECT, None, "replace", (70, 640, 480, None, (False, 0.0)))
    assert ht.fold(s, ("duplicate", "grow")).edits[-1] == ("duplicate",)
    assert ht.fold(s, ("reserve", 5000)) == s and ht.fold(s, ("refused", "edit_raw")) == s
    assert ht.fold(s, ("rotate", ht.QUAT)).edits[-1] == ("transform", "rotate", ht.QUAT) and ht.fold(s, ("rotate", ht.QUAT)).transforms == ()
    assert ht.fold(replace(s, edits=()), ("rotate", ht.QUAT)).transforms == (("rotate", ht.QUAT),)
    c = ht.fold(ht.fold(s, ("contrib_pass",)), ("contrib_pass",))
    assert c.contrib == ((70, 640, 480, None, (False, 0.0), 1),) * 2 and ht.fold(c, ("contrib_reset",)).contrib == ()
    for op in (("erase", False), ("limit_box", ht.BOX), ("scene", ("synth", 33, 1, "rows"))):
        assert ht.fold(c, op).contrib is None
    assert ht.fold(c, ("scene", ("synth", 33, 1, "rows"))).edits == ()
    o = ht.fold(s, ("overlay", (1.0, 0.5, 0.0), 0.5, None))
    assert o.overlay == ((1.0, 0.5, 0.0), 0.5, None) and ht.fold(o, ("overlay", None)).overlay is None
    g = ht.fold(ht.fold(o, ("ring_open", "rgba8", False, None, 1)), ("ring_overlay", True))
    assert g.ring_overlay and ht.fold(g, ("resize", 320, 200)).ring_overlay and not ht.fold(g, ("ring_close",)).ring_overlay
    # the ring's switch stays when the options go: the one State whose deliveries are refused, until options return
    off = ht.fold(g, ("overlay", None))
    assert off.ring_overlay and off.overlay is None and ht.overlay_ring_refuses(off) and not ht.overlay_ring_refuses(g)
    assert not ht.overlay_ring_refuses(ht.fold(off, ("overlay", (0.0, 0.0, 1.0), 1.0, None))) and not ht.overlay_ring_refuses(ht.fold(off, ("ring_overlay", False)))
    assert ht.fold(ht.fold(s, ("sh", (1, 0.0, 0.5, 0.5))), ("erase", True)).sh is None


def test_materialise_agrees_with_the_references_by_hand(oracle):
    import gsplat_hip as gh
    import edit_reference as er
    import hide_reference as hr
    import select_reference as sr
    import attr_reference as at
    s = ht.State(scene=("synth", 300, 7, "rows"), transforms=(("translate", (0.25, 0.0, -0.5)),), pose=9)
    ops = [("select_box", tuple(v * 0.5 for v in ht.BOX), "replace"), ("edit", "rotate", ht.QUAT, ht.PIVOT), ("hide", "add"),
           ("select_attr", "opacity", 0.0, 128.0, None, "replace"), ("select_region", ht.RECT, None, "add"), ("duplicate", None),
           ("edit", "rgba", (0x11223344, 0x00ff00ff), None), ("append_arrays", 5, 3), ("invert_selection",), ("scale", (1.0, 2.0, 1.0)),
           ("erase", True), ("set_hidden", (4, 0.5), "subtract"), ("select_hidden", "replace")]
    m = ht.materialise(ht.fold_ops(s, ops), oracle)
    # the same chain, written out
    st = oracle.SceneState(gh.synth.synth_rows(300, 7))
    st.translate((0.25, 0.0, -0.5))
    S = sr.box_pick(st.positions, tuple(v * 0.5 for v in ht.BOX))
    assert 0 < S.sum() < 300
    er.apply(st, S, "rotate", ht.QUAT, ht.PIVOT)
    H = hr.hide_selected(np.zeros(300, bool), S, "add")
    S = at.select(at.attr_value("opacity", data=st.data), 0.0, 128.0)
    cam = gh.orbit_camera(9, 120, 640, 480, fx=0.59 * 640)
    v, p, _ = cam.f32()
    rec, bbox, _ = oracle.project(st.data, v, p, cam.fx, cam.fy, 640, 480)
    P = sr.centre_pick(rec, hr.hide_bbox(bbox, H), ht.RECT)
    assert P.any() and not (P & H).any()
    S = S | P
    k = int(S.sum())
    first, count = append_reference.duplicate(st, S)
    assert (first, count) == (300, k)
    S, H = append_reference.selection_after(st.n, first, count), append_reference.hidden_after(H, count)
    er.paint(st, S, 0x11223344, 0x00ff00ff)
    add = oracle.SceneState(gh.synth.synth_rows(5, 3))
    first, count = append_reference.append_arrays(st, add.data, add.positions, add.rotations, add.scales)
    S, H = append_reference.selection_after(st.n, first, count), append_reference.hidden_after(H, count)
    S = ~S
    st.scale((1.0, 2.0, 1.0))
    H = hr.compact(H, S)
    append_reference.erase(st, ~S)
    S = np.zeros(st.n, bool)
    H = hr.hidden_set(H, np.random.default_rng(4).random(st.n) < 0.5, "subtract")
    S = hr.select_hidden(S, H, "replace")
    assert st.n == 300 + k and m.n == st.n and H.any()
    for name in ("data", "positions", "rotations", "scales"):
        a, b = getattr(m, name), getattr(st, name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    assert np.array_equal(m.selection_words, sr.pack(S)) and np.array_equal(m.hidden_words, sr.pack(H))
    # memoised on the prefixes: a longer recipe starts from this one, and the cached value is not the caller's to change
    m.data[:] = 0
    assert np.array_equal(ht.materialise(ht.fold_ops(s, ops), oracle).data.view(np.uint32), st.data.view(np.uint32))
    # without edits: the scene as it is set
    m0 = ht.materialise(ht.State(scene=("synth", 33, 2, "rows")), oracle)
    assert m0.n == 33 and not m0.selection_words.any() and not m0.hidden_words.any()
    assert np.array_equal(m0.data, oracle.SceneState(gh.synth.synth_rows(33, 2)).data)


def test_the_final_state_is_the_fold_of_the_operations():
    s0 = ht.State(kind="throughput")
    t = ht.tour()
    s = s0
    for st in t:
        s = ht.fold(s, st.op)
    assert ht.fold_all(s0, t) == s and s.kind == "throughput" and s.knobs == s0.knobs
    # by hand, for the tail of the tour: the last ring was closed, the SH spec set before the refusals survives them
    assert s.ring is None and s.sh == (14, 0.0, 0.25, 0.5) and s.pose == 53 and (s.W, s.H) == (640, 480) and s.band is None
    assert s.scene == ("synth", 70000, 4, "rows") and s.transforms == () and s.fade == (False, 0.0) and s.hit_alpha == 0.25
    # operations that observe change nothing
    for op in (("same_pose",), ("sort_only", 2, 5), ("readback", "records"), ("depth_async", True), ("timing_interval", 3),
               ("overflow_sync", 1024), ("deliver",), ("refused", "size_zero")):
        assert ht.fold(s, op) == s
    # and the ones with side conditions
    assert ht.fold(s, ("band", 608, 10000)).band == (608, 640)
    assert ht.fold(ht.fold(s, ("band", 64, 128)), ("resize", 320, 200)).band is None
    assert ht.fold(ht.fold(s, ("sh", (1, 0.0, 0.5, 0.5))), ("limit_box", ht.BOX)).sh is None
    assert ht.fold(s, ("scene", ("synth", 5, 1, "raw"))).sh is None


# ---------------------------------------------------------------------------------------------------------------------------
# the analysis layer
# ---------------------------------------------------------------------------------------------------------------------------
ANALYSIS_WALKS = [(seed, kind) for seed in (7, 14, 21) for kind in ("default", "throughput")]   # tests/test_gpu_history.py::test_analysis_walks
ANALYSIS_WALK_STEPS = 180
EVERY_KIND = ht.KINDS + ht.EDIT_KINDS + ht.ANALYSIS_KINDS
KEEPS = ht.KEEPS_FRAME + ht.EDIT_KEEPS_FRAME + ht.ANALYSIS_KEEPS_FRAME
_analysis_walks = {}


def _analysis_walk(oracle, seed, kind):
    if (seed, kind) not in _analysis_walks:
        _analysis_walks[seed, kind] = ht.walk(seed, ANALYSIS_WALK_STEPS, _start(kind, seed), kinds=EVERY_KIND, oracle=oracle)
    return _analysis_walks[seed, kind]


def _radius_of(op):
    """the radius or cell side of an analysis operation (None: another operation)"""
    return op[2] if op[0] == "report" else op[1] if op[0] in ht.ANALYSIS_KINDS else None


def _assert_analysis_steps_are_sound(start, trace, oracle):
    """on top of _assert_nothing_vacuous: every analysis step runs on a rows scene the CPU fold can afford (a picker and three of the
    reports also on a raw one), every merge merges, and a merge never meets live accumulators in a walk"""
    s = start
    for i, st in enumerate(trace):
        if st.op[0] in ht.ANALYSIS_KINDS:
            n = ht.materialise(s, oracle).n
            assert 1 <= n <= ht.MAX_ANALYSED, (i, st.op, n)
        if st.op[0] == "merge_cells":
            assert ht.scene_form(s.scene) == "rows" and s.sh is None, (i, st.op)
            n1 = ht.materialise(ht.fold(s, st.op), oracle).n
            assert 2 <= n1 < n, (i, st.op, n, n1)
        s = ht.fold(s, st.op)


def test_the_analysis_builders_are_deterministic(oracle):
    assert ht.analysis_tour() == ht.analysis_tour() and ht.analysis_tour(True) == ht.analysis_tour(True)
    for seed, kind in ANALYSIS_WALKS[:2]:
        a = _analysis_walk(oracle, seed, kind)
        assert len(a) == ANALYSIS_WALK_STEPS and a == ht.walk(seed, ANALYSIS_WALK_STEPS, _start(kind, seed), kinds=EVERY_KIND, oracle=oracle)
        assert ht.walk(seed, 53, _start(kind, seed), kinds=EVERY_KIND, oracle=oracle) == a[:53]
    assert _analysis_walk(oracle, 7, "default") != _analysis_walk(oracle, 14, "default")


@pytest.mark.parametrize("band_context", [False, True])
def test_the_analysis_tour_holds_every_kind_refusal_and_pair(oracle, band_context):
    start = ht.State(band=(192, 448) if band_context else None)
    t = ht.analysis_tour(band_context)
    ops = [st.op for st in t]
    kinds = {op[0] for op in ops}
    assert set(ht.ANALYSIS_KINDS) <= kinds <= set(EVERY_KIND), set(ht.ANALYSIS_KINDS) - kinds
    assert {op[1] for op in ops if op[0] == "refused"} == set(ht.ANALYSIS_REFUSALS)
    assert {op[1] for op in ops if op[0] == "report"} == set(ht.REPORTS)
    seen = ht.pairs_in(start, t)
    for a, b, why in ht.ANALYSIS_RISKY_PAIRS:
        assert why
        assert (a, b) in seen, (a, b)
    # every refusal is followed by a camera
    for i, op in enumerate(ops):
        if op[0] == "refused":
            assert ops[i + 1][0] == "camera", op
    # the pickers with every scope and every fold op between them, each under more than one scope; the merge and the reports with
    # every scope; both kinds of seed
    for kind in ht.ANALYSIS_PICKERS:
        assert len({op[-2] for op in ops if op[0] == kind}) >= 2, kind
    assert {op[-1] for op in ops if op[0] in ht.ANALYSIS_PICKERS} == set(ht.SELOPS)
    assert {op[-2] for op in ops if op[0] in ht.ANALYSIS_PICKERS} == set(ht.SCOPES)
    assert {op[2] for op in ops if op[0] == "merge_cells"} == set(ht.SCOPES)
    assert {op[-1] for op in ops if op[0] == "report"} == set(ht.SCOPES)
    seeds = {op[2] for op in ops if op[0] == "select_cluster_at"}
    assert "largest" in seeds and any(isinstance(x, int) for x in seeds)
    assert {op[3] for op in ops if op[0] == "select_knn"} == {"kth", "mean"}
    # the statistical outlier filter: select_knn with a constant threshold and no upper end, then erase
    assert any(a[0] == "select_knn" and a[5] is None and a[4] > 0 and b == ("erase", False) for a, b in zip(ops, ops[1:]))
    # the triple ring_overlay -> merge -> deliver, and a merge at a larger cell directly behind a merge
    assert any(a == ("ring_overlay", True) and b[0] == "merge_cells" and c == ("deliver",) for a, b, c in zip(ops, ops[1:], ops[2:]))
    assert any(a[0] == b[0] == "merge_cells" and b[1] > a[1] for a, b in zip(ops, ops[1:]))
    # neighbouring analysis calls of different features never share a radius: an index kept from the call before is the wrong one
    # (a report and the pickers or the edit of its feature are one feature: the cells report announces the merge at the same side)
    family = {"select_neighbours": "neighbours", "select_clusters": "clusters", "select_cluster_at": "clusters", "select_knn": "knn", "merge_cells": "cells"}
    feature = lambda op: op[1] if op[0] == "report" else family[op[0]]
    calls = [op for op in ops if _radius_of(op) is not None]
    for a, b in zip(calls, calls[1:]):
        if feature(a) != feature(b):
            assert _radius_of(a) != _radius_of(b), (a, b)
    # ... and one feature twice in a row at ONE radius under another scope, no frame in between: an index kept for its radius is wrong
    i = next(i for i, op in enumerate(ops) if op[:2] == ("report", "neighbours") and ops[i + 1][0] == "select_neighbours")
    assert _radius_of(ops[i]) == _radius_of(ops[i + 1]) and ops[i][-1] != ops[i + 1][-2] and not t[i].check
    # the scenes: rows of a few thousand splats, more than one workgroup of 256 and a partial last wave of 64 each
    ns = [ht.scene_n(op[1]) for op in ops if op[0] == "scene"]
    assert set(ns) == {2049, 4099, 2601, 6001} and all(n > 256 and n % 64 for n in ns)
    assert all(ht.scene_form(op[1]) == "rows" for op in ops if op[0] == "scene")
    sizes = {(op[1], op[2]) for op in ops if op[0] == "resize"}
    assert all(w <= 900 and hgt <= 700 for w, hgt in sizes)
    # unchecked steps keep the frame: a merge never goes unchecked
    assert all(st.check or st.op[0] in KEEPS for st in t)
    _assert_nothing_vacuous(start, t, oracle)
    _assert_analysis_steps_are_sound(start, t, oracle)
    # the scratch sizing paths, by the counts: a merge of a larger scene than any before (both shares grow), one of a smaller scene
    # (scratch larger than the scene), a duplicate past the largest merged count followed by a merge, and a cells report of a count no
    # merge has seen (the edit's share is behind)
    s, merged_max, reported_max, paths = start, 0, 0, set()
    for i, st in enumerate(t):
        n = ht.materialise(s, oracle).n
        if st.op[0] == "report" and st.op[1] == "cells":
            reported_max = max(reported_max, n)
        if st.op[0] == "merge_cells":
            if merged_max and n > merged_max:
                paths.add("grown by the report" if reported_max >= n else "grown")
                if t[i - 1].op[0] == "duplicate":
                    paths.add("grown by a duplicate")
            if n < merged_max:
                paths.add("smaller")
            merged_max = max(merged_max, n)
        s = ht.fold(s, st.op)
    assert paths == {"grown", "grown by the report", "grown by a duplicate", "smaller"}, paths
    # duplicates on the side of the capacity the trace says
    dups = _capacities(start, t, oracle)
    said = {i: st.op[1] for i, st in enumerate(t) if st.op[0] == "duplicate"}
    for i, n0, cap, n1 in dups:
        assert n1 > n0 and said[i] == ("fit" if n1 <= cap else "grow"), (i, n0, cap, n1, said[i])
    assert {"fit", "grow"} <= set(said.values())


@pytest.mark.parametrize("seed,kind", ANALYSIS_WALKS)
def test_every_analysis_walk_holds_every_kind_and_stays_cheap(oracle, seed, kind):
    start = _start(kind, seed)
    t = _analysis_walk(oracle, seed, kind)
    assert {st.op[0] for st in t} == set(EVERY_KIND), set(EVERY_KIND) ^ {st.op[0] for st in t}
    refused = {st.op[1] for st in t if st.op[0] == "refused"}
    assert refused & set(ht.EDIT_REFUSALS) and refused & set(ht.ANALYSIS_REFUSALS)
    s = start
    for i, st in enumerate(t):
        assert st.check or st.op[0] in KEEPS
        if st.op[0] == "merge_cells":
            assert not s.contrib, i                # the walks reset the accumulators in front of a merge
        s = ht.fold(s, st.op)
        assert s.W <= 900 and s.H <= 700
    _assert_nothing_vacuous(start, t, oracle)
    _assert_analysis_steps_are_sound(start, t, oracle)


def test_fold_is_pure_for_the_analysis_layer():
    s0 = ht.State(kind="throughput")
    t = ht.analysis_tour()
    s = ht.fold_all(s0, t)
    assert ht.fold_all(s0, t) == s and s0 == ht.State(kind="throughput") and hash(s) == hash(ht.fold_all(s0, t))
    # the tail by hand: the last refusal's camera, SH rows set for merge_with_sh and left on, ring and overlay closed
    assert s.pose == 70 + len(ht.ANALYSIS_REFUSALS) - 1 and s.sh == (11, 0.0, 0.25, 0.5) and s.ring is None and s.overlay is None and s.contrib is None
    assert s.scene == ("synth", 2049, 5, "rows") and s.edits[-1][0] == "merge_cells"
    # the rules, one by one
    s = ht.State(scene=("synth", 2049, 5, "rows"), sh=(1, 0.0, 0.5, 0.5), contrib=((1, 640, 480, None, (False, 0.0), 0),))
    for op in (("select_neighbours", 0.3, 1, None, 8, ("visible",), "add"), ("select_clusters", 0.3, 0, 2, 1, (), "replace"),
               ("select_cluster_at", 0.3, "largest", 0, ("selected",), "subtract"), ("select_knn", 0.3, 4, "mean", 0.0, None, (), "intersect")):
        assert ht.fold(s, op) == replace(s, edits=(op,))                       # a picker joins the recipe and touches nothing else
    m = ("merge_cells", 0.25, ("selected", "visible"))
    assert ht.fold(s, m) == replace(s, edits=(m,), sh=None, contrib=None)      # as a removing erase
    for which, args in (("neighbours", (0.3, 8, ())), ("clusters", (0.3, 0, ())), ("knn", (0.3, 4, "kth", ())), ("cells", (0.3, 8, ()))):
        assert ht.fold(s, ("report", which) + args) == s
    for which in ht.ANALYSIS_REFUSALS:
        assert ht.fold(s, ("refused", which)) == s
    # the tags the pairs are written in
    assert ht.tags(m, s) == {"merge_cells", "merge"} and "select" in ht.tags(("select_knn", 0.3, 4, "mean", 0.0, None, (), "add"), s)
    assert ht.tags(("report", "cells", 0.3, 8, ()), s) == {"report", "report:cells"}
    assert ht.scope_mask((), np.array([1, 0], bool), np.array([0, 1], bool)).tolist() == [True, True]
    assert ht.scope_mask(("selected", "visible"), np.array([1, 1, 0], bool), np.array([0, 1, 0], bool)).tolist() == [True, False, False]


def test_materialise_agrees_with_the_four_references_by_hand(oracle):
    import gsplat_hip as gh
    import cluster_reference as cr
    import knn_reference as kr
    import merge_reference as mr
    import neighbour_reference as nr
    import select_reference as sr
    base = ht.State(scene=("synth", 33, 2, "rows"))
    rows = oracle.SceneState(gh.synth.synth_rows(33, 2))
    pos0 = rows.positions.reshape(-1, 3).copy()
    # two splats i < j, each with a copy exactly on it: rows 33 and 34
    spec = next((seed, 0.06) for seed in range(1, 500) if ht.spec_set((seed, 0.06), 33).sum() == 2)
    i, j = np.flatnonzero(ht.spec_set(spec, 33)).tolist()
    two = [("set_selection", spec, "replace"), ("duplicate", None)]
    m = ht.materialise(ht.fold_ops(base, two), oracle)
    assert m.n == 35 and sr.unpack(m.selection_words, 35).nonzero()[0].tolist() == [33, 34]
    # select_cluster_at("largest") on a tie: two clusters of two at a radius only coincident splats share -- the smallest label wins
    tie = two + [("select_cluster_at", ht.COINCIDENT, "largest", 0, (), "replace")]
    c = cr.Clusters(m.positions, ht.COINCIDENT, 0)
    # (with min_pts 0 every splat is core: 31 clusters of one and the two of two)
    assert c.info["clusters"] == 33 and c.info["largest_size"] == 2 and c.info["largest_label"] == i
    assert np.flatnonzero(c.sizes == 2).tolist() == [i, j, 33, 34] and c.labels[[i, j, 33, 34]].tolist() == [i, j, i, j]
    assert sr.unpack(ht.materialise(ht.fold_ops(base, tie), oracle).selection_words, 35).nonzero()[0].tolist() == [i, 33]
    # ... and with an index seed, the other one
    at_j = two + [("select_cluster_at", ht.COINCIDENT, 34, 0, (), "replace")]
    assert sr.unpack(ht.materialise(ht.fold_ops(base, at_j), oracle).selection_words, 35).nonzero()[0].tolist() == [j, 34]
    # two coincident splats merging: both pairs become one row each, at their leaders; the selection is exactly the merged rows; the
    # mean of two equal positions is that position, bit for bit; every other row keeps its bits
    both = ht.materialise(ht.fold_ops(base, two + [("merge_cells", ht.COINCIDENT, ())]), oracle)
    assert both.n == 33 and sr.unpack(both.selection_words, 33).nonzero()[0].tolist() == [i, j] and not both.hidden_words.any()
    assert np.array_equal(both.positions.view(np.uint32), rows.positions.view(np.uint32))
    others = np.setdiff1d(np.arange(33), [i, j])
    for name, k in (("data", 8), ("rotations", 4), ("scales", 3)):
        assert np.array_equal(getattr(both, name).reshape(-1, k)[others].view(np.uint32), getattr(rows, name).reshape(-1, k)[others].view(np.uint32)), name
    want = mr.merge(m.data, m.positions, m.rotations, m.scales, ht.COINCIDENT)
    assert want["info"]["merged_cells"] == 2 and want["info"]["rows_after"] == 33
    for name in ("data", "positions", "rotations", "scales"):
        assert np.array_equal(getattr(both, name).view(np.uint32), np.ascontiguousarray(want[name]).reshape(-1).view(np.uint32)), name
    # a hidden member under scope visible: j and its copy are hidden, so only i's cell merges, and the hidden bits are carried to the
    # new numbering (row 34 becomes row 33); under scope () the hidden pair merges too and the leader keeps its bit
    hide_j = two + [("select_cluster_at", ht.COINCIDENT, j, 0, (), "replace"), ("hide", "add")]
    vis = ht.materialise(ht.fold_ops(base, hide_j + [("merge_cells", ht.COINCIDENT, ("visible",))]), oracle)
    assert vis.n == 34 and sr.unpack(vis.selection_words, 34).nonzero()[0].tolist() == [i]
    assert sr.unpack(vis.hidden_words, 34).nonzero()[0].tolist() == [j, 33]
    assert np.array_equal(vis.positions.reshape(-1, 3)[33].view(np.uint32), pos0[j].view(np.uint32))
    every = ht.materialise(ht.fold_ops(base, hide_j + [("merge_cells", ht.COINCIDENT, ())]), oracle)
    assert every.n == 33 and sr.unpack(every.selection_words, 33).nonzero()[0].tolist() == [i, j] and sr.unpack(every.hidden_words, 33).nonzero()[0].tolist() == [j]
    # scope "selected" with nothing to merge among the selected: nothing changes, the selection included
    nothing = ht.materialise(ht.fold_ops(base, hide_j + [("merge_cells", ht.COINCIDENT, ("selected", "visible"))]), oracle)
    before = ht.materialise(ht.fold_ops(base, hide_j), oracle)
    assert nothing.n == 35 and all(np.array_equal(a, b) for a, b in zip(nothing, before) if isinstance(a, np.ndarray))
    # the three other pickers, written out with their references on a larger scene, scopes from S and H
    s = ht.State(scene=("synth", 300, 7, "rows"))
    st = oracle.SceneState(gh.synth.synth_rows(300, 7))
    h = ht.analysis_spacing(300)
    S, H = ht.spec_set((3, 0.6), 300), ht.spec_set((4, 0.3), 300)
    ops = [("set_selection", (3, 0.6), "replace"), ("set_hidden", (4, 0.3), "replace")]
    cases = [(("select_neighbours", 1.2 * h, 1, None, 4, ("visible",), "replace"),
              lambda mk: nr.select(nr.counts(st.positions, 1.2 * h, 4, mk), 1, 5, mk)),
             (("select_clusters", 1.1 * h, 2, None, 1, ("selected",), "replace"),
              lambda mk: cr.select(cr.Clusters(st.positions, 1.1 * h, 1, mk).sizes, 2, 0xffffffff, mk)),
             (("select_knn", 1.5 * h, 2, "kth", 0.0, 1.3 * h, ("selected", "visible"), "replace"),
              lambda mk: kr.select(kr.values(*kr.lists(st.positions, 1.5 * h, 2, mk)[::2], 2, "kth", mk), 0.0, 1.3 * h, mk)),
             (("select_knn", 1.5 * h, 3, "mean", 1.0 * h, None, (), "replace"),
              lambda mk: kr.select(kr.values(*kr.lists(st.positions, 1.5 * h, 3, mk)[::2], 3, "mean", mk), 1.0 * h, np.inf, mk))]
    for op, want in cases:
        mk = ht.scope_mask(op[-2], S, H)
        P = want(mk)
        assert 0 < P.sum() < mk.sum() and not (P & ~mk).any(), op
        got = ht.materialise(ht.fold_ops(s, ops + [op]), oracle)
        assert np.array_equal(got.selection_words, sr.pack(P)), op
        assert np.array_equal(got.hidden_words, sr.pack(H)) and got.n == 300
    # the other fold ops go through select_reference.apply_op like every picker's
    op = ("select_neighbours", 1.2 * h, 1, None, 4, ("visible",), "subtract")
    got = ht.materialise(ht.fold_ops(s, ops + [op]), oracle)
    assert np.array_equal(got.selection_words, sr.pack(S & ~cases[0][1](~H)))

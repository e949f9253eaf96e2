"""The traces of tests/history_trace.py, checked without a GPU: the builders are deterministic, the tour holds every operation,
read-back, refusal and risky pair, every random walk the GPU tests use holds every kind of operation, and the State a trace ends
in is the fold of its operations."""
import pytest

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

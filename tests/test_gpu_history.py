"""A long-lived context renders every frame as a fresh one.

A gsr_ctx carries a lot from frame to frame -- frame slots "left clean by their last reader", the sort order chosen from the
previous frame's bucket report, a captured graph with one rewritten node, buffers that grow and never shrink, rectangles and
packed depth slots a band frame writes for survivors only, cached depth planes, a delivery ring that survives a resize.  The
claim ("Frame-to-frame state") is that every observable of a frame depends on the State (tests/history_trace.py)
and on nothing the context did before.  So: one veteran context walks a trace; after every checked step it renders the step's
pose, a context created a moment ago from the State alone renders the same pose once, and everything the two can be asked
is compared BIT FOR BIT.  No tolerance: a wrong entry in one bin list shows.  (Veteran and fresh could be wrong together: the
random walks also meet the CPU oracle every tenth step.)"""
import ctypes
import os
from dataclasses import replace

import numpy as np
import pytest

import hide_reference
import history_trace as ht
import select_reference
import work_items_reference

pytestmark = pytest.mark.gpu

TOL_EXACT = 2e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
ANALYSIS_UNITS = ("merge", "neighbours", "knn", "clusters", "attr")      # the observables run these kernels on every trace
BOUNDS_UNITS = ("blend", "bin", "sort", "depth", "deliver") + ANALYSIS_UNITS

# The only things a veteran and a fresh context may disagree on: what counts frames, deliveries or time.
#   gsr_timings: everything but these four describes the context's life, not the frame
FRAME_STATS = ("visible", "bin_entries", "tile_entries", "n")
#   a delivered frame's trailer is (overflow word, dims, serial low, serial high): the serial counts deliveries
TRAILER_FRAME_WORDS = 2
#   and the serial gsr_deliver_frame_async / gsr_acquire_frame return (never compared)
#   scene_capacity() and the byte count of scene_sharing() depend on the context's life BY RULE ("Growing the scene"): the
#   arrays grow to max(need, capacity + capacity / 2) and never shrink, a compaction keeps the old count's rows, and the selection,
#   hidden and contribution buffers are counted once they exist -- a veteran that grew, reserved or showed everything again holds
#   more than a context that was handed the final scene
#   pair_bound of the four analysis infos is "the pair tests the walk makes at most, AS THE IMPLEMENTATION COUNTS THEM" (include/gsplat_hip.h,
#   "neighbours": the populations of hash buckets, whose number the header leaves to the implementation): a context may size its table
#   by its scratch, which only grows.  The feature suites bound it by an interval (pair_floor <= pair_bound <= budget); every other
#   field of the infos is defined by the scene and the arguments and is compared
NOT_COMPARED = ("scene_capacity()", "scene_sharing() bytes", "pair_bound")
# The analysis observables are asked while the scene holds at most this many splats: every scene of the editing and analysis traces
# (history_trace.MAX_GROWN) and of the walks.  tour()'s scenes of 70 000 .. 3.2 M splats are left to the observables they always had.
ANALYSIS_OBSERVED_MAX = 40000
assert ANALYSIS_OBSERVED_MAX >= ht.MAX_GROWN


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.fields else a.view(np.dtype("u%d" % a.dtype.itemsize)) if a.dtype.kind == "f" else a


def _same(a, b):
    """bit for bit (NaNs and signed zeros included)"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
    return a == b


def _deliver(r):
    """the frame enqueued last through the open ring: (payload planes, depth plane | None, the trailer's frame words)"""
    k = r.deliver()
    got = r.acquire(k)
    assert got[0] == k
    planes = got[1] if isinstance(got[1], tuple) else (got[1],)
    lay = r.delivery_layout()
    off = (lay["bytes"] + 3) & ~3
    depth = None
    if len(got) == 3:
        dl = r.depth_layout()
        off = (dl["offset"] + dl["bytes"] + 15) & ~15
        depth = np.array(got[2])
    trailer = np.array((ctypes.c_uint32 * 4).from_address(planes[0].ctypes.data + off))
    out = (tuple(np.array(p) for p in planes), depth, trailer[:TRAILER_FRAME_WORDS].copy())
    r.release(k)
    return out


def observe(r, state, points=None):
    """Everything the finished frame can be asked, in an order every answer survives (a band context sorts the whole permutation on
    demand for keys / depthIndex, which makes the frame enqueued last a sort-only one: planes and picks are asked first)."""
    o = {}
    if ht.overlay_ring_refuses(state):       # (the one delivery that is refused by design: it takes no slot, and says why)
        import gsplat_hip
        o["delivery refused"] = ht.deliver_refused(gsplat_hip, r)
    elif state.ring is not None:
        o["delivered payload"], o["delivered depth plane"], o["delivered trailer (overflow word, dims)"] = _deliver(r)
    img = r.readPixelsFloat()
    o["f32 image"] = img
    o["RGBA8 image"] = r.readPixels()
    o["depth planes (mean, hit, index)"] = r.read_depth()
    if points is None:      # fixed pixels, and the pixels of largest alpha
        W, H = state.W, state.H
        top = np.argpartition(img[:, :, 3].reshape(-1), -8)[-8:]
        points = [(0, 0), (W - 1, H - 1), (W // 2, H // 2), (W // 3, 2 * H // 3), (min(W - 1, 33), min(H - 1, 31))] + [(int(p % W), int(p // W)) for p in top]
        points = [ht.into_band(state, x, y) for x, y in points]
    o["pick points"] = points
    o["pick()"] = r.pick(points)
    if state.overlay is not None:       # (the pass walks this frame's lists: asked while the frame enqueued last is a render frame)
        o["read_overlay() (rgba, cover)"] = r.read_overlay()
        o["read_overlay_rgba8()"] = r.read_overlay_rgba8()
    starts, lst = r.bin_lists()
    o["bin starts"], o["bin list entries"] = starts, lst
    o["work_items()"] = r.work_items()
    # the work list itself: the order inside a size class is the atomics' (k_bin_finalize), everything else is the frame's
    items, seg_start = r.work_list(max(o["work_items()"]["items"], 1))
    o["work list (items sorted inside their class)"], o["seg_start"] = work_items_reference.canonical(items), seg_start
    o["frame figures"] = tuple(sorted(r.frame_figures().items()))
    rec, bbox = r.read_records()
    o["pixel boxes"] = bbox
    # (a record is defined for the splats the projection draws: k_project_key writes nothing for a culled splat, and nothing reads it)
    o["records of drawn splats"] = rec[bbox[:, 0] <= bbox[:, 2]]
    st = r.stats()
    o["stats " + "/".join(FRAME_STATS)] = tuple(int(st[k]) for k in FRAME_STATS)
    keys, mm = r.read_keys()
    o["keys"], o["key (min, max)"] = keys, mm
    o["depthIndex"] = r.lastDepthIndex()
    # the scene and the sets that are held with it
    o["scene_count()"] = r.scene_count()
    o["read_scene() (data, positions, rotations, scales)"] = r.read_scene(with_rows=ht.scene_form(state.scene) == "rows")
    o["selection words"], o["selection count"] = r.selection_words(), r.selection_count()
    o["hidden words"], o["hidden count"] = r.hidden_words(), r.hidden_count()
    count, lo, hi = r.selection_bounds()         # (values, not bits: which of -0.0 and +0.0 a bound holds is not defined)
    o["selection_bounds()"] = (count, tuple(float(v) for v in lo), tuple(float(v) for v in hi))
    if state.contrib is not None:
        o["read_contrib() (weight, peak, pixels, frames)"] = r.read_contrib()
    o["attr_histogram(opacity, visible and selected)"] = r.attr_histogram("opacity", 0.0, 256.0, 16, selected=True, visible=True)[:2]
    o["attr_stats(opacity, visible and selected)"] = r.attr_stats("opacity", selected=True, visible=True)
    # the analysis calls, over the one neighbour scratch and index the veteran's earlier calls left behind: parameters from the scene's
    # own spacing (history_trace.analysis_spacing), the scope that ties them to both sets wherever both are non-empty
    n = o["scene_count()"]
    if n <= ANALYSIS_OBSERVED_MAX:
        h = ht.analysis_spacing(n)
        scope = ("selected", "visible") if o["selection count"] and o["hidden count"] else ()
        counts, hist, info = r.neighbours(1.1 * h, 16, scope)
        o["neighbours() counts"], o["neighbours() hist"], o["neighbours() info"] = counts, hist, _info(info)
        labels, sizes, info = r.clusters(1.3 * h, 2, scope)
        o["clusters() labels"], o["clusters() sizes"], o["clusters() info"] = labels, sizes, _info(info)
        found, _, _, values, _, info = r.knn(1.6 * h, 4, "mean", scope, hist=False)
        o["knn() found"], o["knn() values"], o["knn() info"] = found, values, _info(info)
        if ht.scene_form(state.scene) == "rows" or not n:       # (cells are of rotations and scales too: a raw scene has none)
            leader, hist, info = r.cells(0.9 * h, 8, scope, leaders=True)
            o["cells() leader"], o["cells() hist"], o["cells() info"] = leader, hist, _info(info)
    return o


def _info(info):
    """an analysis call's info without NOT_COMPARED's field"""
    return tuple(sorted((k, v) for k, v in info.items() if k != "pair_bound"))


def _render(gh, r, state):
    ht._frame(gh, r, state, sync=True)


def compare_with_fresh(gh, vet, state, where, lib_path=None):
    """the veteran's frame of `state` against the frame of a context that has done nothing else; returns the veteran's observables"""
    _render(gh, vet, state)
    a = observe(vet, state)
    fresh = ht.build(gh, state, lib_path)
    try:
        _render(gh, fresh, state)
        b = observe(fresh, state, a["pick points"])
    finally:
        fresh.dispose()
    assert list(a) == list(b)
    for name in a:
        if not _same(a[name], b[name]):
            detail = ""
            x, y = a[name], b[name]
            if isinstance(x, tuple) and x and isinstance(x[0], np.ndarray):      # (planes: name the first one that differs)
                k = [_same(u, v) for u, v in zip(x, y)].index(False)
                x, y, detail = x[k], y[k], " in part %d" % k
            if isinstance(x, np.ndarray) and x.shape == y.shape and x.dtype.fields is None:
                bad = np.flatnonzero(_bits(x).reshape(-1) != _bits(y).reshape(-1))
                detail += ": %d of %d elements differ, first at %d (veteran %r, fresh %r)" % (bad.size, x.size, bad[0], x.reshape(-1)[bad[0]], y.reshape(-1)[bad[0]])
            elif isinstance(x, np.ndarray):
                detail += ": shapes %r and %r" % (x.shape, y.shape)
            else:
                detail += ": veteran %r, fresh %r" % (x, y)
            raise AssertionError("%s: the veteran's %s differs from a fresh context's%s" % (where(), name, detail))
    return a


def meet_oracle(gh, O, vet, state, a, where):
    """depthIndex exact, the band's columns of the image within TOL_EXACT: veteran and fresh are not wrong together.  And the scene,
    the selection and the hidden set the veteran holds are the recipe's, evaluated on the CPU: bit for bit."""
    rows = ht.scene_form(state.scene) == "rows"
    data, pos, rot, scl = a["read_scene() (data, positions, rotations, scales)"]
    n = pos.size // 3
    m = ht.materialise(state, O)
    assert n == m.n == a["scene_count()"], "%s: %d splats, the recipe leaves %d" % (where(), n, m.n)
    want = (m.data, m.positions, m.rotations, m.scales)
    if not rows:      # (a raw scene takes pickers and hides only: its arrays are the upload's)
        _, up_data, up_pos = ht.scene_arrays(gh, state.scene)
        want = (np.ascontiguousarray(up_data[:8 * n]), np.ascontiguousarray(up_pos[:3 * n]), None, None)
    for name, x, y in zip(("data", "positions", "rotations", "scales"), (data, pos, rot, scl), want):
        assert _same(x, y), "%s: the veteran's %s differ from the recipe's" % (where(), name)
    assert _same(a["selection words"], m.selection_words), "%s: the selection differs from the recipe's" % where()
    assert _same(a["hidden words"], m.hidden_words), "%s: the hidden set differs from the recipe's" % where()
    cam = ht.camera_of(gh, state)
    v, p, vp = cam.f32()
    sh = bidx = None
    if state.sh is not None:
        tex, b = ht.sh_arrays(gh, state.sh, n)
        if n - (int(b[0]) + 1) > 0:
            sh, bidx = tex, b
    # the oracle's frame with the hidden splats' boxes made invisible (hide_reference: they are still sorted)
    odi, _, _ = O.sort(vp, pos)
    rec, bbox, raw = O.project(data, v, p, cam.fx, cam.fy, state.W, state.H, sh, bidx, state.fade[1] if state.fade[0] else None)
    bbox = hide_reference.hide_bbox(bbox, select_reference.unpack(m.hidden_words, n))
    oimg = O.render(odi, raw, rec, bbox, state.W, state.H, 1)
    assert np.array_equal(a["depthIndex"], odi), "%s: depthIndex differs from the oracle" % where()
    x0, x1 = (state.band[0] // 32 * 32, min(-(-state.band[1] // 32) * 32, state.W)) if state.band else (0, state.W)
    img = a["f32 image"]
    err = float(np.abs(img[:, x0:x1].astype(np.float64) - oimg[:, x0:x1]).max()) if x1 > x0 else 0.0
    assert err <= TOL_EXACT, "%s: image differs from the oracle by %g" % (where(), err)
    assert not img[:, :x0].any() and not img[:, x1:].any(), "%s: pixels outside the band" % where()


def run_trace(gh, trace, start, label, lib_path=None, oracle=None, oracle_every=10):
    """One veteran context through the trace; returns (checked steps, the library the contexts came from)."""
    def where():
        return "%s, step %d (%s) -- replay: %s" % (label, i, " ".join(str(v) for v in trace[i].op) if i >= 0 else "first frame", ht.describe(trace, i + 1))

    vet = ht.build(gh, start, lib_path)
    lib = vet._L
    state, checked, due, i = start, 0, False, -1
    try:
        compare_with_fresh(gh, vet, state, where, lib_path)
        for i, st in enumerate(trace):
            before = vet.stats()["overflow_frames"]
            try:
                ht.apply(gh, vet, st.op, state)
            except gh.GsplatError as e:
                raise AssertionError("%s: the operation failed: %s" % (where(), e))
            state = ht.fold(state, st.op)
            due = due or (oracle is not None and i % oracle_every == oracle_every - 1)
            if not st.check:
                continue
            try:
                a = compare_with_fresh(gh, vet, state, where, lib_path)
            except gh.GsplatError as e:
                raise AssertionError("%s: rendering or reading the frame failed: %s" % (where(), e))
            checked += 1
            if st.op[0] == "overflow_sync":     # the step's own frame is the one that did not fit, repaired by gsr_sync
                fitted = int(a["bin starts"][-1]) <= max(st.op[1], 1024)
                assert (vet.stats()["overflow_frames"] == before) == fitted, where()
            if due and ht.scene_n(state.scene):
                meet_oracle(gh, oracle, vet, state, a, where)
                due = False
    finally:
        vet.dispose()
    return checked, lib


def test_tour_on_a_default_context(gh):
    t = ht.tour()
    checked, _ = run_trace(gh, t, ht.State(kind="default"), "tour, default context")
    assert checked == sum(st.check for st in t)


def test_tour_on_a_throughput_context(gh):
    """(with stage events: the tour's first operation makes every other frame carry them, the others are graph replays)"""
    t = ht.tour()
    checked, _ = run_trace(gh, t, ht.State(kind="throughput", timing=True), "tour, throughput context")
    assert checked == sum(st.check for st in t)


def test_tour_on_a_band_context(gh):
    """one rank of a multi-GPU frame: created with a band, and the band set again behind every resize"""
    t = ht.tour(band_context=True)
    checked, _ = run_trace(gh, t, ht.State(kind="throughput", band=(192, 448)), "tour, band context")
    assert checked == sum(st.check for st in t)


@pytest.mark.parametrize("kind", ["default", "throughput"])
@pytest.mark.parametrize("seed", [101, 202, 303])
def test_random_walks(gh, oracle, seed, kind):
    start = ht.State(kind=kind, timing=bool(seed & 1))
    t = ht.walk(seed, 60, start)
    run_trace(gh, t, start, "walk(%d, 60), %s context" % (seed, kind), oracle=oracle)


def test_frames_in_flight_have_no_memory(gh):
    """bench.py's way: three throughput contexts, a frame in flight each, issued round-robin without waiting -- here with scene and
    size changes in between.  The last frame of each is a fresh context's."""
    plans = [
        {1: ("scene", ("synth", 70000, 4, "raw")), 3: ("resize", 801, 601), 5: ("scene", ("synth", 2049, 5, "rows")), 6: ("band", 256, 512)},
        {0: ("resize", 333, 219), 2: ("scene", ("synth", 20000, 9, "rows")), 3: ("rotate", ht.QUAT), 4: ("resize", 1279, 717), 6: ("sort_only", 1, 3)},
        {2: ("scene", ("synth", 0, 1, "raw")), 4: ("scene", ("config", "C1", "raw")), 5: ("sh", (11, 0.0, 0.25, 0.5)), 7: ("timing_interval", 2)},
    ]
    states = [ht.State(kind="throughput", timing=True, scene=("synth", 20000, 9 + j, "raw")) for j in range(3)]
    vets = [ht.build(gh, s) for s in states]
    try:
        for k in range(9):
            for j, vet in enumerate(vets):
                op = plans[j].get(k)
                if op:
                    ht.apply(gh, vet, op, states[j])
                    states[j] = ht.fold(states[j], op)
                states[j] = ht.fold(states[j], ("camera", (7 * k + 11 * j) % 120))
                ht._frame(gh, vet, states[j])            # no wait: the next context's frame is issued behind it
        for vet in vets:
            vet.sync()
        for j, vet in enumerate(vets):
            compare_with_fresh(gh, vet, states[j], lambda: "frames in flight, context %d, plan %r" % (j, plans[j]))
    finally:
        for vet in vets:
            vet.dispose()


def test_a_refused_call_changes_nothing(gh):
    start = ht.State(kind="default", scene=("synth", 20000, 9, "rows"))
    prelude = [("rotate", ht.QUAT), ("sh", (11, 0.0, 0.25, 0.5)), ("band", 192, 448), ("fade", True, 0.5), ("hit_alpha", 0.25),
               ("ring_open", "nv12", False, "u16", 2)]
    t = [ht.Step(op, False) for op in prelude[:-1]] + [ht.Step(prelude[-1], True)]
    for which in ht.REFUSALS:
        t += [ht.Step(("refused", which), True), ht.Step(("camera", 40 + len(t)), True)]
    run_trace(gh, t, start, "refused calls")
    # and the codes: a scene whose positions differ from its data is GSR_ERR_SCENE, the others GSR_ERR_ARG
    r = ht.build(gh, start)
    try:
        codes = {which: ht.apply(gh, r, ("refused", which), start)["code"] for which in ht.REFUSALS}
        assert r.scene_count() == 20000
    finally:
        r.dispose()
    assert codes == {"band_off_boundary": ht.GSR_ERR_ARG, "size_zero": ht.GSR_ERR_ARG, "positions_differ": ht.GSR_ERR_SCENE,
                     "timing_interval_zero": ht.GSR_ERR_ARG}


def _bounds_counts(L, units):
    bad = {}
    for unit in units:
        buf = (ctypes.c_uint32 * 8)()
        assert getattr(L, "gsr_debug_bounds_" + unit)(buf) == 0
        bad.update({(unit, site): v for site, v in enumerate(buf) if v})
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# The editing layer: selection, hidden set, edits of the selection, growth and erasure, overlay, contribution (history_trace's
# State.edits / overlay / ring_overlay / contrib).  The fresh context gets the recipe evaluated on the CPU: it never ran an edit
# kernel and never grew, and its capacity equals its count.
# ---------------------------------------------------------------------------------------------------------------------------
EDIT_BOUNDS_UNITS = ("blend", "bin", "sort", "depth", "deliver", "scene", "scene_sh", "select", "edit", "append", "contrib", "overlay") + ANALYSIS_UNITS
ALL_KINDS = ht.KINDS + ht.EDIT_KINDS


def test_editing_tour_on_a_default_context(gh):
    t = ht.editing_tour()
    checked, _ = run_trace(gh, t, ht.State(kind="default"), "editing tour, default context")
    assert checked == sum(st.check for st in t)


def test_editing_tour_on_a_throughput_context(gh):
    """(with stage events on every other frame: the others are graph replays)"""
    t = [ht.Step(("timing_interval", 2), True)] + ht.editing_tour()
    checked, _ = run_trace(gh, t, ht.State(kind="throughput", timing=True), "editing tour, throughput context")
    assert checked == sum(st.check for st in t)


def test_editing_tour_on_a_band_context(gh):
    t = ht.editing_tour(band_context=True)
    checked, _ = run_trace(gh, t, ht.State(kind="throughput", band=(192, 448)), "editing tour, band context")
    assert checked == sum(st.check for st in t)


def test_editing_tour_on_the_bounds_checked_build(gh):
    """a stale row behind n, a selection word of the old capacity, a rectangle of the old numbering: indices into the wrong data,
    counted by the build that checks every index derived from device data"""
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    t = ht.editing_tour(band_context=True)
    _, L = run_trace(gh, t, ht.State(kind="default", band=(192, 448)), "editing tour, bounds-checked build", lib_path=BOUNDS_LIB)
    bad = _bounds_counts(L, EDIT_BOUNDS_UNITS)
    assert not bad, bad


@pytest.mark.parametrize("kind", ["default", "throughput"])
@pytest.mark.parametrize("seed", [11, 22, 33])
def test_editing_walks(gh, oracle, seed, kind):
    """random walks over the old and the new kinds together (tests/test_history_trace.py: each holds every kind, no step is vacuous)"""
    start = ht.State(kind=kind, timing=bool(seed & 1))
    t = ht.walk(seed, 150, start, kinds=ALL_KINDS, oracle=oracle)
    run_trace(gh, t, start, "walk(%d, 150, kinds=KINDS + EDIT_KINDS), %s context" % (seed, kind), oracle=oracle)


SHARED_FIELDS = ("scene", "transforms", "sh", "edits", "contrib")      # what the members of a shared scene have together


def test_two_veterans_share_one_scene(gh, oracle):
    """A default context and a throughput context of another size render one device scene.  Operations arrive through either member
    in turn while a frame of the other is in flight; after each, every member's frame is the frame of a fresh context of its kind
    built from the same State, a pick through the member that did not act is refused exactly when the operation was an edit, and
    selection and hidden set read the same through both."""
    box = tuple(v * 0.5 for v in ht.BOX)
    ops = [("select_box", box, "replace"), ("hide", "add"), ("set_selection", (3, 0.3), "replace"), ("edit", "translate", (0.25, -0.5, 0.0), None),
           ("duplicate", "grow"), ("edit", "rotate", ht.QUAT, ht.PIVOT), ("set_hidden", (5, 0.3), "add"), ("select_region", (80, 50, 250, 170), None, "replace"),
           ("edit", "rgba", (0x80ff2010, 0xffffffff), None), ("select_attr", "opacity", 0.0, 128.0, None, "add"), ("duplicate", None), ("erase", False),
           ("select_region", ht.RECT, None, "replace"), ("reserve", 9000), ("duplicate", "fit"), ("rotate", ht.QUAT), ("set_hidden", None, "replace"),
           ("invert_selection",), ("append_arrays", 33, 4), ("limit_box", ht.BOX), ("set_selection", (6, 0.5), "replace"), ("erase", True),
           # the analysis layer: a merge through member 0, a picker and a report through member 1, frames of both in between
           ("set_selection", (7, 0.3), "replace"), ("duplicate", None), ("merge_cells", ht.COINCIDENT, ()),
           ("select_neighbours", 0.4, 1, None, 8, (), "replace"), ("set_hidden", (8, 0.3), "replace"), ("report", "clusters", 0.5, 1, ("visible",)),
           ("merge_cells", 0.3, ("visible",)), ("select_knn", 0.6, 2, "kth", 0.0, 0.45, ("selected", "visible"), "add")]
    scene = ("synth", 2049, 5, "rows")
    states = [ht.State(kind="default", scene=scene), ht.State(kind="throughput", timing=True, W=333, H=219, scene=scene)]
    vets = [ht.build(gh, s) for s in states]
    k = -1

    def where(j):
        return lambda: "shared scene, operation %d (%s) through member %d, seen by member %d" % (k, " ".join(str(v) for v in ops[k]) if k >= 0 else "none", k % 2, j)

    try:
        vets[1].share_scene(vets[0])
        for j in (0, 1):
            compare_with_fresh(gh, vets[j], states[j], where(j))
        for k, op in enumerate(ops):
            actor, other = k % 2, 1 - k % 2
            assert ht.vacuous(states[actor], op, oracle) is None, (k, op)
            states[other] = ht.fold(states[other], ("camera", (7 * k + 3) % 120))
            ht._frame(gh, vets[other], states[other])                       # in flight: the operation does not wait for it
            ht.apply(gh, vets[actor], op, states[actor])
            after = ht.fold(states[actor], op)
            states = [replace(s, **{f: getattr(after, f) for f in SHARED_FIELDS}) for s in states]
            edit = op[0] not in ht.SELECT_KINDS + ht.ANALYSIS_KEEPS_FRAME and op[0] != "reserve"
            got = ht.apply(gh, vets[other], ("readback", "pick"), states[other], edited=edit)
            assert ("refused" in got) == edit, (k, op, got)
            seen = [compare_with_fresh(gh, vets[j], states[j], where(j)) for j in (0, 1)]
            for name in ("scene_count()", "selection words", "selection count", "hidden words", "hidden count", "selection_bounds()"):
                assert _same(seen[0][name], seen[1][name]), "%s: the members disagree on %s" % (where(1)(), name)
            m = ht.materialise(states[0], oracle)
            assert _same(seen[0]["selection words"], m.selection_words) and _same(seen[0]["hidden words"], m.hidden_words), where(0)()
        assert vets[0].scene_sharing()[0] == 2
    finally:
        for vet in vets:
            vet.dispose()


def test_frames_in_flight_with_edits_have_no_memory(gh):
    """test_frames_in_flight_have_no_memory with hides, duplicates, erases and a merge between the frames"""
    pick = [("set_selection", (3, 0.3), "replace"), ("set_selection", (4, 0.1), "replace"), ("select_box", tuple(v * 0.5 for v in ht.BOX), "replace")]
    plans = [
        {1: [pick[0], ("hide", "add")], 3: [("duplicate", None)], 5: [("erase", False)], 6: [("set_hidden", None, "replace")], 7: [pick[1], ("duplicate", None)]},
        {0: [("resize", 333, 219)], 2: [pick[2], ("duplicate", None)], 3: [("hide", "add")], 4: [("resize", 801, 601)], 5: [pick[1], ("erase", False)],
         7: [("band", 256, 512)]},
        {1: [pick[1], ("duplicate", None)], 2: [("duplicate", None)], 4: [("set_hidden", (5, 0.5), "replace")], 5: [pick[0], ("erase", True)], 6: [("set_hidden", (6, 0.5), "add")],
         7: [pick[1], ("duplicate", None), ("merge_cells", ht.COINCIDENT, ())],     # a merge between frames in flight: the copies merge with their originals
         8: [("timing_interval", 2)]},
    ]
    states = [ht.State(kind="throughput", timing=True, scene=("synth", 20000, 9 + j, "rows")) for j in range(3)]
    vets = [ht.build(gh, s) for s in states]
    try:
        for k in range(9):
            for j, vet in enumerate(vets):
                for op in plans[j].get(k, ()):
                    ht.apply(gh, vet, op, states[j])
                    states[j] = ht.fold(states[j], op)
                states[j] = ht.fold(states[j], ("camera", (7 * k + 11 * j) % 120))
                ht._frame(gh, vet, states[j])            # no wait: the next context's frame is issued behind it
        for vet in vets:
            vet.sync()
        for j, vet in enumerate(vets):
            assert states[j].edits and vet.scene_count() not in (0, 20000)
            compare_with_fresh(gh, vet, states[j], lambda: "frames in flight with edits, context %d, plan %r" % (j, plans[j]))
    finally:
        for vet in vets:
            vet.dispose()


def test_the_editing_refusals_change_nothing_and_say_why(gh):
    """the codes of EDIT_REFUSALS, each from the State it needs (the editing tour walks them with a frame behind each)"""
    raw = ht.State(kind="default", scene=("synth", 2049, 5, "raw"))
    rows = ht.State(kind="default", scene=("synth", 2049, 5, "rows"))
    some = ("set_selection", (3, 0.5), "replace")
    cases = {"edit_raw": (raw, [some], ht.GSR_ERR_ARG), "erase_raw": (raw, [some], ht.GSR_ERR_ARG),
             "grow_with_sh": (rows, [("sh", (11, 0.0, 0.25, 0.5))], ht.GSR_ERR_ARG),
             "rotate_selected_sh_follow": (rows, [some, ("sh", (11, 0.0, 0.25, 0.5))], ht.GSR_ERR_ARG),
             "append_positions_differ": (rows, [], ht.GSR_ERR_SCENE)}
    assert set(cases) == set(ht.EDIT_REFUSALS)
    for which, (start, prelude, code) in cases.items():
        r, s = ht.build(gh, start), start
        try:
            for op in prelude:
                ht.apply(gh, r, op, s)
                s = ht.fold(s, op)
            cap = r.scene_capacity()
            assert ht.apply(gh, r, ("refused", which), s)["code"] == code, which
            assert (r.scene_count(), r.scene_capacity()) == (2049, cap) and r.sh_frame()[1] is False
        finally:
            r.dispose()


# ---------------------------------------------------------------------------------------------------------------------------
# The analysis layer: neighbour counts, clusters, k nearest neighbours and merge cells (history_trace's ANALYSIS_KINDS).  All four
# share one neighbour scratch and one hashed index per context; a merge replaces the scene from the inside.  The fresh context gets
# the recipe evaluated on the CPU by the feature suites' references: it never ran an analysis kernel before its own observables.
# ---------------------------------------------------------------------------------------------------------------------------
EVERY_KIND = ht.KINDS + ht.EDIT_KINDS + ht.ANALYSIS_KINDS
ANALYSIS_WALK_STEPS = 180


def test_analysis_tour_on_a_default_context(gh):
    t = ht.analysis_tour()
    checked, _ = run_trace(gh, t, ht.State(kind="default"), "analysis tour, default context")
    assert checked == sum(st.check for st in t)


def test_analysis_tour_on_a_throughput_context(gh):
    """(with stage events on every other frame: the others are graph replays)"""
    t = [ht.Step(("timing_interval", 2), True)] + ht.analysis_tour()
    checked, _ = run_trace(gh, t, ht.State(kind="throughput", timing=True), "analysis tour, throughput context")
    assert checked == sum(st.check for st in t)


def test_analysis_tour_on_a_band_context(gh):
    t = ht.analysis_tour(band_context=True)
    checked, _ = run_trace(gh, t, ht.State(kind="throughput", band=(192, 448)), "analysis tour, band context")
    assert checked == sum(st.check for st in t)


def test_analysis_tour_on_the_bounds_checked_build(gh):
    """a bucket of the table the call before sized, an entry of the old numbering, a mask word of the larger scene's scratch: indices
    into the wrong data, counted by the build that checks every index derived from device data"""
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    t = ht.analysis_tour(band_context=True)
    _, L = run_trace(gh, t, ht.State(kind="default", band=(192, 448)), "analysis tour, bounds-checked build", lib_path=BOUNDS_LIB)
    bad = _bounds_counts(L, EDIT_BOUNDS_UNITS)
    assert not bad, bad


@pytest.mark.parametrize("kind", ["default", "throughput"])
@pytest.mark.parametrize("seed", [7, 14, 21])
def test_analysis_walks(gh, oracle, seed, kind):
    """random walks over all three kind sets together (tests/test_history_trace.py: each holds every kind, no step is vacuous)"""
    start = ht.State(kind=kind, timing=bool(seed & 1))
    t = ht.walk(seed, ANALYSIS_WALK_STEPS, start, kinds=EVERY_KIND, oracle=oracle)
    run_trace(gh, t, start, "walk(%d, %d, kinds=KINDS + EDIT_KINDS + ANALYSIS_KINDS), %s context" % (seed, ANALYSIS_WALK_STEPS, kind), oracle=oracle)


def test_the_analysis_refusals_change_nothing_and_say_why(gh):
    """the codes and texts of ANALYSIS_REFUSALS, each from the State it needs (the analysis tour walks them with a frame behind each):
    scene, selection and count stay, and a picker refused for its budget leaves the selection untouched"""
    raw = ht.State(kind="default", scene=("synth", 2049, 5, "raw"))
    rows = ht.State(kind="default", scene=("synth", 2049, 5, "rows"))
    some = ("set_selection", (3, 0.5), "replace")
    for which in ht.ANALYSIS_REFUSALS:
        start = raw if which == "merge_raw" else rows
        prelude = [some] + ([("sh", (11, 0.0, 0.25, 0.5))] if which == "merge_with_sh" else [])
        r, s = ht.build(gh, start), start
        try:
            for op in prelude:
                ht.apply(gh, r, op, s)
                s = ht.fold(s, op)
            scene, words, cap = r.read_scene(with_rows=which != "merge_raw"), r.selection_words().copy(), r.scene_capacity()
            got = ht.apply(gh, r, ("refused", which), s)
            assert got["code"] == ht.GSR_ERR_ARG and ht.ANALYSIS_REFUSAL_TEXTS[which] in got["message"], (which, got)
            assert (r.scene_count(), r.scene_capacity()) == (2049, cap) and _same(r.selection_words(), words), which
            assert _same(r.read_scene(with_rows=which != "merge_raw"), scene), which
        finally:
            r.dispose()


def test_tour_on_the_bounds_checked_build(gh):
    """The tour once more on the build that checks every index derived from device data (tests/test_gpu_bounds.py): a stale rectangle
    or a stale survivor slot is an index into the wrong frame's data, and this build counts that instead of trapping."""
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    t = ht.tour(band_context=True)
    _, L = run_trace(gh, t, ht.State(kind="default", band=(192, 448)), "tour, bounds-checked build", lib_path=BOUNDS_LIB)
    bad = {}
    for unit in BOUNDS_UNITS:
        buf = (ctypes.c_uint32 * 8)()
        assert getattr(L, "gsr_debug_bounds_" + unit)(buf) == 0
        bad.update({(unit, site): v for site, v in enumerate(buf) if v})
    assert not bad, bad

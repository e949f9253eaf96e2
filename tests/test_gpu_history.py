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

import numpy as np
import pytest

import history_trace as ht
import work_items_reference

pytestmark = pytest.mark.gpu

TOL_EXACT = 2e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
BOUNDS_UNITS = ("blend", "bin", "sort", "depth", "deliver")

# The only things a veteran and a fresh context may disagree on: what counts frames, deliveries or time.
#   gsr_timings: everything but these four describes the context's life, not the frame
FRAME_STATS = ("visible", "bin_entries", "tile_entries", "n")
#   a delivered frame's trailer is (overflow word, dims, serial low, serial high): the serial counts deliveries
TRAILER_FRAME_WORDS = 2
#   and the serial gsr_deliver_frame_async / gsr_acquire_frame return (never compared)


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
    if state.ring is not None:
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
    return o


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
    """depthIndex exact, the band's columns of the image within TOL_EXACT: veteran and fresh are not wrong together"""
    data, pos, _, _ = vet.read_scene(with_rows=False)
    n = pos.size // 3
    cam = ht.camera_of(gh, state)
    v, p, vp = cam.f32()
    sh = bidx = None
    if state.sh is not None:
        tex, b = ht.sh_arrays(gh, state.sh, n)
        if n - (int(b[0]) + 1) > 0:
            sh, bidx = tex, b
    oimg, odi, _, _ = O.render_scene(data, pos, v, p, vp, cam.fx, cam.fy, state.W, state.H, mode=1, sh=sh, band=bidx,
                                     fade=state.fade[1] if state.fade[0] else None)
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

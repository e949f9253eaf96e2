"""Depth planes and picking on the GPU (k_depth.hip, gsr_depth.cpp) against tests/depth_reference.py -- the specification
in numpy, fed by the oracle's projection and sort, never by device read-backs -- and against themselves where the
specification says two results are the same bits: every kind of context and binning form (same lists, same recurrence),
the skip of entries that cannot reach a tile, pick against the planes, a band against the full frame.  The frame itself
must not notice the pass."""
import ctypes
import os

import numpy as np
import pytest

import blend_reference as BR
import depth_reference as DR
from test_oracle_render import make_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
KNOBS = ("GSR_BIN_TWO_LEVEL", "GSR_LONG_ITEMS", "GSR_DEPTH_SKIP")
NONE = DR.NONE
GSR_ERR_ARG = -1
POSES = {"C1": (3, 40), "C2": (13, 40), "C3": (21, 84)}


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _cam(gh, name, k):
    cfg = gh.synth.CONFIGS[name]
    return gh.orbit_camera(k, width=cfg["width"], height=cfg["height"], fx=cfg["fx"])


def _window(name, gh):
    """the part of the image the numpy reference is evaluated on: all of C1, a centre window of the large scenes"""
    cfg = gh.synth.CONFIGS[name]
    if name == "C1":
        return (0, 0, cfg["width"], cfg["height"])
    return (cfg["width"] // 2 - 128, cfg["height"] // 2 - 128, 256, 256)


class Ref:
    """The oracle's projection and order of one (scene, pose), and the reference planes of its window."""

    def __init__(self, oracle, gh, name, data, pos, k, hit_alpha=0.5, fade=None):
        cfg = gh.synth.CONFIGS[name]
        self.evaluate(oracle, _cam(gh, name, k), data, pos, cfg["width"], cfg["height"], _window(name, gh), hit_alpha, fade)

    @classmethod
    def of_scene(cls, oracle, cam, data, pos, W, H, hit_alpha):
        """the reference of a scene that is no named configuration, over the whole W x H image"""
        ref = cls.__new__(cls)
        ref.cam, ref.data, ref.pos = cam, data, pos
        ref.evaluate(oracle, cam, data, pos, W, H, (0, 0, W, H), hit_alpha)
        return ref

    def evaluate(self, oracle, cam, data, pos, W, H, window, hit_alpha, fade=None):
        self.W, self.H = W, H
        v, p, vp = cam.f32()
        kw = {} if fade is None else {"fade": fade}
        self.rec, self.bbox, raw = oracle.project(data, v, p, cam.fx, cam.fy, self.W, self.H, **kw)
        self.z = np.ascontiguousarray(raw[:, 10])
        self.order = oracle.sort(vp, pos)[0]
        self.window = window
        self.planes = DR.depth_planes_reference(self.rec, self.bbox, self.z, self.order, self.W, self.H, self.window, hit_alpha)
        vis = (self.bbox[:, 0] <= self.bbox[:, 2]) & (self.bbox[:, 1] <= self.bbox[:, 3])
        self.zmin, self.zmax = float(self.z[vis].min()), float(self.z[vis].max())

    def check(self, got, what):
        x0, y0, w, h = self.window
        mean, hit, index = (a[y0:y0 + h, x0:x0 + w] for a in got)
        pl = self.planes
        ok = ~pl["mask"]
        assert pl["mask"].mean() < 0.01, (what, pl["mask"].mean())
        assert (pl["index"] != NONE).any(), what
        bad = ok & (index != pl["index"])
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        some = ok & (index != NONE)
        assert np.array_equal(hit[some], self.z[index[some]]), (what, "hit is not z of index, bit for bit")
        assert np.all(np.isinf(hit[ok & (index == NONE)])), what
        err = np.abs(mean.astype(np.float64) - pl["mean"])[ok].max()
        assert err <= 2e-4 * max(1.0, self.zmax), (what, err)


@pytest.fixture(scope="module")
def refs(oracle, scenes, gh):
    cache = {}

    def get(name, k, **kw):
        key = (name, k, tuple(sorted(kw.items())))
        if key not in cache:
            _, data, pos = scenes(name)
            cache[key] = Ref(oracle, gh, name, data, pos, k, **kw)
        return cache[key]

    yield get
    cache.clear()


def _context(gh, monkeypatch, name, scenes, env=None, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    cfg = gh.synth.CONFIGS[name]
    r = gh.HIPRenderer(cfg["width"], cfg["height"], **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)
    _, data, pos = scenes(name)
    r.set_raw_scene(data, pos)
    return r


def _frame(gh, r, name, k):
    r.set_camera(_cam(gh, name, k))
    r.render_async()
    r.sync()


def _bounds_zero(r, what):
    buf = (ctypes.c_uint32 * 8)()
    assert r._L.gsr_debug_bounds_depth(buf) == 0
    assert not any(buf), (what, list(buf))


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("throughput", [False, True], ids=["default", "throughput"])
@pytest.mark.parametrize("name", ["C1", "C2"])
def test_planes_meet_the_reference(gh, monkeypatch, scenes, refs, name, throughput):
    r = _context(gh, monkeypatch, name, scenes, throughput=throughput)
    for k in POSES[name]:              # the first frame sorts in the LSD order, the second in the bucket order
        _frame(gh, r, name, k)
        refs(name, k).check(r.read_depth(), (name, throughput, k))
    r.dispose()


# 2 -------------------------------------------------------------------------------------------------------------------
def test_every_kind_of_context_gives_the_same_bits(gh, monkeypatch, scenes):
    name, k = "C2", POSES["C2"][0]
    want = None
    forms = [({}, False), ({}, True), ({"GSR_BIN_TWO_LEVEL": "1"}, False), ({"GSR_LONG_ITEMS": "0"}, True), ({"GSR_LONG_ITEMS": "1"}, False)]
    for env, throughput in forms:
        r = _context(gh, monkeypatch, name, scenes, env=env, throughput=throughput)
        _frame(gh, r, name, k)
        got = r.read_depth()
        r.dispose()
        if want is None:
            want = got
            assert (want[2] != NONE).any()
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (env, throughput)


# 3 -------------------------------------------------------------------------------------------------------------------
def test_the_frame_does_not_notice_the_pass(gh, monkeypatch, scenes):
    name, k = "C2", POSES["C2"][1]
    plain = _context(gh, monkeypatch, name, scenes)
    r = _context(gh, monkeypatch, name, scenes)
    assert r._L.gsr_depth_device_ptr(r._ctx, 0) is None          # nothing allocated before the first use
    for c in (plain, r):
        _frame(gh, c, name, POSES["C2"][0])
        _frame(gh, c, name, k)
    before = (r.readPixelsFloat(), r.lastDepthIndex(), r.work_items(), r.stats())
    r.depth_async()
    r.read_depth()
    r.pick([(960, 540)])
    assert r._L.gsr_depth_device_ptr(r._ctx, 2) is not None and r._L.gsr_depth_device_ptr(r._ctx, 3) is None
    after = (r.readPixelsFloat(), r.lastDepthIndex(), r.work_items(), r.stats())
    other = (plain.readPixelsFloat(), plain.lastDepthIndex(), plain.work_items(), plain.stats())
    for got in (after, other):
        assert np.array_equal(got[0].view(np.uint32), before[0].view(np.uint32)) and np.array_equal(got[1], before[1])
        assert got[2] == before[2] and got[3] == before[3]
    plain.dispose(); r.dispose()


# 4 -------------------------------------------------------------------------------------------------------------------
def test_c3_three_throughput_contexts_in_flight(gh, monkeypatch, scenes, refs):
    name = "C3"
    ctxs = [_context(gh, monkeypatch, name, scenes, throughput=True) for _ in range(3)]
    poses = [POSES[name][0], POSES[name][1], POSES[name][1]]
    for rnd in range(3):               # the depth pass behind every frame, three frames in flight
        for r, k in zip(ctxs, poses):
            r.set_camera(_cam(gh, name, k if rnd == 2 else k + 1 + rnd))
            r.render_async()
            r.depth_async()
    for r in ctxs:
        r.sync()
    got = [r.read_depth() for r in ctxs]
    alpha = [r.readPixelsFloat()[..., 3] for r in ctxs]
    for r in ctxs:
        r.dispose()
    for a, b in zip(got[1], got[2]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for (mean, hit, index), al, k in zip(got[:2], alpha[:2], poses[:2]):
        ref = refs(name, k)
        ref.check((mean, hit, index), (name, k))
        # the whole image: hit is z of index, the pixel lies in that splat's box, expected depth lies among the visible splats'
        some = index != NONE
        assert some.mean() > 0.05
        assert np.array_equal(hit[some], ref.z[index[some]]) and np.all(np.isinf(hit[~some]))
        ys, xs = np.nonzero(some)
        bb = ref.bbox[index[some]]
        assert np.all((bb[:, 0] <= xs) & (xs <= bb[:, 2]) & (bb[:, 1] <= ys) & (ys <= bb[:, 3]))
        seen = al > 1e-3
        e = mean[seen].astype(np.float64) / al[seen]
        assert e.min() >= ref.zmin * (1 - 1e-3) and e.max() <= ref.zmax * (1 + 1e-3), (e.min(), e.max(), ref.zmin, ref.zmax)


# 5 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,band", [({}, (864, 1056)), ({"GSR_BIN_TWO_LEVEL": "1"}, (512, 1230))], ids=["one level", "two level"])
def test_band_context(gh, monkeypatch, scenes, env, band):
    name, k = "C2", POSES["C2"][0]
    full = _context(gh, monkeypatch, name, scenes)
    _frame(gh, full, name, k)
    want = full.read_depth()
    full.dispose()
    r = _context(gh, monkeypatch, name, scenes, env=env, band=band)
    _frame(gh, r, name, k)
    got = r.read_depth()
    x0, x1 = band[0] // 32 * 32, min(-(-band[1] // 32) * 32, r.width)
    inside = np.zeros(got[0].shape, bool)
    inside[:, x0:x1] = True
    for a, b, rest in zip(got, want, (np.float32(0).view(np.uint32), np.float32(np.inf).view(np.uint32), np.uint32(NONE))):
        assert np.array_equal(a.view(np.uint32)[inside], b.view(np.uint32)[inside])
        assert np.all(a.view(np.uint32)[~inside] == rest)
    assert (got[2][inside] != NONE).any()
    one = r.pick([(x0, 500), (x1 - 1, 500)])
    assert one["index"][0] == got[2][500, x0] and one["index"][1] == got[2][500, x1 - 1]
    for x in (x0 - 1, x1):
        with pytest.raises(gh.GsplatError, match="band") as ei:
            r.pick([(x, 500)])
        assert ei.value.code == GSR_ERR_ARG
    r.dispose()


# 6 -------------------------------------------------------------------------------------------------------------------
def test_depth_fade_and_sh_scene(gh, monkeypatch, scenes, refs):
    name, k = "C1", POSES["C1"][0]
    r = _context(gh, monkeypatch, name, scenes)
    r.set_depth_fade(1, 0.8)                # (at this pose 0.8 scales 96 % of the visible splats' axes; 0.5 leaves three splats)
    _frame(gh, r, name, k)
    refs(name, k, fade=0.8).check(r.read_depth(), "depth fade")
    r.set_depth_fade(0, 0.0)
    n = gh.synth.CONFIGS[name]["n"]
    sh = [np.full(8 * n, 0x34003400, dtype=np.uint32) for _ in range(3)]   # (every half-float coefficient 0.25)
    bands = [-1, n // 4, n // 2]
    r.set_sh(sh, bands)
    _frame(gh, r, name, k)
    refs(name, k).check(r.read_depth(), "SH scene")                        # colours do not enter the planes
    r.dispose()


# 7 -------------------------------------------------------------------------------------------------------------------
def test_hit_alpha(gh, monkeypatch, scenes, refs):
    name, k = "C1", POSES["C1"][0]
    r = _context(gh, monkeypatch, name, scenes)
    _frame(gh, r, name, k)
    half = r.read_depth()
    counts = {}
    for a in (0.1, 0.99):
        r.set_hit_alpha(a)
        got = r.read_depth()                                               # (the planes are redone for the new threshold)
        refs(name, k, hit_alpha=a).check(got, ("hit_alpha", a))
        assert np.array_equal(got[0].view(np.uint32), half[0].view(np.uint32))   # mean does not depend on it
        counts[a] = int((got[2] != NONE).sum())
    assert counts[0.1] > int((half[2] != NONE).sum()) > counts[0.99] > 0
    r.set_hit_alpha(1.0)
    for a in (0.0, 1.5, float("nan")):
        with pytest.raises(gh.GsplatError, match="hit_alpha") as ei:
            r.set_hit_alpha(a)
        assert ei.value.code == GSR_ERR_ARG
    r.dispose()


# 8 -------------------------------------------------------------------------------------------------------------------
def _pick_at(r, planes, pts):
    pts = np.asarray(pts)
    res = r.pick(pts)
    mean, hit, index = planes
    ys, xs = pts[:, 1], pts[:, 0]
    assert np.array_equal(res["index"], index[ys, xs])
    assert np.array_equal(res["depth"].view(np.uint32), hit[ys, xs].view(np.uint32))
    assert np.array_equal(res["mean"].view(np.uint32), mean[ys, xs].view(np.uint32))
    assert np.abs(res["alpha"].astype(np.float64) - r.readPixelsFloat()[ys, xs, 3]).max() <= 2e-6
    return res


def _pick_equals_planes(gh, r, planes, seed=8):
    W, H = r.width, r.height
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.integers(0, W, 512), rng.integers(0, H, 512)], axis=1)
    pts = np.concatenate([pts, [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]])
    res = _pick_at(r, planes, pts)
    assert (res["index"] != NONE).any()
    return res


def test_pick(gh, monkeypatch, scenes):
    name = "C1"
    cfg = gh.synth.CONFIGS[name]
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    with pytest.raises(gh.GsplatError, match="no frame") as ei:
        r.pick([(1, 1)])
    assert ei.value.code == GSR_ERR_ARG
    with pytest.raises(gh.GsplatError, match="no frame"):
        r.depth_async()
    with pytest.raises(gh.GsplatError, match="no frame"):
        r.read_depth()
    _, data, pos = scenes(name)
    r.set_raw_scene(data, pos)
    _frame(gh, r, name, POSES[name][0])
    planes = r.read_depth()
    _pick_equals_planes(gh, r, planes)
    empty = np.argwhere(r.readPixelsFloat()[..., 3] == 0)
    assert len(empty)
    y, x = empty[0]
    one = r.pick([(x, y)])[0]
    assert one["index"] == NONE and np.isinf(one["depth"]) and one["mean"] == 0 and one["alpha"] == 0
    W, H = r.width, r.height
    for bad in ([(-1, 0)], [(W, 0)], [(0, H)], [(0, -1)], np.zeros((0, 2)), np.zeros((4097, 2))):
        with pytest.raises(gh.GsplatError) as ei:
            r.pick(bad)
        assert ei.value.code == GSR_ERR_ARG
    assert len(r.pick(np.zeros((4096, 2)))) == 4096
    r.sort()                                                                # a sort-only frame has no lists
    with pytest.raises(gh.GsplatError, match="sort-only"):
        r.pick([(1, 1)])
    _frame(gh, r, name, POSES[name][0])
    r.set_raw_scene(data, pos)                                              # the scene changed since the frame
    with pytest.raises(gh.GsplatError, match="no frame"):
        r.read_depth()
    _frame(gh, r, name, POSES[name][0])
    r.setSize(320, 240)
    with pytest.raises(gh.GsplatError, match="no frame"):
        r.pick([(1, 1)])
    r.dispose()


# 9 -------------------------------------------------------------------------------------------------------------------
def _overflow_is_repaired(gh, scenes, name, lib_path=None):
    cfg = gh.synth.CONFIGS[name]
    _, data, pos = scenes(name)
    cam = _cam(gh, name, POSES[name][1])
    ref = gh.HIPRenderer(cfg["width"], cfg["height"], lib_path=lib_path)
    ref.set_raw_scene(data, pos)
    ref.set_camera(cam)
    ref.render_async(); ref.sync()
    want = ref.read_depth()
    assert ref.stats()["overflow_frames"] == 0 and ref.stats()["bin_entries"] > 4096
    ref.dispose()
    r = gh.HIPRenderer(cfg["width"], cfg["height"], lib_path=lib_path)
    r.set_raw_scene(data, pos)
    r.set_camera(_cam(gh, name, POSES[name][0]))
    r.render_async(); r.sync()
    r.read_depth()                             # planes of an earlier frame are on the device
    r.set_list_capacity(1024)                  # far too small for the next frame
    r.set_camera(cam)
    r.render_async()
    r.depth_async()                            # behind a frame that does not fit: walks nothing, writes nothing
    got = r.read_depth()                       # the frame is rendered again with regrown lists, the pass redone
    assert r.stats()["overflow_frames"] == 1 and r.stats()["dropped_frames"] == 0
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    r.set_list_capacity(1024)
    r.render_async()
    res = r.pick([(cfg["width"] // 2, cfg["height"] // 2)])   # the same repair in front of a pick
    assert res["index"][0] == want[2][cfg["height"] // 2, cfg["width"] // 2]
    return r


def test_overflow_is_repaired_before_anything_is_returned(gh, scenes):
    _overflow_is_repaired(gh, scenes, "C1").dispose()


# 10 ------------------------------------------------------------------------------------------------------------------
def test_bounds_twin(gh, monkeypatch, scenes, refs):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    name = "C1"
    for throughput in (False, True):
        r = _context(gh, monkeypatch, name, scenes, throughput=throughput, lib_path=BOUNDS_LIB)
        for k in POSES[name]:
            _frame(gh, r, name, k)
            planes = r.read_depth()
            refs(name, k).check(planes, ("bounds", throughput, k))
            _pick_equals_planes(gh, r, planes)
        _bounds_zero(r, ("bounds", throughput))
        r.dispose()
    r = _overflow_is_repaired(gh, scenes, name, lib_path=BOUNDS_LIB)
    _bounds_zero(r, "overflow")
    r.dispose()


def test_skip_changes_no_bit(gh, monkeypatch, scenes):
    for name, k in (("C2", POSES["C2"][0]), ("C3", POSES["C3"][0])):
        got = []
        for env in ({}, {"GSR_DEPTH_SKIP": "0"}):
            r = _context(gh, monkeypatch, name, scenes, env=env, throughput=True)
            _frame(gh, r, name, k)
            planes = r.read_depth()
            if name == "C3":
                x0, y0, w, h = _window(name, gh)
                planes = tuple(a[y0:y0 + h, x0:x0 + w] for a in planes)
            got.append(planes)
            r.dispose()
        assert (got[0][2] != NONE).any()
        for a, b in zip(*got):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


# 11 ------------------------------------------------------------------------------------------------------------------
# The walk at its chunk edges (chunks of 256 entries): L - 1 faint co-located splats over the whole 96 x 96 frame (3 x 3 bins) and one
# opaque splat behind them, so that every bin's list has exactly L entries, every entry adds a term to the mean plane and, at
# hit_alpha 0.9, the only possible hit is the list's last entry.  (At 0.5 the reference's own knife-edge mask is 4.6 % to 15.8 %
# of these frames; at 0.9 it is at most 0.0009, far inside the 1 % Ref.check allows.)
STACK_LENGTHS = (1, 255, 256, 257, 512, 513)
STACK_HIT_ALPHA = 0.9


@pytest.fixture(scope="module")
def stack_refs(oracle):
    """length -> the scene and its reference planes: computed once, shared with the bounds twin, dropped with the module"""
    cache = {}

    def get(length):
        if length not in cache:
            W, H = BR.STACK_FRAME
            cam, to_world = BR.front_view(W, H)
            splats = BR.stack(to_world, 48, 48, length - 1, 100.0, (90, 160, 220, 1)) + BR.stack(to_world, 48, 48, 1, 100.0, (255, 230, 40, 255), dz0=1.0)
            cache[length] = Ref.of_scene(oracle, cam, *make_scene(oracle, splats), W, H, STACK_HIT_ALPHA)
            assert np.array_equal(cache[length].order, np.arange(length))
        return cache[length]

    yield get
    cache.clear()


def _stack_at_the_chunk_edges(gh, ref, monkeypatch, length, lib_path=None):
    W, H = BR.STACK_FRAME
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    kw = {} if lib_path is None else {"lib_path": lib_path}
    r = gh.HIPRenderer(W, H, **kw)
    r.set_raw_scene(ref.data, ref.pos)
    r.set_hit_alpha(STACK_HIT_ALPHA)
    r.set_camera(ref.cam)
    r.render_async()
    r.sync()
    assert r.stats()["bin_entries"] == 9 * length and r.stats()["overflow_frames"] == 0
    planes = r.read_depth()
    ref.check(planes, ("stack", length, lib_path is not None))
    mean, hit, index = planes
    assert (index == length - 1).any() and np.all((index == length - 1) | (index == NONE) | ref.planes["mask"])
    # pick: the centre, a corner and one pixel of each bin
    _pick_at(r, planes, [(48, 48), (W - 1, 0)] + [(32 * bx + 5 + 7 * by, 32 * by + 11 + 6 * bx) for by in range(3) for bx in range(3)])
    # the strided pass: the samples of a depth ring (f32, step 2) are the hit plane at (2i, 2j)
    r.open_delivery_depth(2, depth="f32", depth_step=2)
    r.render_async()
    s, _, depth = r.acquire(r.deliver())
    want = np.ascontiguousarray(hit[::2, ::2])
    assert depth.shape == want.shape and np.array_equal(depth.view(np.uint32), want.view(np.uint32)), (length, "strided pass")
    r.release(s)
    r.close_delivery()
    return r


@pytest.mark.parametrize("length", STACK_LENGTHS)
def test_depth_at_the_chunk_edges(gh, stack_refs, monkeypatch, length):
    ref = stack_refs(length)
    _stack_at_the_chunk_edges(gh, ref, monkeypatch, length).dispose()
    if length in (256, 257):
        assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
        r = _stack_at_the_chunk_edges(gh, ref, monkeypatch, length, lib_path=BOUNDS_LIB)
        _bounds_zero(r, ("bounds", "stack", length))
        r.dispose()

"""The contribution pass on the GPU (k_contrib.hip, gsr_contrib.cpp) against tests/contrib_reference.py -- the specification in
numpy, fed by the oracle's projection and sort, never by device read-backs -- in every form the frame in front of it runs in,
for accumulation in either order, band contexts, a shared scene, the selection it feeds and the bounds-checked twin.
pixels is compared EXACTLY (coverage is bit-exact, DESIGN.md 5.5 group A); weight and peak within their derived bounds."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import blend_reference as BR
import contrib_reference as CR
from test_oracle_render import make_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
KNOBS = ("GSR_BIN_TWO_LEVEL", "GSR_LONG_ITEMS", "GSR_DEPTH_SKIP")
GSR_ERR_ARG = -1
NAME, POSES = "C1", (3, 40)
W, H = 640, 480
STACKS = (1, 255, 256, 257, 512, 513, 4100)
RATIOS = {}     # what -> (largest |gpu - ref| / bound of weight, of peak), printed at the end of the module: DESIGN.md 5.8 quotes it


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    yield gsplat_hip
    for what in sorted(RATIOS):
        print("\ncontrib: max |gpu - ref| / bound  %-28s weight %.3f  peak %.3f" % ((what,) + RATIOS[what]), end="")


def _cam(gh, k, w=W, h=H):
    cfg = gh.synth.CONFIGS[NAME]
    return gh.orbit_camera(k, width=w, height=h, fx=cfg["fx"] * w / W)


def _view(oracle, cam, data, pos, w, h, window=None):
    v, p, vp = cam.f32()
    rec, bbox, _ = oracle.project(data, v, p, cam.fx, cam.fy, w, h)
    view = (rec, bbox, oracle.sort(vp, pos)[0], w, h)
    return view + (window,) if window else view


@pytest.fixture(scope="module")
def c1(oracle, scenes, gh):
    """the oracle's views of C1 at both poses and the reference of both accumulated: computed once, shared, never changed"""
    _, data, pos = scenes(NAME)
    views = [_view(oracle, _cam(gh, k), data, pos, W, H) for k in POSES]
    ref = CR.contrib_reference(views, gh.synth.CONFIGS[NAME]["n"])
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return views, ref


def _context(gh, monkeypatch, scenes, env=None, name=NAME, seed=None, w=W, h=H, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    r = gh.HIPRenderer(w, h, **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)
    if name is not None:
        r.set_scene_rows(scenes(name, seed)[0])
    return r


def _frame(gh, r, k):
    r.set_camera(_cam(gh, k, r.width, r.height))
    r.render_async()
    r.sync()
    assert r.stats()["overflow_frames"] == 0


def _tour(gh, r, poses=POSES, reset=True):
    if reset:
        r.contrib_reset()
    for k in poses:
        _frame(gh, r, k)
        r.contrib_accumulate()
    return r.read_contrib()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what):
    for x, y, name in zip(a[:3], b[:3], ("weight", "peak", "pixels")):
        bad = np.nonzero(_bits(x) != _bits(y))[0]
        assert not bad.size, (what, name, bad[:4].tolist(), x[bad[:4]].tolist(), y[bad[:4]].tolist())


def _inside(got, ref, what):
    """pixels word for word, weight and peak inside their bounds for every splat, the types the header states"""
    weight, peak, pixels = got[:3]
    assert weight.dtype == np.uint64 and peak.dtype == np.float32 and pixels.dtype == np.uint32, what
    bad = np.nonzero(pixels != ref["pixels"])[0]
    assert not bad.size, (what, "pixels", bad[:4].tolist(), pixels[bad[:4]].tolist(), ref["pixels"][bad[:4]].tolist())
    ratios = CR.excess(got, ref)
    print("contrib", what, "max |gpu - ref| / bound: weight %.3f peak %.3f" % ratios)
    RATIOS[str(what)] = ratios
    assert ratios[0] <= 1.0 and ratios[1] <= 1.0, (what, ratios)


def _bounds_zero(r, what):
    for name in ("gsr_debug_bounds_contrib", "gsr_debug_bounds_depth", "gsr_debug_bounds_select"):
        buf = (ctypes.c_uint32 * 8)()
        assert getattr(r._L, name)(buf) == 0
        assert not any(buf), (what, name, list(buf))


@pytest.fixture(scope="module")
def base(gh, scenes):
    """what a default context accumulates over both poses: the arrays every other form must reproduce bit for bit"""
    with pytest.MonkeyPatch.context() as mp:
        r = _context(gh, mp, scenes)
        got = _tour(gh, r)
        r.dispose()
    for a in got[:3]:
        a.flags.writeable = False
    return got


# 1 -------------------------------------------------------------------------------------------------------------------
def test_c1_lies_inside_the_specification(gh, base, c1):
    views, ref = c1
    assert base[3] == 2 == ref["frames"]
    _inside(base, ref, "C1 poses 3 + 40")
    assert (base[2] > 0).sum() > 1000 and (base[2] == 0).sum() > 100 and base[1].max() <= 1.0


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["throughput", "two level", "short items", "long items"])
def test_every_form_gives_the_same_bits(gh, monkeypatch, scenes, base, form):
    env = {"two level": {"GSR_BIN_TWO_LEVEL": "1"}, "short items": {"GSR_LONG_ITEMS": "0"}, "long items": {"GSR_LONG_ITEMS": "1"}}.get(form)
    r = _context(gh, monkeypatch, scenes, env=env, throughput=form == "throughput")
    got = _tour(gh, r)
    assert got[3] == 2
    _same(got, base, form)
    r.dispose()


def _digest(arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays[:3])).hexdigest()


def test_without_the_tile_skip_in_a_child_process(gh, base):
    code = ("import sys, hashlib, numpy as np; sys.path[:0] = %r; import gsplat_hip as gh\n"
            "cfg = gh.synth.CONFIGS[%r]; r = gh.HIPRenderer(%d, %d); r.set_scene_rows(gh.synth.config_rows(%r)); r.contrib_reset()\n"
            "for k in %r:\n"
            "    r.set_camera(gh.orbit_camera(k, width=%d, height=%d, fx=cfg['fx'])); r.render_async(); r.sync(); r.contrib_accumulate()\n"
            "a = r.read_contrib(); print('digest', hashlib.sha256(b''.join(x.tobytes() for x in a[:3])).hexdigest(), a[3])\n"
            % ([p for p in sys.path if p], NAME, W, H, NAME, POSES, W, H))
    env = dict(os.environ, GSR_DEPTH_SKIP="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "digest %s 2" % _digest(base) in out.stdout, out.stdout[-500:]


def test_either_order_of_the_poses(gh, monkeypatch, scenes, base):
    r = _context(gh, monkeypatch, scenes)
    got = _tour(gh, r, POSES[::-1])
    _same(got, base, "pose B then A")
    r.dispose()


def test_two_bands_add_up_to_the_frame(gh, monkeypatch, scenes, base, c1, oracle):
    halves = []
    for band in ((0, 320), (320, 640)):
        r = _context(gh, monkeypatch, scenes, band=band)
        halves.append(_tour(gh, r))
        r.dispose()
    assert (halves[0][2] > 0).any() and (halves[1][2] > 0).any() and not np.array_equal(halves[0][2], halves[1][2])
    _same(CR.combine(*halves), base, "bands [0, 320) + [320, 640)")
    views, _ = c1
    left = CR.contrib_reference([v + ((0, 0, 320, H),) for v in views], base[0].size)
    _inside(halves[0], left, "band [0, 320)")


# 3 -------------------------------------------------------------------------------------------------------------------
STACK_REFS = {}   # length -> the scene, the oracle's view and the reference: computed once, shared with the bounds twin


def _stack(gh, oracle, monkeypatch, length, lib_path=None):
    Ws, Hs = BR.STACK_FRAME
    if length not in STACK_REFS:
        cam, splats, last = CR.hidden_stack_scene(length)
        data, pos = make_scene(oracle, splats)
        view = _view(oracle, cam, data, pos, Ws, Hs)
        STACK_REFS[length] = (cam, last, data, pos, view, CR.contrib_reference([view], len(splats)))
    cam, last, data, pos, view, ref = STACK_REFS[length]
    r = _context(gh, monkeypatch, None, name=None, w=Ws, h=Hs, lib_path=lib_path)
    r.set_raw_scene(data, pos)
    r.set_camera(cam)
    r.render_async()
    r.sync()
    r.contrib_accumulate()          # (no reset in front: the first call does what a reset does)
    got = r.read_contrib()
    assert got[3] == 1
    assert r.stats()["bin_entries"] >= 9 * length
    _inside(got, ref, ("stack", length))
    weight, peak, pixels = got[:3]
    # the front splat, from that splat alone: T = 1, so w = B
    rec = view[0]
    q = BR.coverage_q(rec[0], np.arange(Ws), np.arange(Hs))
    B = np.exp2(BR.exponent(q, rec[0, 6]).astype(np.float64))[q <= 4]
    assert pixels[0] == B.size and abs(float(weight[0]) - np.rint(B * 2.0 ** 24).sum()) <= ref["weight_bound"][0]
    if length >= 255:               # T is exactly 0 under the hidden splat long before the stack ends
        assert pixels[last] > 50 and weight[last] == 0 and peak[last] == 0.0, (length, pixels[last], weight[last], peak[last])
    else:
        assert pixels[last] > 50 and weight[last] > 0 and peak[last] > 0.0
    return r


@pytest.mark.parametrize("length", STACKS)
def test_stacks(gh, oracle, monkeypatch, length):
    _stack(gh, oracle, monkeypatch, length).dispose()


def _giant(gh, oracle, monkeypatch, lib_path=None):
    """A full-opacity giant at the projection's 1024-pixel axis clamp over the 96 x 96 frame: every wave's sum of quanta is just
    under 2^32 (w == 1.0f exactly is reached at the centre pixel only: the clamp leaves q = 3.8e-6 d^2 at d pixels from it),
    past 31 bits and past what a 32-bit sum of more than one 16-lane row holds together with a second tile's."""
    Ws, Hs = BR.STACK_FRAME
    cam, to_world = BR.front_view(Ws, Hs)
    splats = BR.stack(to_world, 48.5, 48.5, 1, 20000.0, (255, 255, 255, 255))
    data, pos = make_scene(oracle, splats)
    view = _view(oracle, cam, data, pos, Ws, Hs)
    ref = CR.contrib_reference([view], 1)
    r = _context(gh, monkeypatch, None, name=None, w=Ws, h=Hs, lib_path=lib_path)
    r.set_raw_scene(data, pos)
    r.set_camera(cam)
    r.render_async()
    r.sync()
    r.contrib_accumulate()
    weight, peak, pixels, frames = r.read_contrib()
    assert frames == 1
    _inside((weight, peak, pixels), ref, "giant")
    assert pixels[0] == Ws * Hs and peak[0] == 1.0
    assert weight[0] > 0.98 * pixels[0] * 2.0 ** 24 and weight[0] <= int(pixels[0]) << 24
    assert int(weight[0]) // 36 > 2 ** 31           # per tile (36 of them): beyond a signed 32-bit sum
    return r


def test_giant_wave_sums(gh, oracle, monkeypatch):
    _giant(gh, oracle, monkeypatch).dispose()


@pytest.mark.parametrize("n", [1, 33, 1025])
def test_small_scenes_on_a_frame_with_partial_bins(gh, oracle, monkeypatch, scenes, n):
    w, h = 200, 150                 # 7 x 5 bins, the last column 8 pixels wide, the last row 22 high
    r = _context(gh, monkeypatch, scenes, name=n, seed=7, w=w, h=h)
    _, data, pos = scenes(n, 7)
    got = _tour(gh, r)
    views = [_view(oracle, _cam(gh, k, w, h), data, pos, w, h) for k in POSES]
    _inside(got, CR.contrib_reference(views, n), ("scene of", n))
    r.dispose()


# 4 -------------------------------------------------------------------------------------------------------------------
def _values(arrays):
    return {"weight": arrays[0].astype(np.float64) * 2.0 ** -24, "peak": arrays[1].astype(np.float64), "pixels": arrays[2].astype(np.float64)}


def _selection_is(r, want, what):
    got = r.selection()
    bad = np.nonzero(got != want)[0]
    assert not bad.size and r.selection_count() == int(want.sum()), (what, bad[:4].tolist())


def test_select_contrib_and_erase(gh, monkeypatch, scenes):
    r = _context(gh, monkeypatch, scenes)
    n = r.scene_count()
    with pytest.raises(gh.GsplatError, match="frames == 0") as ei:       # never reset, never accumulated
        r.select_contrib("weight", 1.0)
    assert ei.value.code == GSR_ERR_ARG
    r.contrib_reset()
    with pytest.raises(gh.GsplatError, match="frames == 0") as ei:       # an empty tour must not select the whole scene
        r.select_contrib("pixels", 1.0)
    assert ei.value.code == GSR_ERR_ARG and r.selection_count() == 0
    arrays = _tour(gh, r, reset=False)
    vals = _values(arrays)
    for stat, v in vals.items():
        own = float(np.sort(v[v > 0])[v[v > 0].size // 2])               # a value equal to one splat's own: `<` leaves that splat out
        for below in (0.0, own, float("inf")):
            want = v < below
            assert r.select_contrib(stat, below) == int(want.sum()), (stat, below)
            _selection_is(r, want, (stat, below))
        assert 0 < (v < own).sum() < n and (v == own).any()
    S = np.arange(n) % 3 == 0
    P = vals["peak"] < 0.01
    assert 0 < (S & P).sum() < P.sum() < n
    for op, want in (("replace", P), ("add", S | P), ("subtract", S & ~P), ("intersect", S & P)):
        r.set_selection(S)
        assert r.select_contrib("peak", 0.01, op=op) == int(want.sum()), op
        _selection_is(r, want, op)
    for bad in (lambda: r.select_contrib(3, 1.0), lambda: r.select_contrib(-1, 1.0), lambda: r.select_contrib("weight", 1.0, op=4),
                lambda: r.select_contrib("weight", float("nan"))):
        with pytest.raises(gh.GsplatError) as ei:
            bad()
        assert ei.value.code == GSR_ERR_ARG
    _selection_is(r, S & P, "after the refusals")
    # prune what never showed, then the next frame is that of a fresh context given the compacted arrays
    never = vals["pixels"] < 1.0
    assert r.select_contrib("pixels", 1.0) == int(never.sum()) and 0 < never.sum() < n
    before = r.read_scene()
    assert r.scene_erase_selected() == n - int(never.sum())
    after = r.read_scene()
    for a, b, per in zip(after, before, (8, 3, 4, 3)):
        assert np.array_equal(_bits(a), _bits(b.reshape(n, per)[~never].reshape(-1))), per
    fresh = gh.HIPRenderer(W, H)
    fresh.set_scene_arrays(*after)
    for c in (r, fresh):
        _frame(gh, c, POSES[1])
    assert np.array_equal(_bits(r.readPixelsFloat()), _bits(fresh.readPixelsFloat()))
    # (what never had a fragment changes no pixel of the views it was judged from)
    with pytest.raises(gh.GsplatError) as ei:                            # a removing erase dropped the accumulators
        r.read_contrib()
    assert ei.value.code == GSR_ERR_ARG
    fresh.dispose(); r.dispose()


# 5 -------------------------------------------------------------------------------------------------------------------
def test_state_rules(gh, monkeypatch, scenes):
    r = _context(gh, monkeypatch, scenes)
    n = r.scene_count()
    bytes0 = r.scene_sharing()[1]
    with pytest.raises(gh.GsplatError, match="ever reset") as ei:
        r.read_contrib()
    assert ei.value.code == GSR_ERR_ARG
    with pytest.raises(gh.GsplatError, match="no frame") as ei:          # what gsr_depth_async demands of the frame
        r.contrib_accumulate()
    assert ei.value.code == GSR_ERR_ARG and r.scene_sharing()[1] == bytes0
    r.contrib_reset()
    assert r.scene_sharing()[1] == bytes0 + 16 * n + 8                   # 16 bytes per splat row plus the counter words
    got = _tour(gh, r, POSES[:1], reset=False)
    assert got[3] == 1 and got[2].any()
    assert r._L.gsr_read_contrib(r._ctx, None, None, None, n - 1, None) == GSR_ERR_ARG
    assert r._L.gsr_read_contrib(r._ctx, None, None, None, n, None) == 0  # any output may be NULL
    r.sort()
    with pytest.raises(gh.GsplatError, match="sort-only"):
        r.contrib_accumulate()
    for edit in (lambda: r.scene_translate((0.5, 0.0, 0.0)), lambda: r.scene_rotate((0.0, 0.0, 0.38268343, 0.92387953)), lambda: r.scene_scale((1.5, 1.5, 1.5))):
        edit()
        _same(r.read_contrib(), got, "kept across an edit")
        with pytest.raises(gh.GsplatError, match="no frame"):            # the frame is of another scene: nothing enqueued
            r.contrib_accumulate()
    assert r.read_contrib()[3] == 1
    r.contrib_reset()
    z = r.read_contrib()
    assert z[3] == 0 and not z[0].any() and not z[1].any() and not z[2].any()
    assert r.scene_limit_box((-100.0, 100.0, -100.0, 100.0, -100.0, 100.0)) == n    # removes nothing, and still drops them
    with pytest.raises(gh.GsplatError, match="ever reset"):
        r.read_contrib()
    assert r.scene_sharing()[1] == bytes0
    r.contrib_reset()
    r.set_scene_rows(scenes(NAME)[0])
    with pytest.raises(gh.GsplatError, match="ever reset"):
        r.read_contrib()
    r.contrib_reset()
    r.set_selection(None)
    assert r.scene_erase_selected() == n and r.read_contrib()[3] == 0    # an erase that removes nothing keeps them
    r.dispose()


def test_shared_scene_has_one_set(gh, monkeypatch, scenes, base):
    a = _context(gh, monkeypatch, scenes)
    b, c = gh.HIPRenderer(W, H, throughput=True), gh.HIPRenderer(W, H)
    b.share_scene(a)
    c.share_scene(a)
    a.contrib_reset()
    for m, k in ((a, POSES[0]), (b, POSES[1])):                          # two members, their own streams, no wait in between
        m.set_camera(_cam(gh, k))
        m.render_async()
        m.contrib_accumulate()
    got = c.read_contrib()                                               # read through a third, which never rendered
    assert got[3] == 2
    _same(got, base, "two members, read through a third")
    for m in (a, b):
        m.sync()
        assert m.stats()["overflow_frames"] == 0
    assert a.scene_sharing() == b.scene_sharing() == c.scene_sharing()
    c.set_scene_rows(scenes(NAME)[0])                                    # a member that leaves starts empty; the others keep theirs
    with pytest.raises(gh.GsplatError, match="ever reset"):
        c.read_contrib()
    _same(a.read_contrib(), base, "after a member left")
    for x in (a, b, c):
        x.dispose()


# 6 -------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(gh, monkeypatch, scenes):
    plain = _context(gh, monkeypatch, scenes)
    r = _context(gh, monkeypatch, scenes)
    for c in (plain, r):
        _frame(gh, c, POSES[0])
    pts = [(320, 240), (100, 100), (317, 243)]
    state = lambda c: (c.readPixelsFloat(), c.lastDepthIndex(), c.work_items(), c.stats(), c.read_depth(), c.pick(pts))

    def same(x, y, what, stats=True):
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1]) and x[2] == y[2] and (x[3] == y[3] or not stats), what
        assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(x[4], y[4])) and np.array_equal(x[5], y[5]), what

    before = state(r)
    for k, call in enumerate((r.contrib_reset, r.contrib_accumulate, r.read_contrib, lambda: r.select_contrib("pixels", 1.0), r.contrib_accumulate)):
        call()
        same(state(r), before, k)
    same(state(r), state(plain), "a context that never ran it", stats=False)
    for c in (plain, r):
        _frame(gh, c, POSES[1])
    r.contrib_accumulate()
    same(state(r), state(plain), "the next frame", stats=False)
    assert r.read_contrib()[3] == 3
    plain.dispose(); r.dispose()


# 7 -------------------------------------------------------------------------------------------------------------------
def test_a_frame_that_did_not_fit_adds_nothing(gh, monkeypatch, scenes, base):
    r = _context(gh, monkeypatch, scenes)
    one = _tour(gh, r, POSES[:1])
    assert r.stats()["bin_entries"] > 4096
    r.set_list_capacity(1024)                                            # far too small for the next frame (the handled regrowth path)
    r.set_camera(_cam(gh, POSES[1]))
    r.render_async()
    r.contrib_accumulate()                                               # behind a frame whose lists did not fit
    got = r.read_contrib()
    assert got[3] == 1
    _same(got, one, "an unfit frame")
    r.sync()                                                             # the lists are regrown, the frame is rendered again
    assert r.stats()["overflow_frames"] == 1
    r.set_camera(_cam(gh, POSES[1]))
    r.render_async()
    r.sync()
    r.contrib_accumulate()
    got = r.read_contrib()
    assert got[3] == 2
    _same(got, base, "the repeated pose")
    r.dispose()


# 8 -------------------------------------------------------------------------------------------------------------------
def test_bounds_twin(gh, oracle, monkeypatch, scenes, c1):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    r = _context(gh, monkeypatch, scenes, lib_path=BOUNDS_LIB)
    got = _tour(gh, r)
    _inside(got, c1[1], "bounds C1")
    assert r.select_contrib("pixels", 1.0) == int((got[2] == 0).sum())
    _bounds_zero(r, "C1")
    r.dispose()
    for length in STACKS:
        r = _stack(gh, oracle, monkeypatch, length, lib_path=BOUNDS_LIB)
        _bounds_zero(r, ("stack", length))
        r.dispose()
    r = _giant(gh, oracle, monkeypatch, lib_path=BOUNDS_LIB)
    _bounds_zero(r, "giant")
    r.dispose()

"""The compositor (k_blend / k_blend2, k_combine) against tests/blend_reference.py -- the colour of every pixel in f64 with
a derived bound of what f32 may do to it, fed by the oracle's projection and sort, never by device read-backs -- in every
form the kernel runs in: one and two waves per tile, whole-bin and segmented work items, the fold inside the compositor
and as a separate launch, a band context, throughput contexts in flight, and the bounds-checked twin of the library.
Coverage ({alpha > 0} against {some q <= 4}) is compared EXACTLY: no mask, no tolerance.
Groups: A coverage and the hardware exponential, B dense frames, C the benchmarked configuration, D saturation and early
termination at their edges, E work-item boundaries and the fold."""
import ctypes
import os

import numpy as np
import pytest

import blend_reference as BR
from test_oracle_render import make_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
KNOBS = ("GSR_BLEND_SUB", "GSR_LONG_ITEMS", "GSR_FUSE_COMBINE", "GSR_SATURATE", "GSR_SEG_LEN", "GSR_SEG_TARGET")
TOL_EXACT = 2e-4
# name -> (environment at creation, constructor arguments, waves per tile the form must run with: None = by the bin count)
FORMS = {
    "default": ({}, {}, None),
    "throughput": ({}, {"throughput": True}, 1),
    "sub1": ({"GSR_BLEND_SUB": "1"}, {}, 1),
    "sub2": ({"GSR_BLEND_SUB": "2"}, {}, 2),
    "short": ({"GSR_LONG_ITEMS": "0"}, {}, None),
    "long": ({"GSR_LONG_ITEMS": "1"}, {}, None),
    "unfused": ({"GSR_FUSE_COMBINE": "0", "GSR_LONG_ITEMS": "0"}, {}, None),
    "band": ({}, {"band": True}, None),
    "bounds": ({}, {"lib_path": BOUNDS_LIB}, None),
}
ALL = tuple(FORMS)
RATIOS = {}     # what -> largest |gpu - ref| / bound seen (printed at the end of the module: DESIGN.md 5.5 quotes it)


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    yield gsplat_hip
    for what in sorted(RATIOS):
        print("\nblend: max |gpu - ref| / bound  %-40s %.3f" % (what, RATIOS[what]), end="")


class Frame:
    """One (scene, camera) on a W x H frame: the oracle's records and order, and the reference of some windows."""

    def __init__(self, oracle, data, pos, cam, W, H, windows=None, **project_kw):
        self.data, self.pos, self.cam, self.W, self.H = data, pos, cam, W, H
        v, p, vp = cam.f32()
        self.rec, self.bbox, self.raw = oracle.project(data, v, p, cam.fx, cam.fy, W, H, **project_kw)
        self.order = oracle.sort(vp, pos)[0]
        self.refs = {win: BR.blend_reference(self.rec, self.bbox, self.raw, self.order, W, H, win) for win in (windows or [(0, 0, W, H)])}

    def check(self, img, what, eps=0.0, cover=False, columns=None):
        """img f32[H, W, 4] within the bound on every pixel of every window (columns: of a band context, these only)"""
        worst = 0.0
        for (x0, y0, w, h), ref in self.refs.items():
            xa, xb = (x0, x0 + w) if columns is None else (max(x0, columns[0]), min(x0 + w, columns[1]))
            if xa >= xb:
                continue
            got = img[y0:y0 + h, xa:xb].astype(np.float64)
            sl = (slice(None), slice(xa - x0, xb - x0))
            bound = ref["bound"][sl] + eps
            ratio = np.abs(got - ref["rgba"][sl]) / bound
            if cover:
                lit, kept = got[..., 3] > 0.0, ref["kept"][sl] > 0
                assert np.array_equal(lit, kept), (what, "covered pixels differ", np.argwhere(lit != kept)[:4].tolist(), int((lit != kept).sum()))
            bad = ratio > 1.0
            assert not bad.any(), (what, (x0, y0, w, h), int(bad.sum()), float(ratio.max()), np.argwhere(bad)[:4].tolist())
            worst = max(worst, float(ratio.max()))
        key = what if isinstance(what, str) else " ".join(str(x) for x in what)
        RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
        return worst


def _context(gh, monkeypatch, form, W, H, window=None, env=None, **kw):
    fenv, fkw, _ = FORMS[form]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    fenv = dict(fenv, **(env or {}))
    for k, v in fenv.items():
        monkeypatch.setenv(k, v)
    fkw = dict(fkw, **kw)
    columns = None
    if fkw.get("band") is True:       # the 32-pixel columns around the window's middle (or the frame's)
        mid = (window[0] + window[2] // 2) if window else W // 2
        columns = (max(mid // 32 * 32 - 64, 0), min(mid // 32 * 32 + 64, W))
        fkw["band"] = columns
    if "lib_path" in fkw:
        assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    r = gh.HIPRenderer(W, H, **fkw)
    for k in fenv:
        monkeypatch.delenv(k)
    return r, columns


def _render(r, fr):
    r.set_raw_scene(fr.data, fr.pos)
    r.set_camera(fr.cam)
    r.render_async()
    r.sync()
    assert r.stats()["overflow_frames"] == 0
    return r.readPixelsFloat()


def _ran_as(r, form, env=None):
    """the form really ran: the kernel (waves per tile) and the cut of the lists"""
    wi = r.work_items()
    want = FORMS[form][2]
    if want is None:
        want = 2 if wi["bins"] <= 4096 else 1
    assert wi["waves_per_tile"] == want, (form, wi)
    fenv = dict(FORMS[form][0], **(env or {}))
    if fenv.get("GSR_LONG_ITEMS") == "1":
        assert wi["items"] == wi["bins"], (form, wi)
    if fenv.get("GSR_LONG_ITEMS") == "0":
        assert wi["items"] >= wi["bins"], (form, wi)
    if "GSR_SEG_LEN" in fenv:
        assert wi["seg_len"] == int(fenv["GSR_SEG_LEN"]), (form, wi)
    return wi


def _bounds_zero(r, what):
    buf = (ctypes.c_uint32 * 8)()
    assert r._L.gsr_debug_bounds_blend(buf) == 0
    assert not any(buf), (what, list(buf))


def _forms(gh, monkeypatch, fr, what, forms=ALL, env=None, cover=False, rgba8=True, window=None):
    """render fr in each form, check it against the reference; name -> image"""
    imgs = {}
    for form in forms:
        r, columns = _context(gh, monkeypatch, form, fr.W, fr.H, window=window or next(iter(fr.refs)), env=env)
        img = _render(r, fr)
        _ran_as(r, form, env)
        fr.check(img, (what, form), cover=cover, columns=columns)
        if rgba8:      # readPixels() is the stated rounding of readPixelsFloat(), bit for bit
            assert np.array_equal(r.readPixels().reshape(fr.H, fr.W, 4), BR.to_rgba8(img)), (what, form)
        if form == "bounds":
            _bounds_zero(r, what)
        r.dispose()
        imgs[form] = img
    return imgs


# A -------------------------------------------------------------------------------------------------------------------
def _regions(W, H):
    if W * H <= 1000 * 712:
        return [(0, 0, W, H)]
    # large frames: the reference is evaluated on windows -- a corner at the origin, the far corner (partial bins, far bin
    # coordinates) and the middle -- and the splats are placed there
    return [(0, 0, 192, 192), (W - 192, H - 192, 192, 192), (W // 2 - 96, H // 2 - 96, 192, 192)]


@pytest.fixture(scope="module")
def exp_error():
    seen = {"max": 0.0, "pixels": 0}
    yield seen
    print("\nblend: v_exp_f32 on %d single-fragment pixels: max relative error %.3g = %.2f * 2^-23 (E_EXP = 2^-22)"
          % (seen["pixels"], seen["max"], seen["max"] * 2.0 ** 23), end="")


@pytest.mark.parametrize("size", [(640, 480), (1000, 712), (322, 241), (3840, 2160), (8192, 8192)], ids=lambda s: "%dx%d" % s)
def test_coverage_is_exact_and_the_exponential_as_accurate_as_assumed(gh, oracle, monkeypatch, exp_error, size):
    W, H = size
    regions = _regions(W, H)
    cam, splats = BR.coverage_scene(W, H, regions, seed=5 + W, per_region=1200 if len(regions) == 1 else 400, giants=(W == 322))
    data, pos = make_scene(oracle, splats)
    fr = Frame(oracle, data, pos, cam, W, H, windows=regions)
    pairs = sum(BR.small_quadrant_pairs(fr.rec, fr.bbox, fr.order, W, H, win) for win in regions)
    assert pairs >= 300, pairs
    forms = ALL if W == 640 else ("default", "throughput", "sub1", "sub2", "short", "long") if W <= 1000 else ("default", "throughput")
    imgs = _forms(gh, monkeypatch, fr, "A %dx%d" % size, forms=forms, cover=True, rgba8=W <= 1000)
    # single-fragment pixels: T = 1, so red = fma(w, 1.0f, 0) = w = v_exp_f32(a) exactly (every splat here has red 255,
    # and 255 * (1.0f / 255.0f) is 1.0f): the hardware exponential against 2^a, on the arguments it really sees.  This ONE
    # measurement takes la from the device's records (the projection's v_log_f32), so that it measures v_exp_f32 alone; the
    # device's la itself is held to E_LA of the oracle's.  Every image comparison above used the oracle's la.
    vis = fr.raw[:, 11] == 1
    assert BR.colours(fr.rec, fr.raw)[vis, 0].min() == 1.0
    r, _ = _context(gh, monkeypatch, "default", W, H)
    again = _render(r, fr)
    la_dev = r.read_records()[0][:, 6]
    r.dispose()
    assert np.array_equal(again, imgs["default"])
    assert np.all(np.abs(la_dev[vis].astype(np.float64) - fr.rec[vis, 6]) <= BR.E_LA * np.maximum(1.0, np.abs(fr.rec[vis, 6])))
    for win, ref in fr.refs.items():
        x0, y0, w, h = win
        one = ref["kept"] == 1
        if not one.any():
            continue
        px = BR.Pixels(h, w)
        for i, sl, q in BR.fragments(fr.rec, fr.bbox, fr.order, W, H, win):
            px.add(sl, q, la_dev[i], (1.0, 1.0, 1.0))
        want = px.result()["rgba"][..., 0][one]
        for form in ("default", "throughput"):
            got = imgs[form][y0:y0 + h, x0:x0 + w, 0].astype(np.float64)[one]
            rel = np.abs(got / want - 1.0)
            assert rel.max() <= BR.E_EXP + 2 * BR.U, (size, form, rel.max())
            exp_error["max"] = max(exp_error["max"], float(rel.max()))
            exp_error["pixels"] += int(one.sum())
    if W == 640:
        assert exp_error["pixels"] > 10000


# B -------------------------------------------------------------------------------------------------------------------
def _config_frame(gh, oracle, scenes, name, k, windows):
    cfg = gh.synth.CONFIGS[name]
    _, data, pos = scenes(name)
    cam = gh.orbit_camera(k, width=cfg["width"], height=cfg["height"], fx=cfg["fx"])
    return Frame(oracle, data, pos, cam, cfg["width"], cfg["height"], windows=windows)


def _windows(gh, name):
    """a centre window (bins saturate, lists are long) and a rim window (sparse, cut into segments) of the large scenes"""
    cfg = gh.synth.CONFIGS[name]
    W, H = cfg["width"], cfg["height"]
    if name == "C1":
        return None
    if name == "C4":
        return [(W // 2 - 48, H // 2 - 48, 96, 96)]
    dx, dy = (256, -160) if name == "C2" else (560, -340)
    return [(W // 2 - 64, H // 2 - 64, 128, 128), (W // 2 - 64 + dx, H // 2 - 64 + dy, 128, 128)]


@pytest.fixture(scope="module")
def frames(gh, oracle, scenes):
    cache = {}

    def get(name, k):
        if (name, k) not in cache:
            cache[(name, k)] = _config_frame(gh, oracle, scenes, name, k, _windows(gh, name))
        return cache[(name, k)]

    yield get
    cache.clear()


@pytest.mark.parametrize("name,k", [("C1", 3), ("C1", 40), ("C2", 13), ("C3", 21), ("C3", 84), ("C4", 50)])
def test_dense_frames_lie_inside_the_bound_in_every_form(gh, monkeypatch, frames, name, k):
    fr = frames(name, k)
    forms = ALL if name in ("C1", "C3") and k in (3, 21) else ("default", "throughput", "sub1", "sub2", "short", "long", "unfused")
    if name == "C4":
        forms = ("default", "throughput", "short")
    for ref in fr.refs.values():
        assert ref["kept"].max() > 10
    if name == "C3":      # the centre saturates behind long lists, the rim does not
        centre, rim = list(fr.refs.values())
        assert centre["T"].max() < 1e-12 and centre["kept"].min() > 500 and rim["T"].max() > 0.01
    _forms(gh, monkeypatch, fr, "B %s pose %d" % (name, k), forms=forms)


def test_sh_colours_and_depth_fade_lie_inside_the_bound(gh, oracle, scenes, monkeypatch):
    n, (W, H) = 40000, (640, 480)
    rows, data, pos = scenes(n, 41)
    rng = np.random.default_rng(8)
    b0, b1, b2 = 9999, 19999, 29999          # test_sh_colour_parity's scene: splats 0..9999 plain, then degree 1, 2, 3
    shs = (rng.standard_normal((n - (b0 + 1), 48)) * 0.35).astype(np.float32)
    scene = gh.Scene()
    scene.bandsIndices = np.array([b0, b1, b2], dtype=np.int32)
    scene.setData(rows, shs)
    cam = gh.orbit_camera(33, width=W, height=H)
    fr = Frame(oracle, data, pos, cam, W, H, sh=oracle.scene_pack_sh(shs), band=scene.bandsIndices)
    assert ((np.ascontiguousarray(fr.rec[:, 7]).view(np.uint32) & BR.SH_BIT) != 0).sum() > 1000
    for form in ("default", "throughput"):
        r, _ = _context(gh, monkeypatch, form, W, H)
        r.render(scene, cam)
        _ran_as(r, form)
        fr.check(r.readPixelsFloat(), ("B sh", form))
        r.dispose()
    cfg = gh.synth.CONFIGS["C1"]
    _, data, pos = scenes("C1")
    cam = gh.orbit_camera(19, width=W, height=H, fx=cfg["fx"])
    fr = Frame(oracle, data, pos, cam, W, H, fade=0.11)
    for form in ("default", "throughput"):
        r, _ = _context(gh, monkeypatch, form, W, H)
        r.set_depth_fade(True, 0.11)
        fr.check(_render(r, fr), ("B fade", form))
        r.dispose()


@pytest.mark.parametrize("sub", ["1", "2"])
def test_more_than_64_segments_lie_inside_the_bound(gh, oracle, scenes, monkeypatch, sub):
    """C3 at a third of its resolution (test_bins_with_more_than_64_segments' frame): bins of several ten thousand entries cut
    into 256-entry segments, the last of 64 taking the rest."""
    cfg = gh.synth.CONFIGS["C3"]
    W, H = 640, 360
    _, data, pos = scenes("C3")
    cam = gh.orbit_camera(17, 120, W, H, cfg["fx"] / 3)
    fr = Frame(oracle, data, pos, cam, W, H, windows=[(W // 2 - 32, H // 2 - 32, 64, 64), (96, 64, 64, 64)])
    env = {"GSR_LONG_ITEMS": "0", "GSR_SEG_LEN": "256", "GSR_SEG_TARGET": "100000", "GSR_BLEND_SUB": sub}
    imgs = {}
    for fuse in ("1", "0"):
        r, _ = _context(gh, monkeypatch, "default", W, H, env=dict(env, GSR_FUSE_COMBINE=fuse))
        imgs[fuse] = _render(r, fr)
        wi = r.work_items()
        assert wi["seg_len"] == 256 and wi["waves_per_tile"] == int(sub) and int(r.bin_totals().max()) > 64 * 256
        fr.check(imgs[fuse], ("B 64+ segments", "sub" + sub, "fused" if fuse == "1" else "separate"))
        r.dispose()
    assert np.array_equal(imgs["1"], imgs["0"])


# C -------------------------------------------------------------------------------------------------------------------
def _oracle_checks(oracle, fr, r, img, what):
    """what _full_size_checks asserts, on the frame of a context that is already rendered"""
    from test_gpu_parity import _check_against_ideal_mode
    assert np.array_equal(r.lastDepthIndex(), fr.order), what
    V, D = oracle.tile_stats(fr.bbox)
    st = r.stats()
    assert st["visible"] == V and st["tile_entries"] == D, what
    exact = oracle.render(fr.order, fr.raw, fr.rec, fr.bbox, fr.W, fr.H, 1)
    err = np.abs(img.astype(np.float64) - exact.astype(np.float64)).max()
    assert err <= TOL_EXACT, (what, err)
    _check_against_ideal_mode(img, oracle.render(fr.order, fr.raw, fr.rec, fr.bbox, fr.W, fr.H, 0))


def test_the_benchmarked_configuration(gh, oracle, scenes, monkeypatch, frames):
    """Three throughput contexts in flight on C3, poses interleaved as bench.py issues them (render_async on all three, then
    sync): k_blend, whole-bin items cut by the per-bin policy, saturation skip on, the assembly walk."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = gh.synth.CONFIGS["C3"]
    W, H = cfg["width"], cfg["height"]
    _, data, pos = scenes("C3")
    ctx = [gh.HIPRenderer(W, H, throughput=True) for _ in range(3)]
    for r in ctx:
        r.set_raw_scene(data, pos)
    rounds = [(21, 84, 21), (84, 21, 84)]
    for poses in rounds:
        for r, k in zip(ctx, poses):
            r.set_camera(gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"]))
            r.render_async()
        for r in ctx:
            r.sync()
        for i, (r, k) in enumerate(zip(ctx, poses)):
            wi = r.work_items()
            assert wi["waves_per_tile"] == 1 and wi["items"] >= wi["bins"], wi
            img = r.readPixelsFloat()
            fr = frames("C3", k)
            fr.check(img, "C three in flight, C3 pose %d" % k)
            assert np.array_equal(r.readPixels().reshape(H, W, 4), BR.to_rgba8(img))
            if i == 0:
                _oracle_checks(oracle, fr, r, img, ("C3", k))
    for r in ctx:
        r.dispose()


def test_the_benchmarked_configuration_at_4k(gh, oracle, scenes, monkeypatch, frames):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = gh.synth.CONFIGS["C4"]
    fr = frames("C4", 50)
    r = gh.HIPRenderer(cfg["width"], cfg["height"], throughput=True)
    img = _render(r, fr)
    assert r.work_items()["waves_per_tile"] == 1
    fr.check(img, "C throughput, C4 pose 50")
    _oracle_checks(oracle, fr, r, img, ("C4", 50))
    r.dispose()


# D -------------------------------------------------------------------------------------------------------------------
def _stack_frame(oracle, kind, length):
    W, H = BR.STACK_FRAME
    cam, splats = BR.stack_scene(kind, length)
    data, pos = make_scene(oracle, splats)
    return Frame(oracle, data, pos, cam, W, H)


STACKS = [("grey", n) for n in BR.STACK_LENGTHS] + [(kind, n) for kind, n in BR.STACK_LENGTH.items()]


@pytest.mark.parametrize("kind,length", STACKS, ids=["%s-%d" % s for s in STACKS])
def test_saturation_and_termination_at_their_edges(gh, oracle, monkeypatch, kind, length):
    """Both kernels: the image with the saturation skip equals the image without it bit for bit, both lie inside the bound, and
    with early termination inside the bound plus eps (instead of the flat 1e-3)."""
    fr = _stack_frame(oracle, kind, length)
    W, H = fr.W, fr.H
    ref = fr.refs[(0, 0, W, H)]
    assert ref["kept"].max() == length
    if kind == "corner":
        assert ref["kept"][32, 32] == 1 and ref["rgba"][32, 32, 0] > 0.5
    for form in ("throughput", "default"):
        imgs = {}
        for sat in ("1", "0"):
            r, _ = _context(gh, monkeypatch, form, W, H, env={"GSR_SATURATE": sat, "GSR_LONG_ITEMS": "1"})
            imgs[sat] = _render(r, fr)
            wi = _ran_as(r, form, {"GSR_LONG_ITEMS": "1"})
            assert wi["items"] == 9 and np.all(r.bin_totals() == length), (wi, r.bin_totals())
            fr.check(imgs[sat], ("D %s %d" % (kind, length), form, "skip" if sat == "1" else "no skip"))
            r.dispose()
        assert np.array_equal(imgs["1"], imgs["0"]), (kind, length, form)
        if kind == "corner":       # the live pixel of an otherwise saturated quadrant shows the splat behind the stack
            assert imgs["1"][32, 32, 0] > 0.5 and imgs["1"][63, 63, 0] > 0.5
        for eps in (1e-2, 1e-4):
            r, _ = _context(gh, monkeypatch, form, W, H, early_out_eps=eps)
            img = _render(r, fr)
            fr.check(img, ("D %s %d" % (kind, length), form, "eps %g" % eps), eps=eps)
            if kind == "corner":   # a tile with one uncovered pixel never stops early: the plain bound
                tile = (slice(32, 48), slice(32, 48))
                assert np.all(np.abs(img[tile].astype(np.float64) - ref["rgba"][tile]) <= ref["bound"][tile])
            r.dispose()


# E -------------------------------------------------------------------------------------------------------------------
def test_work_item_boundaries_and_the_fold(gh, oracle, monkeypatch):
    W, H = BR.ITEM_FRAME
    cam, splats = BR.item_scene()
    data, pos = make_scene(oracle, splats)
    fr = Frame(oracle, data, pos, cam, W, H)
    counts = list(BR.ITEM_COUNTS) + [0] * (24 - len(BR.ITEM_COUNTS))
    for seg_len in ("256", "512"):
        for form in ("sub1", "sub2", "throughput"):
            imgs = {}
            for fuse in ("1", "0"):
                env = {"GSR_LONG_ITEMS": "0", "GSR_SEG_LEN": seg_len, "GSR_SEG_TARGET": "100000", "GSR_FUSE_COMBINE": fuse}
                r, _ = _context(gh, monkeypatch, form, W, H, env=env)
                imgs[fuse] = _render(r, fr)
                wi = _ran_as(r, form, env)
                assert r.bin_totals().reshape(-1).tolist() == counts
                # every bin is cut into ceil(entries / seg_len) segments, at most 64 (the last takes the rest); an empty bin is one item
                want = sum(min(max(-(-c // int(seg_len)), 1), 64) for c in counts)
                assert wi["items"] == want, (wi, want)
                fr.check(imgs[fuse], ("E seg_len " + seg_len, form, "fused" if fuse == "1" else "separate"))
                r.dispose()
            assert np.array_equal(imgs["1"], imgs["0"]), (seg_len, form)
    _forms(gh, monkeypatch, fr, "E", forms=("default", "long", "bounds"))

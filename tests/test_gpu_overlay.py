"""The selection overlay on the GPU (k_overlay.hip, gsr_overlay.cpp) against tests/overlay_reference.py -- the specification in
numpy, fed by the oracle's projection and sort and by the selection as the host holds it, never by device read-backs -- for four
kinds of selection, in every form the frame in front of it runs in, with and without the trimmed walk and the tile skip, on
stacks around the chunk edges, partial bins, a band context, an SH scene, a shared scene, through the delivery ring and on the
bounds-checked twin.  Where the reference says a pixel has no selected fragment the comparison is EXACT (cover 0, overlay = fb
bit for bit); elsewhere cover and (overlay - fb) lie within their derived bounds."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import blend_reference as BR
import overlay_reference as OR
import select_reference as SR
import yuv_reference as YR
from test_oracle_render import make_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
KNOBS = ("GSR_BIN_TWO_LEVEL", "GSR_LONG_ITEMS", "GSR_DEPTH_SKIP", "GSR_OVERLAY_TRIM")
GSR_ERR_ARG, GSR_ERR_OVERFLOW = -1, -5
NAME, POSES = "C1", (3, 40)
W, H = 640, 480
TINT, MIX = (1.0, 0.5, 0.0), 0.5
REGION = (200, 150, 420, 330)
SELECTIONS = ("region", "single", "every second", "all")
STACKS = (1, 255, 256, 257, 512, 513)
RATIOS = {}     # what -> (largest |gpu - ref| / bound of cover, of overlay - fb), printed at the end of the module: DESIGN.md 5.10 quotes it


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    assert gsplat_hip.GSR_ERR_OVERFLOW == GSR_ERR_OVERFLOW
    yield gsplat_hip
    for what in sorted(RATIOS):
        print("\noverlay: max |gpu - ref| / bound  %-34s cover %.3f  overlay - fb %.3f" % ((what,) + RATIOS[what]), end="")


def _cam(gh, k, w=W, h=H):
    cfg = gh.synth.CONFIGS[NAME]
    return gh.orbit_camera(k, width=w, height=h, fx=cfg["fx"] * w / W)


def _view(oracle, cam, data, pos, w, h, **kw):
    v, p, vp = cam.f32()
    rec, bbox, raw = oracle.project(data, v, p, cam.fx, cam.fy, w, h, **kw)
    return rec, bbox, raw, oracle.sort(vp, pos)[0]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what):
    for x, y, name in zip(a, b, ("overlay", "cover")):
        bad = np.argwhere(_bits(x) != _bits(y))
        assert not bad.size, (what, name, len(bad), bad[:4].tolist())


def _same_pass(got, fb, want, what):
    """The pass of another form of the frame: cover bit for bit.  The overlay is one rounding of fb + mix * (tint * S - C), and a
    compositor that cut the frame differently may leave other bits in ITS fb (within its own bound: tests/test_gpu_blend.py): where
    fb is the base's the overlay is the base's bit for bit, and everywhere (overlay - fb) differs from the base's by no more than
    the two roundings, half an ulp of each overlay value -- what is added to fb has the same bits in both."""
    over, cover = got
    wover, wcover, wfb = want
    bad = np.argwhere(_bits(cover) != _bits(wcover))
    assert not bad.size, (what, "cover", len(bad), bad[:4].tolist())
    assert np.array_equal(_bits(over[..., 3]), _bits(fb[..., 3])), (what, "alpha")
    same_fb = (_bits(fb) == _bits(wfb)).all(axis=2)
    assert np.array_equal(_bits(over[same_fb]), _bits(wover[same_fb])), (what, "overlay where fb is the same")
    d = (over.astype(np.float64) - fb.astype(np.float64)) - (wover.astype(np.float64) - wfb.astype(np.float64))
    half = 0.5 * (np.spacing(np.abs(over)).astype(np.float64) + np.spacing(np.abs(wover)).astype(np.float64))
    assert (np.abs(d) <= half).all(), (what, "overlay - fb", float((np.abs(d) / half).max()))
    return float(same_fb.mean())


class C1:
    """the oracle's views of C1 at both poses and, per (pose, selection), the selection and its reference: computed once, shared, never changed"""

    def __init__(self, oracle, scenes, gh):
        self.oracle, self.gh = oracle, gh
        self.rows, self.data, self.pos = scenes(NAME)
        self.n = gh.synth.CONFIGS[NAME]["n"]
        self.views, self.blends, self.refs = {}, {}, {}

    def view(self, k):
        if k not in self.views:
            self.views[k] = _view(self.oracle, _cam(self.gh, k), self.data, self.pos, W, H)
        return self.views[k]

    def blend(self, k):
        if k not in self.blends:
            self.blends[k] = BR.blend_reference(*self.view(k), W, H)
        return self.blends[k]

    def selection(self, k, kind):
        rec, bbox, raw, order = self.view(k)
        if kind == "region":
            return SR.centre_pick(rec, bbox, REGION)
        if kind == "single":            # the splat with the largest pixel box among the nearest 400 of the order
            vis = [i for i in order[:400] if bbox[i, 0] <= bbox[i, 2] and bbox[i, 1] <= bbox[i, 3]]
            best = max(vis, key=lambda i: (min(bbox[i, 2], W - 1) - max(bbox[i, 0], 0)) * (min(bbox[i, 3], H - 1) - max(bbox[i, 1], 0)))
            sel = np.zeros(self.n, bool)
            sel[best] = True
            return sel
        if kind == "every second":
            return np.arange(self.n) % 2 == 0
        return np.ones(self.n, bool)

    def ref(self, k, kind):
        if (k, kind) not in self.refs:
            sel = self.selection(k, kind)
            ref = OR.overlay_reference(*self.view(k), sel, W, H)
            for a in ref.values():
                a.flags.writeable = False
            self.refs[(k, kind)] = (sel, ref)
        return self.refs[(k, kind)]


@pytest.fixture(scope="module")
def c1(oracle, scenes, gh):
    return C1(oracle, scenes, gh)


def _context(gh, monkeypatch, scenes, env=None, name=NAME, seed=None, w=W, h=H, overlay=(TINT, MIX), **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    r = gh.HIPRenderer(w, h, **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)
    if name is not None:
        r.set_scene_rows(scenes(name, seed)[0])
    if overlay:
        r.set_overlay(*overlay)
    return r


def _frame(gh, r, k):
    r.set_camera(_cam(gh, k, r.width, r.height))
    r.render_async()
    r.sync()
    assert r.stats()["overflow_frames"] == 0


def _inside(got, fb, ref, what, tint=TINT, mix=MIX):
    """where the reference has no selected fragment: cover exactly 0 and overlay = fb bit for bit; the pixels with cover > 0 are
    the reference's; elsewhere cover and overlay - fb within their bounds; alpha is fb's everywhere"""
    rgba, cover = got
    assert rgba.dtype == np.float32 and cover.dtype == np.float32, what
    none = ~ref["maybe"]
    assert not cover[none].any() and np.array_equal(_bits(rgba[none]), _bits(fb[none])), (what, "pixels without a selected fragment")
    assert np.array_equal(_bits(rgba[..., 3]), _bits(fb[..., 3])), (what, "alpha")
    lit = cover > 0
    assert not (lit & none).any() and not (ref["surely"] & ~lit).any(), (what, "covered pixels differ", int((lit != ref["maybe"]).sum()))
    ratios = OR.excess(cover, rgba, fb, ref, tint, mix)
    print("overlay", what, "max |gpu - ref| / bound: cover %.3f overlay - fb %.3f" % ratios)
    RATIOS[what if isinstance(what, str) else " ".join(str(x) for x in what)] = ratios
    assert ratios[0] <= 1.0 and ratios[1] <= 1.0, (what, ratios)
    return lit


@pytest.fixture(scope="module")
def base(gh, scenes, c1):
    """what a default context gives for every second splat at both poses: the images every other form must reproduce bit for bit"""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        r = _context(gh, mp, scenes)
        r.set_selection(c1.selection(POSES[0], "every second"))
        for k in POSES:
            _frame(gh, r, k)
            out[k] = r.read_overlay() + (r.readPixelsFloat(),)
        r.dispose()
    for v in out.values():
        for a in v:
            a.flags.writeable = False
    return out


# 1 exact ---------------------------------------------------------------------------------------------------------------
def test_empty_selection_and_mix_zero_are_the_frame(gh, monkeypatch, scenes, c1):
    r = _context(gh, monkeypatch, scenes)
    bytes0 = r.scene_sharing()[1]
    _frame(gh, r, POSES[0])
    fb = r.readPixelsFloat()
    rgba, cover = r.read_overlay()                                  # a scene never selected in: no mask is allocated
    assert r.scene_sharing()[1] == bytes0
    assert not cover.any() and np.array_equal(_bits(rgba), _bits(fb)) and fb[..., 3].max() > 0.5
    r.set_selection(None)                                           # the empty selection, with a mask
    rgba, cover = r.read_overlay()
    assert not cover.any() and np.array_equal(_bits(rgba), _bits(fb))
    r.set_selection(c1.selection(POSES[0], "every second"))
    r.set_overlay(TINT, 0.0)
    rgba, cover = r.read_overlay()
    assert np.array_equal(_bits(rgba), _bits(fb)) and (cover > 0).sum() > 1000
    r.set_overlay(TINT, MIX)
    rgba2, cover2 = r.read_overlay()                                # the options changed: the pass ran again
    assert np.array_equal(_bits(cover2), _bits(cover)) and not np.array_equal(_bits(rgba2), _bits(fb))
    assert np.array_equal(r.read_overlay_rgba8(), BR.to_rgba8(rgba2))
    assert np.array_equal(_bits(r.readPixelsFloat()), _bits(fb))   # the pass reads the framebuffer and never writes it
    r.dispose()


# 2 bounded -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SELECTIONS)
@pytest.mark.parametrize("k", POSES)
def test_c1_lies_inside_the_specification(gh, monkeypatch, scenes, c1, k, kind):
    sel, ref = c1.ref(k, kind)
    assert np.array_equal(ref["surely"], ref["maybe"])              # no pixel of C1 where T * B underflows: the covered set is exact
    r = _context(gh, monkeypatch, scenes)
    _frame(gh, r, k)
    if kind == "region":
        assert r.select_region(REGION) == int(sel.sum()) and np.array_equal(r.selection(), sel) and 50 < sel.sum() < c1.n
    else:
        assert r.set_selection(sel) == int(sel.sum())
    fb = r.readPixelsFloat()
    got = r.read_overlay()
    lit = _inside(got, fb, ref, "C1 pose %d %s" % (k, kind))
    assert np.array_equal(lit, ref["maybe"]) and lit.any() and (kind == "all" or not lit.all())
    if kind == "all":                                               # S is the alpha of the frame: within the sum of both bounds
        blend = c1.blend(k)
        assert np.array_equal(ref["maybe"], blend["kept"] > 0)
        d = np.abs(got[1].astype(np.float64) - fb[..., 3].astype(np.float64))
        assert (d <= ref["S_bound"] + blend["bound"][..., 3]).all(), float((d / (ref["S_bound"] + blend["bound"][..., 3])).max())
    r.dispose()


# 3 forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["no trim", "no tile skip", "neither", "throughput", "two level", "short items", "long items"])
def test_every_form_gives_the_same_bits(gh, monkeypatch, scenes, c1, base, form):
    env = {"no trim": {"GSR_OVERLAY_TRIM": "0"}, "no tile skip": {"GSR_DEPTH_SKIP": "0"}, "neither": {"GSR_OVERLAY_TRIM": "0", "GSR_DEPTH_SKIP": "0"},
           "two level": {"GSR_BIN_TWO_LEVEL": "1"}, "short items": {"GSR_LONG_ITEMS": "0"}, "long items": {"GSR_LONG_ITEMS": "1"}}.get(form)
    r = _context(gh, monkeypatch, scenes, env=env, throughput=form == "throughput")
    r.set_selection(c1.selection(POSES[0], "every second"))
    for k in POSES:
        _frame(gh, r, k)
        share = _same_pass(r.read_overlay(), r.readPixelsFloat(), base[k], (form, k))
        print("overlay", form, "pose", k, "pixels whose fb has the base's bits: %.4f" % share)
    # a small selection near the front: the trimmed walk ends early in every list, the untrimmed one does not
    few = np.zeros(c1.n, bool)
    few[c1.view(POSES[1])[3][:40]] = True
    r.set_selection(few)
    got = r.read_overlay()
    plain = _context(gh, monkeypatch, scenes)
    plain.set_selection(few)
    _frame(gh, plain, POSES[1])
    _same_pass(got, r.readPixelsFloat(), plain.read_overlay() + (plain.readPixelsFloat(),), (form, "the 40 nearest"))
    assert got[1].any()
    plain.dispose(); r.dispose()


# 4 end to end ----------------------------------------------------------------------------------------------------------
def test_a_scene_recoloured_on_the_host_is_the_overlay(gh, oracle, monkeypatch, scenes, c1):
    k = POSES[0]
    tint_bytes = (255, 128, 0)
    tint = tuple(float(np.float32(b) * (np.float32(1.0) / np.float32(255.0))) for b in tint_bytes)
    sel, _ = c1.ref(k, "every second")
    ref = OR.overlay_reference(*c1.view(k), sel, W, H)
    rows2 = np.array(c1.rows, copy=True).reshape(-1, 32)
    rows2[sel, 24:27] = np.asarray(tint_bytes, np.uint8)
    data2, pos2 = oracle.scene_pack(rows2.reshape(c1.rows.shape))
    blend2 = BR.blend_reference(*_view(oracle, _cam(gh, k), data2, pos2, W, H), W, H)
    r = _context(gh, monkeypatch, scenes, overlay=(tint, 1.0))
    r.set_selection(sel)
    _frame(gh, r, k)
    fb1 = r.readPixelsFloat()
    over, cover = r.read_overlay()
    r2 = _context(gh, monkeypatch, scenes, name=None, overlay=None)
    r2.set_scene_rows(rows2.reshape(c1.rows.shape))
    _frame(gh, r2, k)
    fb2 = r2.readPixelsFloat()
    # overlay = fb1 + delta; fb1 within the first scene's bound of its reference, delta within its own, fb2 within the second scene's
    bound = c1.blend(k)["bound"][..., :3] + OR.delta_bound(ref, tint, 1.0, fb1) + blend2["bound"][..., :3]
    d = np.abs(over[..., :3].astype(np.float64) - fb2[..., :3].astype(np.float64))
    print("overlay end to end: max |overlay - recoloured frame| / bound %.3f, largest difference %.3g" % (float((d / bound).max()), float(d.max())))
    assert (d <= bound).all(), float((d / bound).max())
    assert np.abs(fb1[..., :3].astype(np.float64) - fb2[..., :3]).max() > 0.2          # (the two frames really differ)
    r.dispose(); r2.dispose()


# 5 boundaries ----------------------------------------------------------------------------------------------------------
STACK_REFS = {}


def _stack_scene(oracle, length):
    """`length` faint co-located splats over the whole 96 x 96 frame (every bin's list holds exactly `length` entries; T is still
    0.13 behind 513 of them), the oracle's view, and per selected position the reference"""
    if length not in STACK_REFS:
        Ws, Hs = BR.STACK_FRAME
        cam, to_world = BR.front_view(Ws, Hs)
        splats = BR.stack(to_world, 48.0, 48.0, length, 100.0, (90, 160, 220, 1))
        data, pos = make_scene(oracle, splats)
        view = _view(oracle, cam, data, pos, Ws, Hs)
        assert view[3].tolist() == list(range(length))
        refs = {}
        for at in sorted({0, 255, 256, length - 1}):
            if at < length:
                refs[at] = OR.overlay_reference(*view, np.arange(length) == at, Ws, Hs)
                assert refs[at]["maybe"].all() and refs[at]["surely"].all()
        STACK_REFS[length] = (cam, data, pos, refs)
    return STACK_REFS[length]


@pytest.mark.parametrize("length", STACKS)
def test_stacks_around_the_chunk_edges(gh, oracle, monkeypatch, length):
    Ws, Hs = BR.STACK_FRAME
    cam, data, pos, refs = _stack_scene(oracle, length)
    for trim in ("1", "0"):
        r = _context(gh, monkeypatch, None, env={"GSR_OVERLAY_TRIM": trim}, name=None, w=Ws, h=Hs)
        r.set_raw_scene(data, pos)
        r.set_camera(cam)
        r.render_async()
        r.sync()
        assert r.stats()["bin_entries"] == 9 * length
        fb = r.readPixelsFloat()
        for at, ref in refs.items():
            r.set_selection(np.arange(length) == at)
            got = r.read_overlay()
            lit = _inside(got, fb, ref, ("stack", length, "selected", at, "trim", trim))
            assert lit.all()
            # the selected splat alone: S = T_before * B, and T_before = (1 - B) ^ at up to the bound
            assert got[1].max() <= 1.0 / 255.0 * 1.001 and got[1].min() > 0.0
        r.dispose()


def test_an_odd_size_has_partial_bins(gh, oracle, monkeypatch, scenes):
    w, h = 333, 207                  # 11 x 7 bins, the last column 13 pixels wide, the last row 15 high
    n = 1025
    r = _context(gh, monkeypatch, scenes, name=n, seed=7, w=w, h=h)
    _, data, pos = scenes(n, 7)
    sel = np.arange(n) % 3 == 0
    r.set_selection(sel)
    for k in POSES:
        _frame(gh, r, k)
        ref = OR.overlay_reference(*_view(oracle, _cam(gh, k, w, h), data, pos, w, h), sel, w, h)
        got = r.read_overlay()
        assert got[0].shape == (h, w, 4) and got[1].shape == (h, w)
        lit = _inside(got, r.readPixelsFloat(), ref, ("333x207 pose", k))
        assert lit[:, 320:].any() and lit[192:, :].any()
    r.dispose()


def test_a_band_context_leaves_the_other_columns_alone(gh, monkeypatch, scenes, c1, base):
    k = POSES[0]
    band = (192, 448)
    r = _context(gh, monkeypatch, scenes, band=band)
    r.set_selection(c1.selection(k, "every second"))
    _frame(gh, r, k)
    fb = r.readPixelsFloat()
    rgba, cover = r.read_overlay()
    out = np.ones(W, bool)
    out[band[0]:band[1]] = False
    assert not cover[:, out].any() and np.array_equal(_bits(rgba[:, out]), _bits(fb[:, out]))
    # inside the band the lists hold what the frame's hold for those bins: the same bits as the whole frame's overlay
    assert np.array_equal(_bits(cover[:, ~out]), _bits(base[k][1][:, ~out])) and np.array_equal(_bits(rgba[:, ~out]), _bits(base[k][0][:, ~out]))
    assert cover[:, ~out].any()
    r.dispose()


def test_an_sh_scene_takes_its_colours_from_shcol(gh, oracle, monkeypatch, scenes):
    n = 20000
    rows, data, pos = scenes(n, 41)
    rng = np.random.default_rng(8)
    b0, b1, b2 = 4999, 9999, 14999            # splats 0..4999 plain, then degree 1, 2, 3
    shs = (rng.standard_normal((n - (b0 + 1), 48)) * 0.35).astype(np.float32)
    scene = gh.Scene()
    scene.bandsIndices = np.array([b0, b1, b2], dtype=np.int32)
    scene.setData(rows, shs)
    cam = gh.orbit_camera(33, width=W, height=H)
    view = _view(oracle, cam, data, pos, W, H, sh=oracle.scene_pack_sh(shs), band=scene.bandsIndices)
    assert ((np.ascontiguousarray(view[0][:, 7]).view(np.uint32) & BR.SH_BIT) != 0).sum() > 1000
    sel = np.arange(n) % 2 == 1
    ref = OR.overlay_reference(*view, sel, W, H)
    r = _context(gh, monkeypatch, scenes, name=None)
    r.render(scene, cam)
    assert r.stats()["overflow_frames"] == 0
    r.set_selection(sel)
    got = r.read_overlay()
    _inside(got, r.readPixelsFloat(), ref, "SH scene")
    # (with byte colours in place of shcol the selected sums would be far outside: the SH colours leave [0, 1])
    assert np.abs(ref["C"]).max() > 0.05
    r.dispose()


# 6 state ---------------------------------------------------------------------------------------------------------------
def _refused(gh, call, match, code=GSR_ERR_ARG):
    with pytest.raises(gh.GsplatError, match=match) as ei:
        call()
    assert ei.value.code == code


def test_options_and_frame_rules(gh, monkeypatch, scenes, c1):
    r = _context(gh, monkeypatch, scenes, overlay=None)
    assert not r._L.gsr_overlay_device_ptr(r._ctx, 0) and not r._L.gsr_overlay_device_ptr(r._ctx, 1)
    _frame(gh, r, POSES[0])
    _refused(gh, r.overlay_async, "no overlay options")
    _refused(gh, r.read_overlay, "no overlay options")
    _refused(gh, r.read_overlay_rgba8, "no overlay options")
    for bad in (((float("nan"), 0.0, 0.0), 0.5), ((0.0, float("inf"), 0.0), 0.5), (TINT, -0.01), (TINT, 1.01), (TINT, float("nan"))):
        _refused(gh, lambda: r.set_overlay(*bad), "gsr_set_overlay")
    opt = gh.GsrOverlayOptions((ctypes.c_float * 3)(*TINT), MIX, (ctypes.c_int32 * 4)(0, 0, 1, 0))
    assert r._L.gsr_set_overlay(r._ctx, ctypes.byref(opt)) == GSR_ERR_ARG
    _refused(gh, r.overlay_async, "no overlay options")            # nothing changed
    r.set_overlay(TINT, MIX)
    assert r._L.gsr_overlay_device_ptr(r._ctx, 0) and r._L.gsr_overlay_device_ptr(r._ctx, 1) and not r._L.gsr_overlay_device_ptr(r._ctx, 2)
    r.overlay_async()
    sel = c1.selection(POSES[0], "every second")
    r.set_selection(sel)
    first = r.read_overlay()
    assert r._L.gsr_read_overlay(r._ctx, None, None) == 0           # either output may be NULL
    r.sort()
    _refused(gh, r.overlay_async, "sort-only")
    _frame(gh, r, POSES[0])
    _same(r.read_overlay(), first, "the same pose again")
    # stale after an edit of the scene, an erase and a resize: what gsr_depth_async needs of the frame is gone
    r.scene_translate((0.5, 0.0, 0.0))
    _refused(gh, r.read_overlay, "no frame")
    _refused(gh, r.overlay_async, "no frame")
    r.scene_translate((-0.5, 0.0, 0.0))
    _frame(gh, r, POSES[0])
    r.read_overlay()
    few = np.zeros(c1.n, bool)
    few[:100] = True
    r.set_selection(few)
    assert r.scene_erase_selected() == c1.n - 100
    _refused(gh, r.read_overlay, "no frame")
    _frame(gh, r, POSES[0])
    rgba, cover = r.read_overlay()                                  # the erase left the empty selection
    assert not cover.any() and np.array_equal(_bits(rgba), _bits(r.readPixelsFloat()))
    r.setSize(800, 600)
    _refused(gh, r.read_overlay, "no frame")
    r.set_selection(np.arange(c1.n - 100) % 2 == 0)
    _frame(gh, r, POSES[0])
    rgba, cover = r.read_overlay()                                  # (the images grew with the size)
    assert rgba.shape == (600, 800, 4) and cover.any() and np.array_equal(_bits(rgba[..., 3]), _bits(r.readPixelsFloat()[..., 3]))
    r.set_overlay(None)                                             # off: the buffers go
    assert not r._L.gsr_overlay_device_ptr(r._ctx, 0)
    _refused(gh, r.read_overlay, "no overlay options")
    r.dispose()


def test_nothing_else_moves(gh, monkeypatch, scenes, c1):
    plain = _context(gh, monkeypatch, scenes, overlay=None)
    r = _context(gh, monkeypatch, scenes)
    sel = c1.selection(POSES[0], "every second")
    for c in (plain, r):
        c.set_selection(sel)
        _frame(gh, c, POSES[0])
    pts = [(320, 240), (100, 100), (317, 243)]
    state = lambda c: (c.readPixelsFloat(), c.lastDepthIndex(), c.work_items(), c.read_depth(), c.pick(pts), c.selection())

    def same(x, y, what):
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1]) and x[2] == y[2], what
        assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(x[3], y[3])) and np.array_equal(x[4], y[4]) and np.array_equal(x[5], y[5]), what

    before = state(r)
    for k, call in enumerate((r.overlay_async, r.read_overlay, r.read_overlay_rgba8, lambda: r.set_overlay((0.0, 1.0, 0.0), 1.0), r.read_overlay)):
        call()
        same(state(r), before, k)
    same(state(r), state(plain), "a context that never ran it")
    for c in (plain, r):
        _frame(gh, c, POSES[1])
    r.overlay_async()
    same(state(r), state(plain), "the next frame")
    assert r.scene_sharing() == plain.scene_sharing()               # the images are the context's, not the scene's
    plain.dispose(); r.dispose()


def test_shared_scene_selection_changes(gh, monkeypatch, scenes, c1, base):
    k = POSES[0]
    a = _context(gh, monkeypatch, scenes)
    b = gh.HIPRenderer(W, H)
    b.share_scene(a)
    b.set_overlay(TINT, MIX)
    sel = c1.selection(k, "every second")
    a.set_selection(sel)
    a.open_delivery(2)
    a.delivery_set_overlay()
    a.set_camera(_cam(gh, k))
    a.render_async()
    serial = a.deliver()                                            # the pass is enqueued on a's stream, nothing waited for
    other = ~sel
    assert b.set_selection(other) == int(other.sum())               # through the OTHER member: waits for a's pass first
    s, px = a.acquire(serial)
    assert np.array_equal(px, BR.to_rgba8(base[k][0]))              # the pass already enqueued never saw the change
    a.release(s)
    a.sync()
    got = a.read_overlay()                                          # a's next overlay shows it, with no new frame
    assert not np.array_equal(_bits(got[1]), _bits(base[k][1]))
    _frame(gh, b, k)
    _same(b.read_overlay(), got, "the other member, the same selection")
    a.set_selection(sel)                                            # and back, through a: b's image is stale too
    _same(b.read_overlay(), base[k][:2], "the first selection again")
    a.close_delivery()
    a.dispose(); b.dispose()


def test_an_overflowed_frame_is_refused(gh, monkeypatch, scenes, c1, base):
    r = _context(gh, monkeypatch, scenes)
    r.set_selection(c1.selection(POSES[0], "every second"))
    _frame(gh, r, POSES[0])
    r.read_overlay()                                                # an image of an earlier frame is on the device
    assert r.stats()["bin_entries"] > 4096
    r.open_delivery(2)
    r.delivery_set_overlay()
    r.set_list_capacity(1024)                                       # far too small for the next frame
    r.set_camera(_cam(gh, POSES[1]))
    r.render_async()
    r.overlay_async()                                               # behind a frame that does not fit: walks nothing, writes nothing
    k = r.deliver()
    _refused(gh, lambda: r.acquire(k), "frame %d was not composited" % k, GSR_ERR_OVERFLOW)
    got = r.read_overlay()                                          # the frame is rendered again with regrown lists, the pass redone
    assert r.stats()["overflow_frames"] == 1
    _same(got, base[POSES[1]][:2], "the repaired frame")
    r.dispose()


# 7 delivery ------------------------------------------------------------------------------------------------------------
def _deliver_one(r):
    r.render_async()
    k = r.deliver()
    s, px = r.acquire(k)
    out = tuple(np.array(p) for p in px) if isinstance(px, tuple) else np.array(px)
    r.release(s)
    return out


@pytest.mark.parametrize("fmt", ["rgba8", "nv12"])
def test_delivery_with_and_without_the_overlay(gh, monkeypatch, scenes, c1, base, fmt):
    k = POSES[0]
    r = _context(gh, monkeypatch, scenes)
    r.set_selection(c1.selection(k, "every second"))
    r.set_camera(_cam(gh, k))
    r.open_delivery(2, format=fmt)                                  # off: the default
    plain = _deliver_one(r)
    fb8 = BR.to_rgba8(base[k][2])
    over8 = BR.to_rgba8(base[k][0])
    assert not np.array_equal(fb8, over8)
    flat = lambda px: np.concatenate([p.ravel() for p in px]) if isinstance(px, tuple) else px
    want = (lambda img8: img8) if fmt == "rgba8" else (lambda img8: YR.payload(img8, "nv12"))
    assert np.array_equal(flat(plain), want(fb8))
    r.delivery_set_overlay(True)
    assert np.array_equal(flat(_deliver_one(r)), want(over8))
    assert np.array_equal(flat(_deliver_one(r)), want(over8))       # (a second frame through the one overlay image)
    r.setSize(320, 240)                                             # resize keeps the ring and the switch
    r.set_camera(_cam(gh, k, 320, 240))
    small = _deliver_one(r)
    assert np.array_equal(flat(small), want(BR.to_rgba8(r.read_overlay()[0]))) and not np.array_equal(flat(small), want(BR.to_rgba8(r.readPixelsFloat())))
    r.delivery_set_overlay(False)
    assert np.array_equal(flat(_deliver_one(r)), want(BR.to_rgba8(r.readPixelsFloat())))
    r.close_delivery()
    _refused(gh, lambda: r.delivery_set_overlay(True), "no delivery ring")
    r.open_delivery(2, format=fmt)                                  # a new ring starts with the switch off
    assert np.array_equal(flat(_deliver_one(r)), want(BR.to_rgba8(r.readPixelsFloat())))
    r.set_overlay(None)
    _refused(gh, lambda: r.delivery_set_overlay(True), "no overlay options")
    r.dispose()


def test_a_depth_rings_plane_is_still_the_frames(gh, monkeypatch, scenes, c1, base):
    k = POSES[0]
    r = _context(gh, monkeypatch, scenes)
    r.set_selection(c1.selection(k, "every second"))
    r.set_camera(_cam(gh, k))
    r.open_delivery_depth(2, depth="f32", depth_step=1)
    r.delivery_set_overlay(True)
    r.render_async()
    s, px, depth = r.acquire(r.deliver())
    assert np.array_equal(px, BR.to_rgba8(base[k][0])) and np.array_equal(_bits(np.array(depth)), _bits(r.read_depth()[1]))
    r.release(s)
    r.dispose()


def test_in_a_group_the_switch_is_refused(gh, monkeypatch, scenes):
    from gsplat_hip import bands
    r = _context(gh, monkeypatch, scenes)

    def allgather(send, recv, nbytes, stream):                      # never called: no frame is gathered here
        raise AssertionError

    r.open_delivery(2)
    r.delivery_set_overlay(True)
    r.join_group_custom(0, 1, bands.band_edges(W, 1), allgather)    # joined AFTER the switch: the delivery is refused
    r.set_camera(_cam(gh, POSES[0]))
    r.render_async()
    _refused(gh, r.deliver, "RGBA8 of other ranks")
    r.delivery_set_overlay(False)
    _refused(gh, lambda: r.delivery_set_overlay(True), "RGBA8 of other ranks")
    r.leave_group()
    r.delivery_set_overlay(True)
    r.render_async()
    s, px = r.acquire(r.deliver())
    r.release(s)
    r.dispose()


# 8 the bounds twin -----------------------------------------------------------------------------------------------------
def _digest(arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def test_bounds_twin_in_a_child_process(gh, base):
    """the bounds-checked build over C1, an odd size and a band: no site counts anything, and C1's bits are the shipped build's"""
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    code = ("import sys, ctypes, hashlib, numpy as np; sys.path[:0] = %r; import gsplat_hip as gh\n"
            "cfg = gh.synth.CONFIGS[%r]; n = cfg['n']\n"
            "def run(r, cam, sel):\n"
            "    r.set_overlay(%r, %r); r.set_camera(cam); r.render_async(); r.sync(); r.set_selection(sel); return r.read_overlay()\n"
            "def counters(r, what):\n"
            "    for name in ('gsr_debug_bounds_overlay', 'gsr_debug_bounds_depth', 'gsr_debug_bounds_select'):\n"
            "        buf = (ctypes.c_uint32 * 8)(); assert getattr(r._L, name)(buf) == 0; print('bounds', what, name, list(buf)); assert not any(buf), (what, name, list(buf))\n"
            "r = gh.HIPRenderer(%d, %d); r.set_scene_rows(gh.synth.config_rows(%r))\n"
            "for k in %r:\n"
            "    a = run(r, gh.orbit_camera(k, width=%d, height=%d, fx=cfg['fx']), np.arange(n) %% 2 == 0)\n"
            "    print('digest', k, hashlib.sha256(a[0].tobytes() + a[1].tobytes()).hexdigest())\n"
            "few = np.zeros(n, bool); few[:3] = True; run(r, gh.orbit_camera(3, width=%d, height=%d, fx=cfg['fx']), few); counters(r, 'C1'); r.dispose()\n"
            "r = gh.HIPRenderer(333, 207); r.set_scene_rows(gh.synth.synth_rows(1025, 7)); run(r, gh.orbit_camera(3, width=333, height=207), np.arange(1025) %% 3 == 0); counters(r, 'odd'); r.dispose()\n"
            "r = gh.HIPRenderer(%d, %d, band=(192, 448)); r.set_scene_rows(gh.synth.config_rows(%r)); run(r, gh.orbit_camera(3, width=%d, height=%d, fx=cfg['fx']), np.arange(n) %% 2 == 0); counters(r, 'band'); r.dispose()\n"
            "print('done')\n"
            % ([p for p in sys.path if p], NAME, TINT, MIX, W, H, NAME, POSES, W, H, W, H, W, H, NAME, W, H))
    env = dict(os.environ, GSPLAT_HIP_LIB=BOUNDS_LIB)
    for k in KNOBS:
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "done" in out.stdout, out.stdout[-3000:]
    for k in POSES:
        assert "digest %d %s" % (k, _digest(base[k][:2])) in out.stdout, out.stdout[-1500:]


def test_bounds_twin_on_the_stacks(gh, oracle, monkeypatch):
    """the stacks need the oracle's scene packing, so they run on the twin in this process, as tests/test_gpu_contrib.py runs its own"""
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    Ws, Hs = BR.STACK_FRAME
    for length in STACKS:
        cam, data, pos, refs = _stack_scene(oracle, length)
        r = _context(gh, monkeypatch, None, name=None, w=Ws, h=Hs, lib_path=BOUNDS_LIB)
        r.set_raw_scene(data, pos)
        r.set_camera(cam)
        r.render_async()
        r.sync()
        fb = r.readPixelsFloat()
        for at, ref in refs.items():
            r.set_selection(np.arange(length) == at)
            _inside(r.read_overlay(), fb, ref, ("bounds stack", length, at))
        for name in ("gsr_debug_bounds_overlay", "gsr_debug_bounds_depth", "gsr_debug_bounds_select"):
            buf = (ctypes.c_uint32 * 8)()
            assert getattr(r._L, name)(buf) == 0
            assert not any(buf), (length, name, list(buf))
        r.dispose()

"""The selection outline on the GPU (k_outline_bits / k_outline_apply of k_overlay.hip, gsr_set_overlay_outline) against
tests/outline_reference.py.  cover on the device is within a bound of the oracle, not bit-equal to it, so the outline is tested
against the device's OWN planes, which makes every comparison exact: render and set the overlay, read (ov, cover) with the outline
off, set the outline, read again; cover must be bit-identical and the image must equal apply(ov, outline_mask(cover, ...), ...) bit
for bit.  rgb lies outside [0, 1], so a missed or an extra pixel cannot hide; the threshold is the median of the device's non-zero
cover values, so at least one pixel sits exactly on the tie.

Before it compares, a case asserts conditions on its INPUT (they hold with margin on the oracle's cover: the smallest count below
is 4 pixels, the fractions run from 1.5 % to 48 %): the expected mask has edge pixels in columns x % 64 == 0 and == 63, in the odd
size's partial last word, in row 0, row H - 1, column 0 and column W - 1 (of the domain), and covers between 0.1 % and 50 % of the
domain.  An outer outline of width 16 around "every second" splat cannot meet the last one -- inside is speckled over the whole
frame, so nearly every pixel that is not inside is within 16 of one that is -- so the odd size and the band, whose selections are
this test's to choose, take that one case on a sparse selection (every 32nd splat: 26 % by the oracle; the region: 22 %), as C1
takes it on its region selection (9 %); the border conditions ride on the dense selection, the fraction on the sparse one.  On C1
the issue prescribes "every second", the median threshold and width 16 outer together, and they give 55 %: FORCED names that one
case, which is compared exactly like the rest and exempted from the fraction alone."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import blend_reference as BR
import outline_reference as OL
import outline_twin
import yuv_reference as YR
from test_gpu_overlay import BOUNDS_LIB, KNOBS, MIX, NAME, POSES, REGION, TINT, H, W, _bits, _cam, _context, _deliver_one, _frame, _refused

pytestmark = pytest.mark.gpu

GSR_ERR_ARG, GSR_ERR_OVERFLOW = -1, -5
RGB = (0.125, 7.0, -3.0)
WIDTHS, SIDES, ALPHAS = (1, 2, 3, 16), ("outer", "inner"), (1.0, 0.4)
FORCED = {("every second", "outer", 16)}      # the issue's own contradiction (the module's text); every other case meets every condition
WIDE = ("outer", 16)
POSE = POSES[0]


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _select(r, n, kind):
    if kind == "region":
        assert 50 < r.select_region(REGION) < n
    elif kind == "every 32nd":
        assert r.set_selection(np.arange(n) % 32 == 0) == (n + 31) // 32
    else:
        assert r.set_selection(np.arange(n) % 2 == 0) == (n + 1) // 2


def _hip_copy(dst, src, nbytes, kind):
    """hipMemcpy of the HIP runtime this process already holds (kind 1: host to device)"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths[0])
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(dst, src, nbytes, kind) == 0


def _median(cover, dom=None):
    """the median of the plane's non-zero values (of the domain): an element of the plane, so a pixel sits on the tie"""
    nz = np.sort(cover[(cover > 0) & (True if dom is None else dom)])
    assert nz.size > 100
    return float(nz[nz.size // 2])


def _conditions(mask, what, dom=None, borders=True, last_word=False):
    h, w = mask.shape
    xs = np.arange(w)
    x0, x1 = (0, w) if dom is None else (int(np.flatnonzero(dom[0]).min()), int(np.flatnonzero(dom[0]).max()) + 1)
    frac = mask.sum() / float(h * (x1 - x0))
    print("outline", what, "edge pixels %d (%.2f %% of the domain)" % (mask.sum(), 100 * frac))
    assert mask[:, xs % 64 == 0].any() and mask[:, xs % 64 == 63].any(), (what, "word edges")
    if borders:
        assert mask[0].any() and mask[-1].any() and mask[:, x0].any() and mask[:, x1 - 1].any(), (what, "borders")
    if last_word:
        assert w % 64 and mask[:, (w // 64) * 64:].any(), (what, "the partial last word")
    if what not in FORCED:
        assert 0.001 <= frac <= 0.5, (what, frac)


def _exact(r, ov, cover, thr, width, side, alpha, what, dom=None, masks=None):
    """set the outline, read again: cover bit-identical, the image the specification's bit for bit; the mask"""
    key = (width, side)
    if masks is None or key not in masks:
        m = OL.outline_mask(cover, thr, width, OL.OUTER if side == "outer" else OL.INNER, dom)
        if masks is not None:
            masks[key] = m
    else:
        m = masks[key]
    r.set_overlay_outline(RGB, alpha, thr, width, side)
    got, cover2 = r.read_overlay()
    assert np.array_equal(_bits(cover2), _bits(cover)), (what, "cover changed")
    want = OL.apply(ov, m, RGB, alpha)
    bad = np.argwhere((_bits(got) != _bits(want)).any(axis=2))
    assert not bad.size, (what, width, side, alpha, len(bad), bad[:4].tolist(), "edge pixels expected", int(m.sum()))
    changed = (_bits(got) != _bits(ov)).any(axis=2)
    assert not (changed & ~m).any(), (what, "a pixel outside the mask was written")
    return m


def _sweep(r, what, dom=None, borders=True, last_word=False, alphas=ALPHAS, only=None, skip=None):
    """every (side, width) -- `only` that one, or all but `skip` -- at the median threshold: exact, and the input's conditions"""
    r.set_overlay_outline(None)
    ov, cover = r.read_overlay()
    thr = _median(cover, dom)
    assert (cover == np.float32(thr)).any()
    for side in SIDES:
        for width in WIDTHS:
            if (only and (side, width) != only) or (side, width) == skip:
                continue
            masks = {}
            for alpha in alphas:
                m = _exact(r, ov, cover, thr, width, side, alpha, what, dom, masks)
            _conditions(m, (what, side, width), dom, borders, last_word)
    return ov, cover, thr


# 1 the specification ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["every second", "region"])
def test_c1_is_the_specification_bit_for_bit(gh, monkeypatch, scenes, kind):
    r = _context(gh, monkeypatch, scenes)
    _frame(gh, r, POSE)
    _select(r, gh.synth.CONFIGS[NAME]["n"], kind)
    # (the region's splats do not reach the image's border: the border conditions are "every second"'s)
    _sweep(r, kind, borders=kind == "every second")
    r.dispose()


def test_an_odd_size_has_a_partial_last_word(gh, monkeypatch, scenes):
    w, h, n = 333, 207, 1025            # 6 words a row, the last 13 pixels wide; 11 x 7 bins
    r = _context(gh, monkeypatch, scenes, name=n, seed=7, w=w, h=h)
    _frame(gh, r, POSE)
    _select(r, n, "every second")
    _sweep(r, "odd", last_word=True, alphas=(0.4,), skip=WIDE)
    _select(r, n, "every 32nd")                                     # the wide outer outline on a sparse selection (the module's text)
    _sweep(r, "odd sparse", borders=False, last_word=True, alphas=(0.4,), only=WIDE)
    r.dispose()


def test_a_band_context_draws_inside_its_columns_only(gh, monkeypatch, scenes):
    band = (192, 448)
    r = _context(gh, monkeypatch, scenes, band=band)
    _frame(gh, r, POSE)
    _select(r, gh.synth.CONFIGS[NAME]["n"], "every second")
    dom = OL.band_domain(W, H, band)
    ov, cover, thr = _sweep(r, "band", dom=dom, alphas=(0.4,), skip=WIDE)
    assert not cover[~dom].any()
    # pixels outside the domain are not neighbours: as "not inside" pixels they would draw an inner edge along the band's sides
    with_dom, without = OL.outline_mask(cover, thr, 3, OL.INNER, dom), OL.outline_mask(cover, thr, 3, OL.INNER)
    assert (without & ~with_dom)[:, band[0]:band[0] + 3].any() and (without & ~with_dom)[:, band[1] - 3:band[1]].any()
    # and nothing outside the band's columns is written, whatever the side (what _exact compared, said once more on its own)
    fb = r.readPixelsFloat()
    for side in SIDES:
        r.set_overlay_outline(RGB, 1.0, thr, 16, side)
        got, _ = r.read_overlay()
        assert np.array_equal(_bits(got[~dom]), _bits(fb[~dom])), side
    _select(r, gh.synth.CONFIGS[NAME]["n"], "region")               # the wide outer outline on the region (the module's text)
    _sweep(r, "band region", dom=dom, borders=False, alphas=(0.4,), only=WIDE)
    r.dispose()


# 2 state ---------------------------------------------------------------------------------------------------------------
def test_state_rules(gh, monkeypatch, scenes):
    n = gh.synth.CONFIGS[NAME]["n"]
    r = _context(gh, monkeypatch, scenes)
    _frame(gh, r, POSE)
    fb = r.readPixelsFloat()
    r.set_overlay_outline(RGB, 0.4, 0.25, 2, "outer")
    got, cover = r.read_overlay()                                   # a scene never selected in: nothing is launched, the frame
    assert not cover.any() and np.array_equal(_bits(got), _bits(fb))
    r.set_selection(None)                                           # the empty selection, with a mask: ov bit for bit, either side
    for side in SIDES:
        r.set_overlay_outline(RGB, 0.4, 0.25, 2, side)
        got, cover = r.read_overlay()
        assert not cover.any() and np.array_equal(_bits(got), _bits(fb)), side
    _select(r, n, "every second")
    r.set_overlay_outline(None)
    ov, cover = r.read_overlay()                                    # the parent's overlay
    a = _exact(r, ov, cover, 0.25, 2, "outer", 0.4, "state")
    assert a.any()
    r.set_overlay_outline(None)                                     # off after on: the parent's bits again
    got, cover2 = r.read_overlay()
    assert np.array_equal(_bits(got), _bits(ov)) and np.array_equal(_bits(cover2), _bits(cover))
    # changed outline options re-run the pass (each read is the specification for the options of the moment) ...
    b = _exact(r, ov, cover, 0.25, 3, "outer", 0.4, "state")
    c = _exact(r, ov, cover, 0.25, 3, "inner", 0.4, "state")
    d = _exact(r, ov, cover, 0.5, 3, "inner", 0.4, "state")
    assert (b & ~a).any() and not (b & c).any() and (c != d).any()
    _exact(r, ov, cover, 0.5, 3, "inner", 1.0, "state")
    # equal options do not make the image stale: a mark written into the device image survives them (no pass ran), and goes with
    # the next changed option (the pass rewrites every pixel)
    mark = np.array([-5.0, 6.0, -7.0, 8.0], np.float32)
    r.sync()
    _hip_copy(r._L.gsr_overlay_device_ptr(r._ctx, 0), mark.ctypes.data, mark.nbytes, 1)
    r.set_overlay_outline(RGB, 1.0, 0.5, 3, "inner")
    r.set_overlay(TINT, MIX)                                        # (the overlay's own equal options likewise)
    got, _ = r.read_overlay()
    assert np.array_equal(got[0, 0], mark), "equal options re-ran the pass"
    assert np.array_equal(r.read_overlay_rgba8()[0, 0], BR.to_rgba8(mark[None, None])[0, 0])
    r.set_overlay_outline(RGB, 0.5, 0.5, 3, "inner")
    _exact(r, ov, cover, 0.5, 3, "inner", 1.0, "state")             # changed (twice): the pass ran, the mark is gone
    # ... and so do a changed selection and a new frame
    _select(r, n, "region")
    r.set_overlay_outline(None)
    ov2, cover2 = r.read_overlay()
    assert not np.array_equal(_bits(cover2), _bits(cover))
    _exact(r, ov2, cover2, 0.5, 3, "inner", 1.0, "another selection")
    _frame(gh, r, POSES[1])
    got, cover3 = r.read_overlay()                                  # the outline is still set: the new frame's image carries it
    r.set_overlay_outline(None)
    ov3, cover3b = r.read_overlay()
    assert np.array_equal(_bits(cover3), _bits(cover3b)) and not np.array_equal(_bits(cover3), _bits(cover2))
    m3 = OL.outline_mask(cover3, 0.5, 3, OL.INNER)
    assert m3.any() and np.array_equal(_bits(got), _bits(OL.apply(ov3, m3, RGB, 1.0)))
    # changed overlay options keep the outline
    r.set_overlay_outline(RGB, 1.0, 0.5, 3, "inner")
    r.set_overlay((0.0, 1.0, 0.0), 1.0)
    got, _ = r.read_overlay()
    r.set_overlay_outline(None)
    ov4, _ = r.read_overlay()
    assert not np.array_equal(_bits(ov4), _bits(ov3)) and np.array_equal(_bits(got), _bits(OL.apply(ov4, m3, RGB, 1.0)))
    # gsr_set_overlay(NULL) clears the outline too
    r.set_overlay_outline(RGB, 1.0, 0.5, 3, "inner")
    r.set_overlay(None)
    r.set_overlay((0.0, 1.0, 0.0), 1.0)
    got, _ = r.read_overlay()
    assert np.array_equal(_bits(got), _bits(ov4))
    r.dispose()


def test_every_refusal_changes_nothing(gh, monkeypatch, scenes):
    n = gh.synth.CONFIGS[NAME]["n"]
    r = _context(gh, monkeypatch, scenes, overlay=None)
    _frame(gh, r, POSE)
    _refused(gh, lambda: r.set_overlay_outline(RGB, 0.4, 0.25, 2, "outer"), "no overlay options")
    r.set_overlay_outline(None)                                     # off is always accepted
    r.set_overlay(TINT, MIX)
    _select(r, n, "every second")
    ov, cover = r.read_overlay()
    _exact(r, ov, cover, 0.25, 2, "outer", 0.4, "refusals")
    want = r.read_overlay()[0]
    nan, inf = float("nan"), float("inf")
    for bad, match in ((((nan, 0.0, 0.0), 0.4, 0.25, 2, "outer"), "rgb"), (((0.0, inf, 0.0), 0.4, 0.25, 2, "outer"), "rgb"),
                       (((0.0, 0.0, -inf), 0.4, 0.25, 2, "outer"), "rgb"),
                       ((RGB, -0.01, 0.25, 2, "outer"), "alpha"), ((RGB, 1.01, 0.25, 2, "outer"), "alpha"), ((RGB, nan, 0.25, 2, "outer"), "alpha"),
                       ((RGB, 0.4, 0.0, 2, "outer"), "threshold"), ((RGB, 0.4, -0.5, 2, "outer"), "threshold"), ((RGB, 0.4, nan, 2, "outer"), "threshold"),
                       ((RGB, 0.4, inf, 2, "outer"), "threshold"),
                       ((RGB, 0.4, 0.25, 0, "outer"), "width"), ((RGB, 0.4, 0.25, 17, "outer"), "width"), ((RGB, 0.4, 0.25, -1, "outer"), "width")):
        _refused(gh, lambda: r.set_overlay_outline(*bad), "gsr_set_overlay_outline: " + match)
        assert np.array_equal(_bits(r.read_overlay()[0]), _bits(want)), bad
    for side, reserved in ((2, (0,) * 5), (-1, (0,) * 5), (0, (0, 0, 0, 0, 1)), (0, (1, 0, 0, 0, 0))):
        opt = gh.GsrOutlineOptions((ctypes.c_float * 3)(*RGB), 0.4, 0.25, 2, side, (ctypes.c_int32 * 5)(*reserved))
        assert r._L.gsr_set_overlay_outline(r._ctx, ctypes.byref(opt)) == GSR_ERR_ARG
        assert np.array_equal(_bits(r.read_overlay()[0]), _bits(want)), (side, reserved)
    with pytest.raises(ValueError):
        r.set_overlay_outline(RGB, 0.4, 0.25, 2, "both")
    r.dispose()


def test_an_overflowed_frame_is_still_refused(gh, monkeypatch, scenes):
    n = gh.synth.CONFIGS[NAME]["n"]
    r = _context(gh, monkeypatch, scenes)
    _select(r, n, "every second")
    r.set_overlay_outline(RGB, 0.4, 0.25, 2, "outer")
    _frame(gh, r, POSES[0])
    before = r.read_overlay()                                       # an outlined image of an earlier frame is on the device
    assert r.stats()["bin_entries"] > 4096
    r.open_delivery(2)
    r.delivery_set_overlay()
    r.set_list_capacity(1024)                                       # far too small for the next frame
    r.set_camera(_cam(gh, POSES[1]))
    r.render_async()
    r.overlay_async()                                               # behind a frame that does not fit: nothing walked, nothing drawn
    k = r.deliver()
    _refused(gh, lambda: r.acquire(k), "frame %d was not composited" % k, GSR_ERR_OVERFLOW)
    got, cover = r.read_overlay()                                   # the frame is rendered again with regrown lists, the pass redone
    assert r.stats()["overflow_frames"] == 1
    r.set_overlay_outline(None)
    ov, cover2 = r.read_overlay()
    assert np.array_equal(_bits(cover), _bits(cover2)) and not np.array_equal(_bits(cover), _bits(before[1]))
    m = OL.outline_mask(cover, 0.25, 2, OL.OUTER)
    assert m.any() and np.array_equal(_bits(got), _bits(OL.apply(ov, m, RGB, 0.4)))
    r.dispose()


def test_nothing_else_moves(gh, monkeypatch, scenes):
    n = gh.synth.CONFIGS[NAME]["n"]
    r = _context(gh, monkeypatch, scenes)
    _select(r, n, "every second")
    _frame(gh, r, POSE)
    state = lambda: (r.readPixelsFloat(),) + tuple(r.read_depth()) + (r.read_overlay()[1], r.selection())
    before = state()
    for side in SIDES:
        r.set_overlay_outline(RGB, 0.4, 0.25, 16, side)
        r.read_overlay()
        r.read_overlay_rgba8()
        for x, y in zip(state(), before):
            assert np.array_equal(_bits(x), _bits(y)), side
    r.dispose()


# 3 delivery ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgba8", "nv12"])
def test_a_ring_delivers_the_outlined_image(gh, monkeypatch, scenes, fmt):
    n = gh.synth.CONFIGS[NAME]["n"]
    r = _context(gh, monkeypatch, scenes)
    _select(r, n, "every second")
    _frame(gh, r, POSE)
    ov, cover = r.read_overlay()
    m = OL.outline_mask(cover, 0.25, 2, OL.OUTER)
    want_off, want_on = BR.to_rgba8(ov), BR.to_rgba8(OL.apply(ov, m, RGB, 0.4))
    assert not np.array_equal(want_off, want_on)
    flat = lambda px: np.concatenate([p.ravel() for p in px]) if isinstance(px, tuple) else px
    conv = (lambda img8: img8) if fmt == "rgba8" else (lambda img8: YR.payload(img8, "nv12"))
    r.open_delivery(2, format=fmt)
    r.delivery_set_overlay(True)
    off = flat(_deliver_one(r))
    r.set_overlay_outline(RGB, 0.4, 0.25, 2, "outer")
    on = flat(_deliver_one(r))
    # each frame is its converted reference, so the two differ exactly where the converted references differ
    assert np.array_equal(off, conv(want_off)) and np.array_equal(on, conv(want_on))
    assert np.array_equal(off != on, conv(want_off) != conv(want_on)) and (off != on).any()
    if fmt == "rgba8":
        assert np.array_equal(on, r.read_overlay_rgba8())            # exactly read_overlay_rgba8()'s bytes of the outlined image
    r.set_overlay_outline(None)
    assert np.array_equal(flat(_deliver_one(r)), off)
    r.dispose()


def test_in_a_group_the_refusal_stands(gh, monkeypatch, scenes):
    from gsplat_hip import bands
    r = _context(gh, monkeypatch, scenes)
    r.set_overlay_outline(RGB, 0.4, 0.25, 2, "outer")

    def allgather(send, recv, nbytes, stream):                      # never called: no frame is gathered here
        raise AssertionError

    r.open_delivery(2)
    r.delivery_set_overlay(True)
    r.join_group_custom(0, 1, bands.band_edges(W, 1), allgather)
    r.set_camera(_cam(gh, POSE))
    r.render_async()
    _refused(gh, r.deliver, "RGBA8 of other ranks")
    r.delivery_set_overlay(False)
    _refused(gh, lambda: r.delivery_set_overlay(True), "RGBA8 of other ranks")
    r.leave_group()
    r.dispose()


# 4 shared scenes -------------------------------------------------------------------------------------------------------
def test_members_of_a_shared_scene_have_their_own_outline(gh, monkeypatch, scenes):
    n = gh.synth.CONFIGS[NAME]["n"]
    a = _context(gh, monkeypatch, scenes)
    b = gh.HIPRenderer(W, H)
    b.share_scene(a)
    b.set_overlay(TINT, MIX)
    _select(a, n, "every second")                                   # the selection is the scene's: both see it
    for c in (a, b):
        _frame(gh, c, POSE)
    ov, cover = a.read_overlay()
    ovb, coverb = b.read_overlay()
    assert np.array_equal(_bits(cover), _bits(coverb))
    a.set_overlay_outline(RGB, 0.4, 0.25, 2, "outer")
    b.set_overlay_outline((1.0, 1.0, 1.0), 1.0, 0.5, 5, "inner")
    ma, mb = OL.outline_mask(cover, 0.25, 2, OL.OUTER), OL.outline_mask(cover, 0.5, 5, OL.INNER)
    for _ in range(2):                                              # (in turn, twice: neither sees the other's options)
        assert np.array_equal(_bits(a.read_overlay()[0]), _bits(OL.apply(ov, ma, RGB, 0.4)))
        assert np.array_equal(_bits(b.read_overlay()[0]), _bits(OL.apply(ovb, mb, (1.0, 1.0, 1.0), 1.0)))
    a.set_overlay_outline(None)
    assert np.array_equal(_bits(a.read_overlay()[0]), _bits(ov))
    assert np.array_equal(_bits(b.read_overlay()[0]), _bits(OL.apply(ovb, mb, (1.0, 1.0, 1.0), 1.0)))
    a.dispose(); b.dispose()


# 5 the bounds twin -----------------------------------------------------------------------------------------------------
def test_bounds_twin_in_a_child_process(gh):
    """the bounds-checked build over C1, the odd size and the band (tests/outline_twin.py): no site counts anything, and the bits
    are the shipped build's"""
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    code = "import sys; sys.path[:0] = %r; import outline_twin; outline_twin.main()" % ([p for p in sys.path if p],)
    env = dict(os.environ, GSPLAT_HIP_LIB=BOUNDS_LIB)
    for k in KNOBS:
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "done" in out.stdout, out.stdout[-3000:]
    assert out.stdout.count("gsr_debug_bounds_overlay") == 3
    for name, d in outline_twin.digests(gh).items():
        assert "digest %s %s" % (name, d) in out.stdout, (name, out.stdout[-1500:])

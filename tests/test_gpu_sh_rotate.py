"""Rotating SH coefficients on the GPU ("Rotating SH coefficients"): gsr_scene_rotate_sh bit for bit against
the specification (tests/sh_rotate_reference.py) over every scope, the projection reading what was written, the coefficient form
against the frame form within the derived bound, a selection turned with its coefficients, a frame baked, a shared scene, and
the bounds-checked twin.

300 splats: more than one 256-lane workgroup and five waves; bandsIndices[0] in (-1, 36, 63, 64, 298) puts SH row 0 on lane 0 of a
wave, in mid-wave, on a wave's last lane, on the next wave's first, and leaves a single SH row.  Frames are 64 x 64."""
import ctypes
import os

import numpy as np
import pytest

import history_trace as ht
import sh_follow_reference as sf
import sh_rotate_reference as ref

pytestmark = pytest.mark.gpu

N, W, H = 300, 64, 64
FIRSTS = (-1, 36, 63, 64, 298)
QUAT = (0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214)
QUAT2 = (-0.5, 0.5, 0.5, 0.5)
QUAT3 = (0.6, 0.0, -1.6, 0.4)          # not a unit quaternion: the coefficients use q / |q|
PIVOT = (0.25, -0.5, 0.125)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _band(first):
    """bandsIndices with the first threshold at `first` and the others at the thirds of what is left"""
    left = N - 1 - first
    return np.array([first, first + left // 3, first + 2 * left // 3], dtype=np.int32)


@pytest.fixture(scope="module")
def material(gh):
    """(rows, finite textures, textures with special values, camera), built once: N rows each, a scene takes the first sh_count"""
    rows = np.array(gh.synth.synth_rows(N, 23), dtype=np.uint8).reshape(N, 32)
    rng = np.random.default_rng(29)
    finite, special = [], []
    for ch in range(3):
        c = (rng.standard_normal((N, 16)) * 0.35).astype(np.float16).view(np.uint16)
        finite.append(ref.words(c))
        s = c.copy()
        s[0, 2 + ch] = 0x7c00                      # +inf: row 0, band 1
        s[1, 5 + ch] = 0xfc00                      # -inf: band 2
        s[2, 10 + ch] = 0x7e01 + ch                # a NaN with a payload: band 3
        s[3, :] = 0x8000                           # -0 everywhere, the DC half included
        s[4, 1:] = rng.integers(1, 0x0400, 15).astype(np.uint16)          # subnormals
        s[5, 9:] = 0x7bff                          # the largest half: sums overflow to infinity
        s[N - 1, :] = s[0, :]                      # (a scene of one SH row takes row 0; the last row of the longest scene has them too)
        s[70, 0] = 0x7e55                          # a NaN in a DC half keeps its bits
        special.append(ref.words(s))
    cam = gh.orbit_camera(33, width=W, height=H, fx=40.0)      # (wide: most of the scene is in a 64 x 64 frame)
    return rows.reshape(-1), finite, special, cam


def _textures(material, first, special=False):
    count = N - (first + 1)
    return [t[:8 * count].copy() for t in material[2 if special else 1]]


def _context(gh, material, first, follow=False, special=False, lib_path=None):
    r = gh.HIPRenderer(W, H, lib_path=lib_path)
    r.set_scene_rows(material[0])
    r.set_sh(_textures(material, first, special), _band(first))
    r.set_sh_follow(follow)
    return r


def _frame(r, cam):
    r.set_camera(cam)
    r.render_async()
    r.sync()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_textures(r, tex, band):
    got, got_band = r.read_scene_sh()
    assert list(got_band) == list(band)
    for ch, (a, b) in enumerate(zip(got, tex)):
        assert a.size == b.size and np.array_equal(a, b), "channel %d: %d rows differ" % (ch, (a.reshape(-1, 8) != b.reshape(-1, 8)).any(axis=1).sum())


def _m32(gh, q):
    return ref.m32(gh.sh_rotation(q))


def _scopes(first):
    """name -> the bool mask over the splats (None: GSR_SH_ALL)"""
    rng = np.random.default_rng(100 + first)
    idx = np.arange(N)
    return [("all", None), ("nothing", np.zeros(N, dtype=bool)), ("everything", np.ones(N, dtype=bool)), ("30 %", rng.random(N) < 0.3),
            ("straddling", (idx >= first - 9) & (idx <= first + 12)), ("without SH rows", idx <= first)]


# ---- 1: every scope, bit for bit ----
def _every_scope(gh, material, first, lib_path=None):
    band = _band(first)
    tex = _textures(material, first, special=True)
    r = _context(gh, material, first, special=True, lib_path=lib_path)
    try:
        before = r.read_scene()
        assert r.scene_rotate_sh(QUAT, selected=True) == 0          # never selected in: no buffers, nothing launched
        _same_textures(r, tex, band)
        for k, (name, mask) in enumerate(_scopes(first)):
            q = (QUAT, QUAT2, QUAT3)[k % 3]
            if mask is not None:
                r.set_selection(mask)
            want = ref.apply(tex, band, mask, _m32(gh, q))
            rows = r.scene_rotate_sh(q, selected=mask is not None)
            assert rows == ref.rows_in_scope(N, band, mask), name
            _same_textures(r, want, band)
            for a, b in zip(want, tex):                              # (the specification itself: DC halves and rows out of scope stay)
                ha, hb = ref.halves(a), ref.halves(b)
                assert np.array_equal(ha[:, 0], hb[:, 0])
                out = np.ones(ha.shape[0], dtype=bool) if mask is None else mask[first + 1:]
                assert np.array_equal(ha[~out], hb[~out])
            tex = want
            if mask is not None:
                assert np.array_equal(r.selection(), mask), name       # the selection is untouched
        # a chain of three rotations follows the specification bit for bit
        for q in (QUAT, QUAT2, QUAT3):
            assert r.scene_rotate_sh(q) == N - (first + 1)
            tex = ref.apply(tex, band, None, _m32(gh, q))
        _same_textures(r, tex, band)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, r.read_scene()))      # the geometry is nobody's business here
        assert np.array_equal(r.sh_frame()[0], sf.IDENTITY) and r.sh_frame()[1] is False
    finally:
        r.dispose()


@pytest.mark.parametrize("first", FIRSTS)
def test_every_scope_is_the_specification(gh, material, first):
    _every_scope(gh, material, first)


def test_argument_rules(gh, material):
    band = _band(36)
    tex = _textures(material, 36)
    r = _context(gh, material, 36)
    try:
        rows = ctypes.c_uint32(7)
        q = np.array(QUAT, dtype=np.float64)
        for bad in ((0.0, 0.0, 0.0, 0.0), (float("nan"), 0.0, 0.0, 1.0), (0.0, float("inf"), 0.0, 1.0)):
            with pytest.raises(gh.GsplatError) as e:
                r.scene_rotate_sh(bad)
            assert e.value.code == ht.GSR_ERR_ARG and "finite and not zero" in str(e.value)
            with pytest.raises(gh.GsplatError) as e:
                r.scene_rotate_selected_sh(bad)
            assert e.value.code == ht.GSR_ERR_ARG
        assert r._L.gsr_scene_rotate_sh(r._ctx, q.ctypes.data, 2, ctypes.byref(rows)) == ht.GSR_ERR_ARG and rows.value == 7
        assert r._L.gsr_scene_rotate_sh(r._ctx, None, 0, ctypes.byref(rows)) == ht.GSR_ERR_ARG
        _same_textures(r, tex, band)
        assert r._L.gsr_scene_rotate_sh(r._ctx, q.ctypes.data, 0, None) == 0          # rows may be NULL
        _same_textures(r, ref.apply(tex, band, None, _m32(gh, QUAT)), band)
        # no SH state: GSR_OK, no rows
        r._check(r._L.gsr_set_scene_sh(r._ctx, None, None, None, 0, None))
        assert r.scene_rotate_sh(QUAT) == 0 and r.scene_rotate_sh(QUAT, selected=True) == 0
        assert np.array_equal(r.scene_bake_sh_frame(), [0.0, 0.0, 0.0, 1.0])
    finally:
        r.dispose()


# ---- 2: the projection reads what was written ----
def _visible(oracle, r, cam, tex, band, least):
    data, pos, _, _ = r.read_scene()
    v, p, vp = cam.f32()
    _, _, oraw = oracle.project(data, v, p, cam.fx, cam.fy, W, H, sh=tex, band=band)
    vis = (oraw[:, 11] == 1.0) & (np.arange(N) > band[0])
    assert vis.sum() >= least, vis.sum()
    return vis, pos, v


def test_the_next_frame_evaluates_the_rotated_coefficients(gh, oracle, material):
    cam = material[3]
    band = _band(36)
    tex = _textures(material, 36)
    r = _context(gh, material, 36)
    try:
        _frame(r, cam)
        vis, pos, v = _visible(oracle, r, cam, tex, band, 100)
        plain = sf.colours(oracle, tex, band, pos, v, None, only=vis)
        assert np.array_equal(_bits(r.read_sh_colors()[vis, :3]), _bits(plain[vis]))
        r.scene_rotate_sh(QUAT)
        with pytest.raises(gh.GsplatError):                         # an edit: the last frame's colours are stale
            r.read_sh_colors()
        turned = ref.apply(tex, band, None, _m32(gh, QUAT))
        _frame(r, cam)
        want = sf.colours(oracle, turned, band, pos, v, None, only=vis)
        assert np.array_equal(_bits(r.read_sh_colors()[vis, :3]), _bits(want[vis]))
        assert np.abs(want[vis] - plain[vis]).max() > 0.05
    finally:
        r.dispose()


# ---- 3: the frame form against the coefficient form ----
def test_coefficient_form_is_within_the_bound_of_the_frame_form(gh, oracle, material):
    cam = material[3]
    band = _band(36)
    tex = _textures(material, 36)
    a, b = _context(gh, material, 36, follow=True), _context(gh, material, 36, follow=False)
    try:
        _frame(b, cam)
        plain = b.read_sh_colors()[:, :3].astype(np.float64)
        a.scene_rotate(QUAT)
        b.scene_rotate(QUAT)
        assert b.scene_rotate_sh(QUAT) == N - 37
        assert np.array_equal(b.sh_frame()[0], sf.IDENTITY) and not np.array_equal(a.sh_frame()[0], sf.IDENTITY)
        _frame(a, cam)
        _frame(b, cam)
        vis, pos, v = _visible(oracle, b, cam, tex, band, 100)
        ca, cb = a.read_sh_colors()[:, :3].astype(np.float64), b.read_sh_colors()[:, :3].astype(np.float64)
        bound = ref.colour_bound(tex, band, QUAT, pos, v)
        assert bound[vis].max() < 4e-3
        print("frame form - coefficient form: max %.3g, bound there %.3g" % (np.abs(ca - cb)[vis].max(), bound[vis].max()))
        assert (np.abs(ca - cb)[vis] <= bound[vis]).all()
        # follow off alone leaves the highlights where they were: the rotation of the coefficients is what moved them
        stale = sf.colours(oracle, tex, band, pos, v, None, only=vis).astype(np.float64)
        assert np.abs(cb[vis] - stale[vis]).max() > 0.05
        assert plain.shape == cb.shape
    finally:
        a.dispose()
        b.dispose()


# ---- 4: rotating a selection ----
def _rotate_a_selection(gh, material, first, lib_path=None):
    band = _band(first)
    tex = _textures(material, first, special=True)
    mask = np.random.default_rng(7).random(N) < 0.4
    mask[first:first + 3] = True
    for follow, pivot, q in ((True, PIVOT, QUAT), (False, None, QUAT3)):
        r = _context(gh, material, first, follow=follow, special=True, lib_path=lib_path)
        twin = _context(gh, material, first, follow=False, special=True, lib_path=lib_path)
        try:
            r.set_selection(mask)
            twin.set_selection(mask)
            r.scene_rotate_selected_sh(q, pivot)
            twin.scene_rotate_selected(q, pivot)
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(r.read_scene(), twin.read_scene()))
            _same_textures(twin, tex, band)
            _same_textures(r, ref.apply(tex, band, mask, _m32(gh, q)), band)
            assert np.array_equal(r.selection(), mask)
            assert np.array_equal(r.sh_frame()[0], sf.IDENTITY) and r.sh_frame()[1] is follow
        finally:
            r.dispose()
            twin.dispose()


@pytest.mark.parametrize("first", (36, 64))
def test_a_selection_turns_with_its_coefficients(gh, material, first):
    _rotate_a_selection(gh, material, first)


def test_a_selection_is_refused_while_the_frame_is_not_the_identity(gh, material):
    band = _band(36)
    tex = _textures(material, 36)
    r = _context(gh, material, 36, follow=True)
    plain = gh.HIPRenderer(W, H)
    try:
        r.set_selection(np.arange(N) % 3 == 0)
        r.scene_rotate(QUAT)
        before = r.read_scene()
        frame = r.sh_frame()[0]
        with pytest.raises(gh.GsplatError) as e:
            r.scene_rotate_selected_sh(QUAT2, PIVOT)
        assert e.value.code == ht.GSR_ERR_ARG and "gsr_scene_bake_sh_frame" in str(e.value)
        with pytest.raises(gh.GsplatError) as e:                    # (the call without SH keeps its own refusal)
            r.scene_rotate_selected(QUAT2, PIVOT)
        assert e.value.code == ht.GSR_ERR_ARG and "SH frame is one per scene" in str(e.value)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, r.read_scene()))
        _same_textures(r, tex, band)
        assert np.array_equal(r.sh_frame()[0], frame)
        # baked, it goes through
        r.scene_bake_sh_frame()
        r.scene_rotate_selected_sh(QUAT2, PIVOT)
        # without SH rows it is gsr_scene_rotate_selected
        plain.set_scene_rows(material[0])
        plain.set_selection(np.arange(N) % 3 == 0)
        plain.scene_rotate(QUAT)
        plain.scene_rotate_selected_sh(QUAT2, PIVOT)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(r.read_scene(), plain.read_scene()))
    finally:
        r.dispose()
        plain.dispose()


# ---- 5: baking a frame ----
def test_bake_moves_the_frame_into_the_coefficients(gh, oracle, material):
    cam = material[3]
    band = _band(36)
    tex = _textures(material, 36)
    r = _context(gh, material, 36, follow=True)
    try:
        r.scene_rotate(QUAT)
        r.scene_rotate(QUAT2)
        frame = r.sh_frame()[0]
        assert np.array_equal(frame, sf.frame_rotate(sf.frame_rotate(sf.IDENTITY, QUAT), QUAT2))
        _frame(r, cam)
        vis, pos, v = _visible(oracle, r, cam, tex, band, 100)
        before = r.read_sh_colors()[:, :3].astype(np.float64)
        geometry = r.read_scene()
        q = r.scene_bake_sh_frame()
        assert np.array_equal(q, ref.bake(frame))
        assert np.array_equal(r.sh_frame()[0], sf.IDENTITY) and r.sh_frame()[1] is True
        baked = ref.apply(tex, band, None, _m32(gh, q))
        _same_textures(r, baked, band)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(geometry, r.read_scene()))
        _frame(r, cam)
        after = r.read_sh_colors()[:, :3].astype(np.float64)
        bound = ref.colour_bound(tex, band, q, pos, v)
        print("before the bake - after it: max %.3g, bound there %.3g" % (np.abs(before - after)[vis].max(), bound[vis].max()))
        assert (np.abs(before - after)[vis] <= bound[vis]).all()
        # an identity frame: nothing launched, and no edit -- the frame's colours can still be read
        assert np.array_equal(r.scene_bake_sh_frame(), [0.0, 0.0, 0.0, 1.0])
        _same_textures(r, baked, band)
        assert np.array_equal(_bits(r.read_sh_colors()[:, :3]), _bits(after.astype(np.float32)))
        # a uniform scale on top of a rotation is baked; a non-uniform one is refused with nothing changed
        r.scene_rotate(QUAT)
        r.scene_scale((2.0, 2.0, 2.0))
        q2 = r.scene_bake_sh_frame()
        assert np.array_equal(q2, ref.bake(sf.frame_scale(sf.frame_rotate(sf.IDENTITY, QUAT), (2.0, 2.0, 2.0))))
        baked = ref.apply(baked, band, None, _m32(gh, q2))
        _same_textures(r, baked, band)
        r.scene_scale((1.0, 1.0, 1.25))
        frame = r.sh_frame()[0]
        geometry = r.read_scene()
        with pytest.raises(gh.GsplatError) as e:
            r.scene_bake_sh_frame()
        assert e.value.code == ht.GSR_ERR_ARG and "uniform scale" in str(e.value)
        assert np.array_equal(r.sh_frame()[0], frame)
        _same_textures(r, baked, band)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(geometry, r.read_scene()))
    finally:
        r.dispose()


# ---- 6: a shared scene ----
def test_an_edit_through_one_member_shows_in_the_other(gh, oracle, material):
    cam = material[3]
    band = _band(36)
    tex = _textures(material, 36)
    a = _context(gh, material, 36)
    b = gh.HIPRenderer(W, H)
    try:
        b.share_scene(a)
        _frame(a, cam)
        _frame(b, cam)
        vis, pos, v = _visible(oracle, a, cam, tex, band, 100)
        a.set_selection(np.arange(N) % 2 == 0)
        assert b.scene_rotate_sh(QUAT, selected=True) == ref.rows_in_scope(N, band, np.arange(N) % 2 == 0)      # through the other member
        turned = ref.apply(tex, band, np.arange(N) % 2 == 0, _m32(gh, QUAT))
        _same_textures(a, turned, band)
        _same_textures(b, turned, band)
        for m in (a, b):
            with pytest.raises(gh.GsplatError):                     # every member's frame is marked as edited
                m.read_sh_colors()
        _frame(a, cam)
        _frame(b, cam)
        want = sf.colours(oracle, turned, band, pos, v, None, only=vis)
        for m in (a, b):
            assert np.array_equal(_bits(m.read_sh_colors()[vis, :3]), _bits(want[vis]))
        assert a.scene_sharing()[0] == 2
    finally:
        b.dispose()
        a.dispose()


# ---- 7: the bounds twin ----
def test_bounds_twin_counts_nothing(gh, material):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    for first in FIRSTS:
        _every_scope(gh, material, first, lib_path=BOUNDS_LIB)
    for first in (36, 64):
        _rotate_a_selection(gh, material, first, lib_path=BOUNDS_LIB)
    for unit in (L.gsr_debug_bounds_sh_rotate, L.gsr_debug_bounds_edit):
        buf = (ctypes.c_uint32 * 8)()
        assert unit(buf) == 0
        assert list(buf) == [0] * 8

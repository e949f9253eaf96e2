"""Rotating SH coefficients, the specification against mathematics (tests/sh_rotate_reference.py; no GPU): the band matrices are
orthogonal, compose as rotations do and have the defining property; the identity is exact; the f32 rotation of the halves keeps what
it must keep; a rotation and its inverse stay within the derived bound; the coefficient form of a rotated scene stays within
colour_bound of the frame form.

The matrices' bound is 2^-40 (9e-13): entries are at most 1 and each takes under 200 f64 operations, about 2^-45, with a factor of
32 for the solve."""
import numpy as np
import pytest

import sh_follow_reference as sf
import sh_rotate_reference as ref

TOL = 2.0 ** -40
IDENTITY_Q = (0.0, 0.0, 0.0, 1.0)


def _quaternions(seed, count, unit=True):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((count, 4))
    if unit:
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    else:
        q *= np.exp(rng.uniform(-3.0, 3.0, (count, 1)))
    return q


def _half_rows(seed, rows, scale=0.35):
    """u16[rows, 16]: finite halves of coefficients around `scale`"""
    c = np.random.default_rng(seed).standard_normal((rows, 16)) * scale
    return c.astype(np.float16).view(np.uint16)


def test_the_matrices_are_orthogonal():
    for q in _quaternions(1, 200, unit=False):
        for D in ref.matrices(q):
            assert np.abs(D @ D.T - np.eye(D.shape[0])).max() <= TOL
            assert np.linalg.det(D) > 0.0


def test_the_matrices_compose():
    qs = _quaternions(2, 200)
    for a, b in zip(qs[0::2], qs[1::2]):
        for Dab, Da, Db in zip(ref.matrices(ref.multiply(a, b)), ref.matrices(a), ref.matrices(b)):
            assert np.abs(Dab - Da @ Db).max() <= TOL


def test_the_defining_property():
    """sum (D c)_k B_k(R d) = sum c_k B_k(d) for every c: B(R d)^T D = B(d)^T at random unit d"""
    rng = np.random.default_rng(3)
    for q in _quaternions(4, 100):
        d = rng.standard_normal((50, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        R = sf.rotation_matrix(ref.unit(q))
        before, after = ref.basis(d), ref.basis(d @ R.T)
        for (j0, w), D in zip(ref.BANDS, ref.matrices(q)):
            assert np.abs(after[:, j0 - 1:j0 - 1 + w] @ D - before[:, j0 - 1:j0 - 1 + w]).max() <= TOL


def test_band_one_is_the_rotation_in_the_basis_order():
    """B_1..3 = C1 (-y, -z, x): D_1 = P R P^T for the signed permutation P that takes (x, y, z) to (-y, -z, x)"""
    P = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    for q in _quaternions(5, 50):
        assert np.abs(ref.matrices(q)[0] - P @ sf.rotation_matrix(ref.unit(q)) @ P.T).max() <= TOL


def test_the_identity_is_exact_and_a_bad_quaternion_has_no_unit():
    for q in (IDENTITY_Q, (0.0, 0.0, 0.0, -3.5), (0.0, 0.0, 0.0, 1e-150)):
        for D in ref.matrices(q):
            assert np.array_equal(D, np.eye(D.shape[0]))
    for q in ((0.0, 0.0, 0.0, 0.0), (np.nan, 0.0, 0.0, 1.0), (np.inf, 0.0, 0.0, 1.0), (1e-200, 0.0, 0.0, 0.0), (1e200, 0.0, 0.0, 1.0)):      # (a length that underflows to 0 or overflows is none)
        assert ref.unit(q) is None, q
    # 2l + 1 directions instead of 24 would be singular for bands 1 and 3; the 24 are not
    Y = ref.basis(ref.fibonacci())
    for (j0, w), worst in zip(ref.BANDS, (1.05, 1.15, 1.5)):
        assert np.linalg.cond(Y[:, j0 - 1:j0 - 1 + w]) <= worst


def test_apply_with_the_identity_keeps_every_finite_half():
    """every finite half, in every position, returns bit for bit -- except -0, which the sum with the other columns' +0 products
    turns into +0"""
    every = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    finite = every[(every & 0x7c00) != 0x7c00]
    h = np.resize(finite, (-(-finite.size // 16), 16)).copy()
    M = ref.m32(ref.matrices(IDENTITY_Q))
    got = ref.apply_halves(h, M)
    want = h.copy()
    want[:, 1:][want[:, 1:] == 0x8000] = 0x0000
    assert np.array_equal(got, want)
    assert (h[:, 0] == 0x8000).any() and np.array_equal(got[:, 0], h[:, 0])      # (the DC half keeps even its -0)


def test_apply_keeps_the_dc_half_and_states_the_special_values():
    h = _half_rows(7, 64)
    h[:, 0] = np.arange(64, dtype=np.uint16) * 1031 + 0x7c01                     # any bits, NaNs and infinities among them
    h[1, 2], h[2, 5], h[3, 10] = 0x7c00, 0xfc00, 0x7e01                            # +inf in band 1, -inf in band 2, a NaN in band 3
    h[4, 1:] = 0x0001                                                             # the smallest subnormal everywhere
    M = ref.m32(ref.matrices((0.3, -0.2, 0.5, 0.7)))
    got = ref.apply_halves(h, M)
    assert np.array_equal(got[:, 0], h[:, 0])
    nan = (got & 0x7c00 == 0x7c00) & (got & 0x03ff != 0)
    nan[:, 0] = False                                                             # (the DC half is nobody's result)
    assert np.array_equal(got[nan], np.full(int(nan.sum()), ref.NAN_HALF, dtype=np.uint16))
    assert nan[3, 9:].all() and not nan[3, 1:9].any()                             # a NaN spreads over its own band only
    for row, (j0, w) in ((1, ref.BANDS[0]), (2, ref.BANDS[1])):                   # an infinity: +-inf or NaN across its band, nothing beyond
        assert ((got[row, j0:j0 + w] & 0x7c00) == 0x7c00).all()
        others = np.delete(got[row, 1:], np.arange(j0 - 1, j0 - 1 + w))
        assert ((others & 0x7c00) != 0x7c00).all()
    sub = got[4, 1:].view(np.float16).astype(np.float64)
    assert (np.abs(sub) <= 3 * 2.0 ** -24).all() and (sub != 0).any()             # subnormals are kept, not flushed
    # the store rounds to nearest even, not towards zero: 1 + 2^-11 + 2^-12 in f32 becomes the half 1 + 2^-10 ...
    s = np.array([1.0 + 2.0 ** -11 + 2.0 ** -12, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65520.0], dtype=np.float32)
    assert list(s.astype(np.float16).view(np.uint16)) == [0x3c01, 0x3c00, 0x3c02, 0x7c00]   # ... ties go to even, overflow to infinity


def test_a_round_trip_stays_within_the_derived_bound():
    h = _half_rows(11, 4096)
    h[:64, 1:] = (np.random.default_rng(12).integers(0, 0x0400, (64, 15))).astype(np.uint16)     # rows of subnormals
    c = h.view(np.float16).astype(np.float64)
    worst = 0.0
    for q in _quaternions(13, 8):
        there = ref.apply_halves(h, ref.m32(ref.matrices(q)))
        back = ref.apply_halves(there, ref.m32(ref.matrices(ref.conjugate(q))))
        assert np.array_equal(back[:, 0], h[:, 0])
        b = back.view(np.float16).astype(np.float64)
        for j0, w in ref.BANDS:
            moved = np.linalg.norm(b[:, j0:j0 + w] - c[:, j0:j0 + w], axis=1)
            bound = ref.round_trip_bound(c[:, j0:j0 + w], w)
            assert (moved <= bound).all()
            worst = max(worst, float((moved / bound).max()))
    assert worst > 0.05       # (the bound is not idle: rounding really moves the coefficients)


def test_truncation_would_shrink_what_rounding_keeps():
    """why the store rounds to nearest: 64 turns by the same angle and 64 back leave the bands' length where it was, on average"""
    h = _half_rows(17, 512)
    q = (0.0, np.sin(0.05), 0.0, np.cos(0.05))
    M, Mi = ref.m32(ref.matrices(q)), ref.m32(ref.matrices(ref.conjugate(q)))
    c0 = h.view(np.float16).astype(np.float64)[:, 1:]
    for _ in range(64):
        h = ref.apply_halves(h, M)
    for _ in range(64):
        h = ref.apply_halves(h, Mi)
    c1 = h.view(np.float16).astype(np.float64)[:, 1:]
    drift = np.linalg.norm(c1, axis=1) / np.linalg.norm(c0, axis=1) - 1.0
    assert abs(drift.mean()) <= 2.0 ** -11 * 128 / np.sqrt(512) and np.abs(drift).max() <= 128 * 2.0 ** -11


def test_bake_names_the_rotation_of_the_frame():
    assert np.array_equal(ref.bake(sf.IDENTITY), [0.0, 0.0, 0.0, 1.0])
    for q in list(_quaternions(19, 40)) + [(1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.6, 0.8, 0.0, 0.0), (0.0, 0.6, 0.8, 1e-9)]:
        frame = sf.frame_rotate(sf.IDENTITY, q)                       # Linv = R(q)^T
        got = ref.bake(frame)
        assert got is not None
        same = min(np.abs(got - q).max(), np.abs(got + np.asarray(q)).max())      # (q and -q are one rotation)
        assert same <= 2.0 ** -40
        scaled = ref.bake(sf.frame_scale(frame, (2.5, 2.5, 2.5)))     # a positive uniform scale does not change the rotation
        assert scaled is not None and np.abs(scaled - got).max() <= 2.0 ** -40
        assert ref.bake(sf.frame_scale(frame, (1.0, 1.0, 1.25))) is None            # a non-uniform scale has no rotation
        assert ref.bake(sf.frame_scale(frame, (-1.0, -1.0, -1.0))) is None          # nor has a reflection
    # the condition is 2^-20: a frame just inside it is baked, one outside is not
    near = sf.IDENTITY.copy(); near[0, 1] = 2.0 ** -22
    far = sf.IDENTITY.copy(); far[0, 1] = 2.0 ** -19
    assert ref.bake(near) is not None and ref.bake(far) is None
    assert ref.bake(np.zeros((3, 3))) is None


def test_the_coefficient_form_stays_within_colour_bound_of_the_frame_form(oracle):
    """the specification alone: textures rotated by apply() and evaluated for the plain direction, against the same textures
    evaluated through the frame R(q)^T, both by the f32 specification of the projection (sh_follow_reference.colours)"""
    rng = np.random.default_rng(23)
    n, band = 240, np.array([39, 90, 160], dtype=np.int32)
    pos = (rng.standard_normal((n, 3)) * 1.5).astype(np.float32)
    view = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.25, -0.5, 6.0, 1], dtype=np.float32)
    tex = [ref.words(_half_rows(29 + ch, n - 40)) for ch in range(3)]
    q = (0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214)
    frame = sf.frame_rotate(sf.IDENTITY, q)
    turned = ref.apply(tex, band, None, ref.m32(ref.matrices(q)))
    a = sf.colours(oracle, tex, band, pos, view, frame).astype(np.float64)
    b = sf.colours(oracle, turned, band, pos, view, None).astype(np.float64)
    stale = sf.colours(oracle, tex, band, pos, view, None).astype(np.float64)
    bound = ref.colour_bound(tex, band, q, pos, view)
    assert (bound[:40] == 0).all() and (bound[40:] > 0).all() and bound.max() < 4e-3
    assert (np.abs(a - b) <= bound).all()
    assert np.abs(a - b).max() > bound.max() / 100          # (not idle)
    assert np.abs(a - stale).max() > 0.05                   # (and the rotation really moved the colours)

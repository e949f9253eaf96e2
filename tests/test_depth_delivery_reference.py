"""tests/depth_delivery_reference.py against the words of its definition ("Frame delivery with depth"): the
quantiser's special values, its ties, its monotonicity and its round trip, and the sizes of the strided plane.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import depth_delivery_reference as DD

F32_MAX = np.finfo(np.float32).max
F32_TINY = np.float32(1e-45)          # the smallest subnormal


@pytest.mark.parametrize("near", [0.1, 0.5, 1.0, 3.0])
def test_special_values(near):
    n = np.float32(near)
    z = np.array([np.inf, 0.0, -0.0, -1.0, -np.inf, np.nan, n, n / 2, np.nextafter(n, np.float32(0)), F32_MAX, F32_TINY], dtype=np.float32)
    u = DD.quantise_u16(z, near)
    assert u.dtype == np.uint16
    assert u[0] == 0                                      # no hit
    assert list(u[1:6]) == [65535] * 5                    # not in front of the camera, or not a number: "unless z > 0"
    assert list(u[6:9]) == [65535] * 3                    # at and in front of near
    assert u[9] == 0 and u[10] == 65535                   # the largest and the smallest finite z


def test_scalar_and_plane_shapes_are_kept():
    assert DD.quantise_u16(np.float32(2.0), 1.0).shape == ()
    z = np.full((3, 5), 4.0, np.float32)
    assert DD.quantise_u16(z, 1.0).shape == (3, 5) and (DD.quantise_u16(z, 1.0) == 16384).all()    # rint(16383.75)


def test_ties_round_to_even():
    # near = 1, z = 2: q = 0.5 and q * 65535 = 32767.5 are exact -- the tie goes to the even neighbour
    assert DD.quantise_u16(np.float32(2.0), 1.0) == 32768
    # every z whose binary32 product q * 65535 lands on k + 0.5: both parities of k occur, and u is always the even neighbour
    z = np.nextafter(np.float32(1.5), np.float32(2), dtype=np.float32) + np.arange(1 << 22, dtype=np.float32) * np.float32(2.0 ** -23)
    prod = np.divide(np.float32(1), z, dtype=np.float32) * np.float32(65535)
    ties = prod - np.floor(prod) == np.float32(0.5)
    k = np.floor(prod[ties]).astype(np.int64)
    assert (k % 2 == 0).any() and (k % 2 == 1).any()
    u = DD.quantise_u16(z[ties], 1.0).astype(np.int64)
    assert (u % 2 == 0).all() and (np.abs(u - k - 0.5) == 0.5).all()


def test_every_step_is_binary32():
    """against exact rational arithmetic, rounded once per operation"""
    rng = np.random.default_rng(5)
    zs = np.concatenate([rng.uniform(0.05, 200.0, 4000), 10.0 ** rng.uniform(-3, 6, 2000)]).astype(np.float32)
    for near in (0.1, 0.37, 2.0):
        n = np.float32(near)
        got = DD.quantise_u16(zs, near)
        for z, u in zip(zs[:600], got[:600]):
            q32 = _round_f32(Fraction(float(n)) / Fraction(float(z)))
            assert q32 == np.divide(n, z, dtype=np.float32)
            q32 = min(q32, np.float32(1))
            prod = _round_f32(Fraction(float(q32)) * 65535)
            assert int(u) == int(np.rint(prod)), (near, z)


def _round_f32(x):
    """a Fraction rounded to the nearest binary32, ties to even"""
    f = np.float32(float(x))                    # binary64 first: may double-round only on a binary32 tie of the binary64 value
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    best = min((lo, f, hi), key=lambda c: (abs(Fraction(float(c)) - x), int(np.float32(c).view(np.uint32)) & 1))
    return np.float32(best)


@pytest.mark.parametrize("near", [0.1, 1.0, 7.5])
def test_monotone_non_increasing_in_z(near):
    z = np.sort(np.concatenate([np.geomspace(1e-6, 1e9, 20001), [np.inf]]).astype(np.float32))
    u = DD.quantise_u16(z, near).astype(np.int64)
    assert (np.diff(u) <= 0).all() and u[0] == 65535 and u[-1] == 0


@pytest.mark.parametrize("near", [0.1, 1.0])
def test_round_trip_within_one_quantum(near):
    z = np.geomspace(near, near * 60000.0, 5001).astype(np.float32)
    u = DD.quantise_u16(z, near)
    assert (u > 0).all()
    back = DD.dequantise_u16(u, near)
    # one quantum of inverse depth: |near / z - near / back| <= 1 / 65535 (half a quantum from the rounding, the rest slack)
    assert np.abs(float(np.float32(near)) / z.astype(np.float64) - float(np.float32(near)) / back).max() <= 1.0 / 65535
    assert np.isinf(DD.dequantise_u16(np.uint16(0), near))


@pytest.mark.parametrize("W,H", [(1920, 1080), (1001, 701), (33, 17), (7, 1), (1, 1), (2, 2)])
def test_sizes_of_odd_images(W, H):
    hit = np.arange(W * H, dtype=np.float32).reshape(H, W)
    assert DD.plane_size(W, H, 1) == (W, H) and DD.subsample(hit, 1).shape == (H, W)
    Wd, Hd = DD.plane_size(W, H, 2)
    assert (Wd, Hd) == (-(-W // 2), -(-H // 2))
    s = DD.subsample(hit, 2)
    assert s.shape == (Hd, Wd) and s.flags.c_contiguous
    for j in (0, Hd - 1):
        for i in (0, Wd - 1):
            assert s[j, i] == hit[2 * j, 2 * i]
    with pytest.raises(AssertionError):
        DD.subsample(hit, 4)

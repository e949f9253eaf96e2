"""Neighbours without a GPU: the specification's two statements of the count agree -- grid_counts, through the cell construction
the device uses (side radius * (1 + 2^-10), floor, clamp, 27 cells), equals the blocked O(n^2) counts on every input family of
tests/test_gpu_neighbours.py -- and the construction is what it is for a reason: with a cell side equal to the radius a pair
the definition counts is lost, on a stated input."""
import numpy as np
import pytest

import neighbour_reference as nr

FAMILIES = nr.families()


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_the_cells_find_every_pair(case):
    name, p, radius, cap = case
    n = p.shape[0]
    want = nr.counts(p, radius, cap)
    assert np.array_equal(nr.grid_counts(p, radius, cap), want), name
    scope = np.arange(n) % 3 != 1
    want = nr.counts(p, radius, cap, scope)
    assert np.array_equal(nr.grid_counts(p, radius, cap, scope), want), name
    assert not want[~scope].any()
    h = nr.hist(want, cap, scope)
    assert int(h.sum()) == int(scope.sum()) and h.size == cap + 1
    for lo, hi in ((0, 1), (0, cap + 1), (1, 3), (2, 2)):
        assert int(nr.select(want, lo, hi, scope).sum()) == int(h[lo:hi].sum())
    assert nr.pair_floor(p, radius, scope) >= int(want.sum())       # every neighbour found is a pair tested
    assert nr.pair_floor(p, radius, scope) >= int((scope & np.isfinite(p).all(axis=1)).sum())   # and a splat meets itself


def test_the_definition_on_small_cases():
    by_name = {f[0]: f for f in FAMILIES}
    _, p, r, cap = by_name["n = 1"]
    assert nr.counts(p, r, cap).tolist() == [0]
    _, p, r, cap = by_name["n = 2 at exactly radius"]
    assert nr.counts(p, r, cap).tolist() == [1, 1]                    # distance exactly radius counts
    _, p, r, cap = by_name["n = 2 one ulp beyond"]
    assert nr.counts(p, r, cap).tolist() == [0, 0]
    _, p, r, cap = by_name["300 coincident, cap 7"]
    assert (nr.counts(p, r, cap) == 7).all() and nr.hist(nr.counts(p, r, cap), cap).tolist() == [0] * 7 + [300]
    _, p, r, cap = by_name["300 coincident, cap 4095"]
    assert (nr.counts(p, r, cap) == 299).all()                        # coincident splats count each other, none itself
    _, p, r, cap = by_name["lattice"]
    assert nr.counts(p, r, cap).max() == 6 and nr.counts(p, r, cap).min() == 3    # the six axis neighbours; three at a corner
    _, p, r, cap = by_name["non-finite rows"]
    c = nr.counts(p, r, cap)
    bad = ~np.isfinite(p).all(axis=1)
    assert nr.nonfinite(p) == int(bad.sum()) == 5 and not c[bad].any()
    assert not c[(np.abs(p) > 1e38).any(axis=1)].any()                # 3e38: finite, indexed, and nobody's neighbour
    assert np.array_equal(c[~bad], nr.counts(p[~bad], r, cap))        # such a splat is nobody's neighbour


def test_a_cell_side_equal_to_the_radius_loses_a_pair():
    """d = 0x1.ffff7p-3 is an f32; the radius is the next f64 above it, so two splats d apart are neighbours.  At x = 4 d and
    x = 5 d (both exact in f32) x * (1 / radius) rounds to just below 4 and to exactly 5: with cells of side radius the two land in
    cells 3 and 5, two apart, and the walk of +-1 cell never compares them -- floor or truncation alike.  The shipped side,
    radius * (1 + 2^-10), puts them in cells 3 and 4."""
    d = float.fromhex("0x1.ffff7p-3")
    radius = float.fromhex("0x1.ffff700000001p-3")
    assert np.float64(np.float32(d)) == d and radius == np.nextafter(d, np.inf)
    p = np.array([[4 * d, 0, 0], [5 * d, 0, 0]], np.float32)
    assert p[0, 0] == 4 * d and p[1, 0] == 5 * d
    assert nr.counts(p, radius, 8).tolist() == [1, 1]
    assert nr.cells(p, radius, side=radius, trunc=True)[0][:, 0].tolist() == [3, 5]
    assert nr.grid_counts(p, radius, 8, side=radius, trunc=True).tolist() == [0, 0]     # the pair is lost
    assert nr.grid_counts(p, radius, 8, side=radius).tolist() == [0, 0]                 # floor does not save it: the side does
    assert nr.cells(p, radius)[0][:, 0].tolist() == [3, 4]
    assert nr.grid_counts(p, radius, 8).tolist() == [1, 1]


def test_truncation_differs_from_floor_below_zero():
    p = np.array([[-0.1, 0.3, -2.7]], np.float32)
    assert nr.cells(p, 1.0)[0].tolist() == [[-1, 0, -3]]
    assert nr.cells(p, 1.0, trunc=True)[0].tolist() == [[0, 0, -2]]

"""Point-to-plane registration, the numpy specification held to what it claims (tests/surface_reference.py): the rows do not depend
on the sign of a normal, only matched splats with a normal contribute, and on the box corner the point-to-plane loop converges in
fewer steps and closer to the true motion than register_reference.register; targets of one and of two faces are degenerate, a step
with fewer than six pairs ends the loop, and a non-finite sum is refused.  No device, no library."""
import math

import numpy as np
import pytest

import register_reference as rr
import surface_reference as sr


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


@pytest.fixture(scope="module")
def corner():
    return sr.corner_scenario()


@pytest.fixture(scope="module")
def family():
    return next(f for f in sr.families() if f[0] == "257 x 300")


def test_negating_the_normals_leaves_every_sum_bit_identical(corner, family):
    for src, tgt, nrm, radius, M in ((corner["source"], corner["target"], corner["target_normals"], sr.RADIUS, None),
                                     (family[1], family[2], family[7], family[3], family[4])):
        idx, d2, _ = rr.match(src, tgt, radius, M)
        a = sr.sums(src, tgt, nrm, idx, d2, M)
        b = sr.sums(src, tgt, -nrm, idx, d2, M)
        assert a[0] == b[0] and a[1] == b[1] and a[1] > 0
        assert np.array_equal(_bits(a[2]), _bits(b[2]))
        # row by row a product that is exactly zero may change the sign of its zero (+0 * n_x), and nothing else changes; the
        # tree's padding and the empty rows are +0.0, and -0 + +0 = +0, so the sums above do not see it
        x, y = sr.rows(src, tgt, nrm, idx, M, d2), sr.rows(src, tgt, -nrm, idx, M, d2)
        assert np.array_equal(x, y) and np.array_equal(_bits(x[x != 0]), _bits(y[y != 0]))


def test_only_matched_splats_with_a_normal_have_a_row(family):
    _, src, tgt, radius, M, _, _, nrm = family
    idx, d2, info = rr.match(src, tgt, radius, M)
    x = sr.rows(src, tgt, nrm, idx, M, d2)
    matched = idx != rr.NONE
    has = np.zeros(src.shape[0], bool)
    has[matched] = ~np.isnan(nrm[idx[matched], 0])
    assert 0 < has.sum() < matched.sum() < src.shape[0]                # the family exercises all three kinds of splat
    assert (_bits(x[~has]) == 0).all()                                 # +0.0, not -0.0
    assert (x[has, 28] == d2[has]).all() and (x[has, 27] >= 0).all() and (np.abs(x[has, :21]).sum(axis=1) > 0).all()
    pairs, surface_pairs, s29 = sr.sums(src, tgt, nrm, idx, d2, M)
    assert pairs == info["matched"] == int(matched.sum()) and surface_pairs == int(has.sum())
    assert np.array_equal(_bits(s29), _bits(sr.tree(x)))
    # a component's tree is register_reference's tree of that component: the width changes nothing
    wide = np.zeros((x.shape[0], 16))
    wide[:, 3] = x[:, 27]
    assert _bits([rr.tree(wide)[3]])[0] == _bits([s29[27]])[0]


def test_the_corner_converges_in_fewer_steps_and_closer_than_point_to_point(corner):
    src, tgt, nrm, truth = corner["source"], corner["target"], corner["target_normals"], corner["M_true"]
    M, info = sr.register_surface(src, tgt, nrm, sr.RADIUS, max_iterations=64, tolerance=2.0 ** -30)
    P, pinfo = rr.register(src, tgt, sr.RADIUS, max_iterations=64, tolerance=2.0 ** -30)
    err, perr = float(np.abs(M - truth).max()), float(np.abs(P - truth).max())
    print("surface", info["iterations"], err, "point", pinfo["iterations"], perr)
    assert info["status"] == sr.CONVERGED and pinfo["status"] == rr.CONVERGED
    assert info["iterations"] < pinfo["iterations"]
    assert err < perr
    assert len(info["step_pairs"]) == len(info["step_surface_pairs"]) == len(info["step_rms"]) == len(info["step_surface_rms"]) == info["iterations"]
    assert info["surface_pairs"] == info["pairs"] > 0                  # every target splat of the corner has a normal


@pytest.mark.parametrize("faces,pivot", [((2,), 3), ((0,), 1), ((2, 0), 5), ((0, 1), 6)], ids=["z", "x", "z and x", "x and y"])
def test_one_face_and_two_faces_are_degenerate_at_step_one(corner, faces, pivot):
    tgt, _, _, nrm = sr.corner_faces(faces)
    M, info = sr.register_surface(corner["source"], tgt, nrm, sr.RADIUS, max_iterations=8, tolerance=2.0 ** -30)
    assert info["status"] == sr.DEGENERATE and info["iterations"] == 1 and info["degenerate"] == pivot
    assert info["surface_pairs"] >= sr.MIN_PAIRS and info["delta"] == math.inf
    assert np.array_equal(_bits(M), _bits(rr.IDENTITY))                # M_t, untouched
    D, rms, degenerate = sr.surface_solve(*info["step_sums"][0])
    assert degenerate == pivot and rms is None and np.array_equal(_bits(D), _bits(rr.IDENTITY))


def test_fewer_than_six_surface_pairs_is_too_few(corner):
    tgt, nrm = corner["target"], corner["target_normals"].copy()
    src = corner["source"][:5]
    M, info = sr.register_surface(src, tgt, nrm, sr.RADIUS, max_iterations=8)
    assert info["status"] == sr.TOO_FEW and info["iterations"] == 1 and info["pairs"] == info["surface_pairs"] == 5
    nrm[:] = np.nan                                                    # every splat matched, none with a normal
    M, info = sr.register_surface(corner["source"], tgt, nrm, sr.RADIUS, max_iterations=8)
    assert info["status"] == sr.TOO_FEW and info["pairs"] > 6 and info["surface_pairs"] == 0
    assert info["surface_rms"] == math.inf and info["rms"] == 0.0 and (_bits(info["step_sums"][0][1]) == 0).all()
    far = np.array([1.0, 0.0, 0.0, 500.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    M, info = sr.register_surface(corner["source"], tgt, corner["target_normals"], sr.RADIUS, M0=far)
    assert info["status"] == sr.TOO_FEW and info["pairs"] == 0 and info["rms"] == math.inf and np.array_equal(_bits(M), _bits(far))


def test_the_solve_refuses_what_the_header_says(corner):
    idx, d2, _ = rr.match(corner["source"], corner["target"], sr.RADIUS)
    _, surface_pairs, s29 = sr.sums(corner["source"], corner["target"], corner["target_normals"], idx, d2)
    D, rms, degenerate = sr.surface_solve(surface_pairs, s29)
    assert degenerate == 0 and math.isfinite(rms) and np.isfinite(D).all()
    for k, v in ((0, math.nan), (20, math.inf), (24, -math.inf), (28, math.nan)):
        bad = s29.copy()
        bad[k] = v
        with pytest.raises(ValueError):
            sr.surface_solve(surface_pairs, bad)
    with pytest.raises(ValueError):
        sr.surface_solve(5, s29)
    # the step is a rotation: R R^T = 1 within rounding, though no sin or cos made it
    R = D.reshape(3, 4)[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15

"""tests/register_reference.py against itself (no GPU): the tree against math.fsum and against a scalar restatement of its
definition, the rigid solve on exact pairs of a known motion, compose and decompose, the match against a brute-force loop, and the
noiseless registration scenario the GPU tests run."""
import math

import numpy as np
import pytest

import register_reference as rr


def _tree_by_definition(x):
    """the definition once more, one addition at a time"""
    x = [list(map(float, row)) for row in x]
    if not x:
        return [0.0] * 16
    while True:
        out = []
        for g in range(0, len(x), 256):
            grp = x[g:g + 256] + [[0.0] * 16 for _ in range(256 - len(x[g:g + 256]))]
            s = 128
            while s:
                for l in range(s):
                    grp[l] = [a + b for a, b in zip(grp[l], grp[l + s])]
                s //= 2
            out.append(grp[0])
        x = out
        if len(x) == 1:
            return x[0]


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1000, 65537])
def test_tree_is_its_definition_and_close_to_fsum(n):
    rng = np.random.default_rng(n)
    x = rng.normal(0.0, 1.0, (n, 16)) * np.exp(rng.normal(0.0, 3.0, (n, 16)))
    got = rr.tree(x)
    if n <= 1000:
        assert np.array_equal(got.view(np.uint64), np.array(_tree_by_definition(x), np.float64).view(np.uint64))
    # Every input passes through at most `depth` additions, each with a relative error of at most u = 2^-53, so
    # |tree - exact| <= gamma_depth * sum |x| with gamma_k = k u / (1 - k u); fsum is the exact sum rounded once (one more u).
    levels = 0
    rows = n
    while True:
        rows = (rows + 255) // 256
        levels += 1
        if rows <= 1:
            break
    depth, u = 8 * levels, 2.0 ** -53
    gamma = depth * u / (1.0 - depth * u)
    for c in range(16):
        exact, mag = math.fsum(x[:, c]), math.fsum(np.abs(x[:, c]))
        assert abs(got[c] - exact) <= gamma * mag + u * abs(exact), (n, c)


def test_tree_depends_on_the_order_of_its_rows():
    """it is a function of the rows IN ORDER: nothing but the definition leaves the bits alone"""
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 1.0, (1000, 16))
    a, b = rr.tree(x), rr.tree(x[::-1])
    assert not np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert not np.array_equal(a.view(np.uint64), x.sum(axis=0).view(np.uint64))


def _exact_pairs(R, t, n=200, seed=2):
    rng = np.random.default_rng(seed)
    T = rng.normal(0.0, 1.0, (n, 3)) * np.array([1.0, 0.4, 0.7])
    Q = T @ R.T + t
    rows = np.zeros((n, 16))
    rows[:, 0:3], rows[:, 3:6] = T, Q
    for a in range(3):
        for b in range(3):
            rows[:, 6 + 3 * a + b] = T[:, a] * Q[:, b]
    return n, rr.tree(rows)


@pytest.mark.parametrize("angle,axis", [(0.12, (0.3, 0.9, 0.2)), (1.0, (1, 0, 0)), (3.1, (1, 0.01, 0)), (3.1, (0, 1, 0.01)), (3.1, (0.01, 0, 1)), (0.0, (0, 0, 1)),
                                        (2.0, (-0.5, 0.5, 0.7))])
def test_rigid_solve_returns_a_known_motion_and_decompose_inverts_it(angle, axis):
    R, t = rr.motion(angle, axis, (0.5, -0.25, 2.0))
    pairs, s16 = _exact_pairs(R, t)
    D, rms = rr.rigid_solve(pairs, s16)
    want = np.concatenate([R, t[:, None]], axis=1).reshape(12)
    # 200 pairs spread over a unit cloud: the sums carry a relative error near 200 * 2^-53, the cloud's smallest spread (0.4)
    # conditions the rotation by less than ten, and 8 sweeps leave the off-diagonal below the rounding level: 1e-12 is generous
    assert np.abs(D - want).max() < 1e-12, (D, want)
    assert rms == 0.0                                  # d2 sums of zero
    q, tt = rr.rigid_decompose(D)
    assert np.array_equal(tt, D.reshape(3, 4)[:, 3])
    x, y, z, w = q
    assert abs(((x * x + y * y) + z * z) + w * w - 1.0) < 1e-12
    Rq = np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w],
                   [2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w],
                   [2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y]])
    assert np.abs(Rq - D.reshape(3, 4)[:, :3]).max() < 1e-11


def test_rigid_solve_refuses_and_compose_composes():
    with pytest.raises(ValueError):
        rr.rigid_solve(2, np.zeros(16))
    bad = np.zeros(16)
    bad[7] = np.inf
    with pytest.raises(ValueError):
        rr.rigid_solve(5, bad)
    Ra, ta = rr.motion(0.3, (1, 2, 3), (1.0, 2.0, 3.0))
    Rb, tb = rr.motion(-0.7, (0, 1, 1), (-0.5, 0.0, 0.25))
    A, B = np.concatenate([Ra, ta[:, None]], axis=1), np.concatenate([Rb, tb[:, None]], axis=1)
    C = rr.rigid_compose(A, B).reshape(3, 4)
    p = np.array([0.3, -1.2, 0.8])
    assert np.abs(C[:, :3] @ p + C[:, 3] - (Ra @ (Rb @ p + tb) + ta)).max() < 1e-15
    assert np.array_equal(rr.rigid_compose(rr.IDENTITY, B), B.reshape(12))


def test_match_equals_a_brute_force_loop():
    name, src, tgt, radius, M = [f for f in rr.families() if f[0] == "non-finite rows"][0]
    smask, tmask = np.arange(src.shape[0]) % 4 != 1, np.arange(tgt.shape[0]) % 3 != 0
    idx, d2, info = rr.match(src, tgt, radius, M, smask, tmask)
    t, ok = rr.transform(src, M)
    r2 = radius * radius
    for i in range(src.shape[0]):
        if not smask[i]:
            assert idx[i] == rr.NONE and math.isnan(d2[i])
            continue
        best = (math.inf, rr.NONE)
        if ok[i]:
            for j in range(tgt.shape[0]):
                if not tmask[j] or not np.isfinite(tgt[j]).all():
                    continue
                e = [float(t[i, k]) - float(tgt[j, k]) for k in range(3)]
                d = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                if d <= r2 and (d, j) < best:
                    best = (d, j)
        assert (float(d2[i]), int(idx[i])) == best, i
    assert info["matched"] == int((idx != rr.NONE).sum()) and info["in_scope"] == int(smask.sum())
    assert info["pair_bound"] >= info["matched"]


def test_families_are_what_they_claim():
    fam = {f[0]: f for f in rr.families()}
    _, src, tgt, radius, M = fam["lattice, radius = spacing"]
    idx, d2, info = rr.match(src, tgt, radius, M)
    assert (d2[idx != rr.NONE] == radius * radius).any() and (d2 == 0.0).any()      # a distance of exactly the radius counts
    assert (d2 == 0.125 * 0.125).any() and info["matched"] < src.shape[0]
    _, src, tgt, radius, M = fam["coincident targets"]
    idx, d2, _ = rr.match(src, tgt, radius, M)
    assert idx.tolist() == [1, 0, 1, rr.NONE] and d2[0] == 0.0                       # the tie goes to the smaller index
    _, src, tgt, radius, M = fam["M overflows for some rows"]
    _, _, info = rr.match(src, tgt, radius, M)
    assert info["nonfinite"] == 33 and info["matched"] > 0
    for name in ("2^19 radii out", "beyond the clamp"):
        _, src, tgt, radius, M = fam[name]
        _, _, info = rr.match(src, tgt, radius, M)
        assert 0 < info["matched"] < src.shape[0], name


@pytest.mark.parametrize("floaters", [False, True])
def test_the_noiseless_scenario_converges(floaters):
    src, tgt, partner = rr.scenario(floaters)
    M, info = rr.register(src, tgt, rr.RADIUS, None, max_iterations=12, tolerance=2.0 ** -40)
    print(info)
    if floaters:                                       # floaters pull the fit: it must still end, and close to the motion
        assert info["status"] in (rr.CONVERGED, rr.MAX_ITERATIONS)
        R, t = rr.motion()
        assert np.abs(M.reshape(3, 4) - np.concatenate([R, t[:, None]], axis=1)).max() < 0.05
        return
    assert info["status"] == rr.CONVERGED and info["iterations"] <= 12
    assert info["pairs"] == rr.PARTNERS
    # coordinates below 4 are stored with at most half an f32 ulp (2^-23) of error each, so the TRUE motion leaves a residual of
    # at most sqrt(3) * 2^-23 per pair, and a least-squares fit cannot do worse than the truth
    assert info["rms"] <= math.sqrt(3.0) * 2.0 ** -23
    idx, d2, _ = rr.match(src, tgt, rr.RADIUS, M)
    assert np.array_equal(idx[:rr.PARTNERS], partner) and (idx[rr.PARTNERS:] == rr.NONE).all()

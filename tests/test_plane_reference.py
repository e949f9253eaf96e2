"""The specification of "Planes" checked against itself and by hand, without a GPU: pinned vectors of the generator, scores and the
closed interval on cases small enough to count on paper, the tie rule, the reference alone finding the floor of the 8192-splat
family, and gsr_plane_alignment of the built library -- a pure function -- bit for bit against plane_reference.alignment."""
import ctypes

import numpy as np
import pytest

import plane_reference as pr


def test_pinned_mix_and_rank_vectors():
    # splitmix64 seeded with 0 yields these as its first three outputs: mix(k * golden) is output k + 1
    golden = 0x9E3779B97F4A7C15
    assert [pr.mix((k * golden) & pr.MASK64) for k in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert pr.mix(1) == 0x910A2DEC89025CC1 and pr.mix(pr.MASK64) == pr.mix(-1 & pr.MASK64)
    assert pr.mulhi64(pr.MASK64, pr.MASK64) == pr.MASK64 - 1 and pr.mulhi64(1 << 63, 6) == 3 and pr.mulhi64(12345, 1) == 0
    assert pr.rank(0, 0, 0, 1000) == 883                                # 0xE220.. / 2^64 * 1000
    assert [pr.rank(7, h, j, 1) for h in range(3) for j in range(3)] == [0] * 9
    assert pr.rank(pr.MASK64, 1, 0, 1 << 32) == pr.mix(2) >> 32         # the seed wraps: MASK64 + 3 = 2
    for m in (3, 64, 8192, (1 << 32) - 1):
        assert all(0 <= pr.rank(5, h, j, m) < m for h in range(50) for j in range(3))


def test_candidates_drop_non_finite_rows_and_follow_the_scope():
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 1, 1], [0, np.inf, 0], [2, 2, 2], [0, 0, -np.inf]], np.float32)
    cand, in_scope, nonfinite = pr.candidates(p)
    assert cand.tolist() == [0, 2, 4] and (in_scope, nonfinite) == (6, 3)
    cand, in_scope, nonfinite = pr.candidates(p, np.array([0, 1, 1, 0, 1, 1], bool))
    assert cand.tolist() == [2, 4] and (in_scope, nonfinite) == (4, 2)


def test_hypotheses_by_hand():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32)
    cand = np.arange(3, dtype=np.uint32)
    planes, tri, deg = pr.hypotheses(p, cand, 65, 3)
    for h in range(65):
        r = [pr.rank(3, h, j, 3) for j in range(3)]
        assert tri[h].tolist() == r
        assert deg[h] == (len(set(r)) < 3)
        if not deg[h]:
            # the one plane through the three: normal (0, -0.5, 1) / sqrt(1.25), the first component that is not zero positive
            n = planes[h, :3]
            assert abs(n[0]) == 0 and n[1] > 0 and np.allclose(n, [0, 0.5 / np.sqrt(1.25), -1 / np.sqrt(1.25)], rtol=0, atol=1e-15)
            assert abs(planes[h, 3]) < 1e-15
            assert ((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) == pytest.approx(1.0, abs=4e-16)
    assert 0 < deg.sum() < 65
    # coincident and colinear triples have no normal
    _, _, deg = pr.hypotheses(np.tile(np.float32([[0.5, 0.5, 0.5]]), (70, 1)), np.arange(70, dtype=np.uint32), 63, 0)
    assert deg.all()
    line = (np.arange(100)[:, None] * np.array([[0.25, -0.5, 0.125]])).astype(np.float32)
    _, _, deg = pr.hypotheses(line, np.arange(100, dtype=np.uint32), 64, 0)
    assert deg.all()


def test_the_sign_rule_keeps_a_negative_zero():
    # A, B, C with N = (0, -0.5, 1): negated, so nx becomes -0.0 and stays part of the result
    p = np.array([[1, 0, 0], [0, 1, 0.5], [0, 0, 0]], np.float32)
    for seed in range(200):
        if [pr.rank(seed, 0, j, 3) for j in range(3)] == [0, 1, 2]:
            break
    planes, _, deg = pr.hypotheses(p, np.arange(3, dtype=np.uint32), 1, seed)
    assert not deg[0] and planes[0, 1] > 0 and planes[0, 2] < 0
    assert planes[0, 0] == 0 and np.signbit(planes[0, 0])


def test_scores_and_the_closed_interval_by_hand():
    up, down = np.nextafter(np.float32(0.75), np.float32(np.inf)), np.nextafter(np.float32(0.25), np.float32(-np.inf))
    z = np.array([0.25, 0.5, 0.75, up, down, np.nan, np.inf], np.float32)
    p = np.stack([np.arange(7, dtype=np.float32), np.zeros(7, np.float32), z], axis=1)
    cand, in_scope, nonfinite = pr.candidates(p)
    assert cand.tolist() == [0, 1, 2, 3, 4] and nonfinite == 2
    plane = (0.0, 0.0, 1.0, -0.5)
    assert pr.scores(p, cand, [plane], 0.25).tolist() == [3]
    assert pr.scores(p, cand, [plane, (0, 0, 2, -1), (0, 0, 1, 0)], 0.5).tolist() == [5, 3, 3]   # used as given: twice the plane is half the band
    assert pr.scores(p, cand, [plane], 0.25, np.array([True])).tolist() == [0]                   # a degenerate hypothesis scores 0
    assert pr.select(p, plane, -0.25, 0.25).tolist() == [True, True, True, False, False, False, False]
    assert pr.select(p, plane, 0.25, np.inf).tolist() == [False, False, True, True, False, False, True]
    assert pr.select(p, plane, -np.inf, -0.25).tolist() == [True, False, False, False, True, False, False]
    assert pr.select(p, plane, -np.inf, np.inf).sum() == 6             # never the NaN


def test_ties_go_to_the_smallest_hypothesis():
    name, p, t, h, seed = [f for f in pr.families() if f[0] == "two parallel lattice planes"][0]
    info, sc = pr.fit(p, t, h, seed)
    top = int(sc.max())
    winners = np.nonzero(sc == top)[0]
    assert top == 64 and winners.size >= 2 and info["best"] == int(winners[0]) and info["inliers"] == 64
    planes, _, _ = pr.hypotheses(p, pr.candidates(p)[0], h, seed)
    assert {float(planes[w, 3]) for w in winners} == {0.0, -1.0}       # both lattice planes are among the winners


def test_small_scenes_find_nothing():
    for name, p, t, h, seed in pr.families()[:2]:
        info, sc = pr.fit(p, t, h, seed)
        assert info["found"] == 0 and info["degenerate"] == h and not sc.any() and not info["plane"].any(), name
    info, _ = pr.fit(np.zeros((0, 3), np.float32), 0.1, 8)
    assert info["in_scope"] == info["hypotheses"] == info["degenerate"] == info["found"] == 0
    info, _ = pr.fit(np.full((4, 3), np.nan, np.float32), 0.1, 8)      # in scope, and no candidate: every hypothesis is degenerate
    assert (info["in_scope"], info["nonfinite"], info["hypotheses"], info["degenerate"], info["found"], info["tests"]) == (4, 4, 8, 8, 0, 0)


def test_the_reference_alone_finds_the_floor():
    p, n_true, floor = pr.floor_scene()
    assert p.shape == (pr.FLOOR_N, 3) and np.abs(p).max() <= 4.0 and floor.sum() == (pr.FLOOR_N * 6) // 10
    info, _ = pr.fit(p, pr.FLOOR_THRESHOLD, pr.FLOOR_HYPOTHESES)
    off = 1.0 - abs(float(info["plane"][:3] @ n_true))
    kept = int((pr.select(p, info["plane"], -pr.FLOOR_THRESHOLD, pr.FLOOR_THRESHOLD) & floor).sum())
    print("1 - |n . n_true| = %.3g, %d of the floor's %d splats are inliers, %d inliers in all" % (off, kept, floor.sum(), info["inliers"]))
    assert info["found"] == 1 and off < 1e-3
    assert kept >= 0.95 * floor.sum()
    assert info["inliers"] == int(pr.select(p, info["plane"], -pr.FLOOR_THRESHOLD, pr.FLOOR_THRESHOLD).sum())   # the consistency guarantee, in the reference


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.spacing(np.maximum(np.abs(b), 2.0 ** -60))


def test_alignment_of_the_library_equals_the_reference_bit_for_bit():
    import gsplat_hip as gh
    rng = np.random.default_rng(3)
    cases = [((0, 0, 1, -0.5), (0, 1, 0)), ((0, 1, 0, 0), (0, 1, 0)), ((0, -3, 0, 3), (0, 1, 0)), ((0, -1, 0, 0.25), (0, 2, 0)), ((-1, 0, 0, 1), (1, 0, 0)),
             ((0, 0, -1, 2), (0, 0, 5)), ((1e-9, -1, 0, 0.5), (0, 1, 0)), ((3e-4, -1, 2e-4, 0.5), (0, 1, 0)), ((2e-3, -1, 0, 0.5), (0, 1, 0)),
             ((1, 1, -2, 3), (-1, -1, 2)), (pr.fit(*pr.families()[-1][1:])[0]["plane"], (0, 1, 0))]
    cases += [(rng.normal(0, 1, 4) * 10.0 ** rng.integers(-3, 4), rng.normal(0, 1, 3)) for _ in range(40)]
    half_turns = 0
    for plane, axis in cases:
        q, t = gh.plane_alignment(plane, axis)
        wq, wt = pr.alignment(plane, axis)
        assert np.array_equal(q.view(np.uint64), wq.view(np.uint64)) and np.array_equal(t.view(np.uint64), wt.view(np.uint64)), (plane, axis, q, wq, t, wt)
        half_turns += int(q[3] == 0)
        # R n = a to 4 ulp (of 1), and the plane's points land on axis . p = 0
        n = np.asarray(plane[:3], np.float64) / np.linalg.norm(plane[:3])
        a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
        R = pr.quat_matrix(q)
        c = float(n @ a)
        if q[3] != 0:
            assert c > -1.0 + 2.0 ** -20
            # 4 ulp wherever n and a are no more than a right angle apart.  Beyond it w = 1 + c cancels: c carries an absolute error
            # of an ulp or two whatever its size, the turn's angle is 2 atan(|v| / w), and d(angle) = dw * sqrt((1 - c) / (1 + c)), so
            # the same 4 ulp grow by that factor (1 at c = 0, 1450 at the branch's edge c = -1 + 2^-20)
            grow = max(1.0, float(np.sqrt((1.0 - c) / (1.0 + c))))
            err = np.abs(R @ n - a).max()
            print("c = %+.9f  |R n - a| = %.3g = %.2f of the bound" % (c, err, err / (4 * 2.0 ** -52 * grow)))
            assert err <= 4 * 2.0 ** -52 * grow, (plane, axis, R @ n, a)
        else:
            # the half turn takes n to -n, which lies within sqrt(2 + 2 c) <= 2^-9.5 of a
            assert c <= -1.0 + 2.0 ** -20
            assert np.abs(R @ n + n).max() <= 4 * 2.0 ** -52, (plane, axis, R @ n, n)
            assert np.linalg.norm(R @ n - a) <= 2.0 ** -9.5 * (1 + 2.0 ** -40)
            continue
        on_plane = -plane[3] / float(np.dot(plane[:3], plane[:3])) * np.asarray(plane[:3], np.float64)
        assert abs(float(a @ (R @ on_plane + t))) <= 16 * 2.0 ** -52 * max(1.0, float(np.abs(on_plane).max()))
    assert half_turns >= 5                                             # the antiparallel branch, exact and within 2^-20 of it
    assert _ulps(gh.plane_alignment((0, 0, 1, -0.5))[0], [-np.sqrt(0.5), 0, 0, np.sqrt(0.5)]).max() <= 1


def test_alignment_refusals_need_no_device():
    import gsplat_hip as gh
    L = gh.load_library()
    q, t = np.full(4, 7.0), np.full(3, 7.0)
    ok, axis = np.array([0.0, 0.0, 1.0, 0.5]), np.array([0.0, 1.0, 0.0])
    call = lambda p, a, qq=q, tt=t: L.gsr_plane_alignment(None if p is None else p.ctypes.data, None if a is None else a.ctypes.data,
                                                            None if qq is None else qq.ctypes.data, None if tt is None else tt.ctypes.data)
    bad = [(None, axis), (ok, None), (np.array([0.0, 0.0, 0.0, 1.0]), axis), (ok, np.zeros(3)), (np.array([np.nan, 0, 1, 0]), axis),
           (np.array([0, 0, 1, np.inf]), axis), (ok, np.array([0, np.inf, 0])), (ok, np.array([np.nan, 1, 0]))]
    for k, (p, a) in enumerate(bad):
        assert call(p, a) == -1, k
        assert L.gsr_last_error(None), k
        assert (q == 7.0).all() and (t == 7.0).all(), k
    assert call(ok, axis, None, t) == -1 and call(ok, axis, q, None) == -1
    assert call(ok, axis) == 0 and not (q == 7.0).all()
    with pytest.raises(gh.GsplatError) as ei:
        gh.plane_alignment((0, 0, 0, 1))
    assert ei.value.code == -1 and "normal is zero" in str(ei.value)
    assert ctypes.sizeof(gh.GsrPlaneInfo) == 88

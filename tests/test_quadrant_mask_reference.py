"""The staging mask of the compositor (tests/quadrant_mask_reference.py: k_blend.hip's rule in numpy f32) against brute force:
no (splat, quadrant) pair with a covered pixel centre is ever left unflagged -- on the coverage scenes of the compositor tests
and on three families of records aimed at the diagonal axes -- and the four-axis rule is strictly tighter than the two-axis one.
No GPU: records come from the oracle's projection or are written down directly."""
import numpy as np
import pytest

import blend_reference as BR
import quadrant_mask_reference as QM
from depth_reference import coverage_q
from test_oracle_render import make_scene

_f32 = np.float32
FRAMES = [(96, 96), (256, 96)]


def _counts(rec, W, H):
    """over every bin of the frame: covered pairs, pairs the four-axis / two-axis rule flags, covered pairs either one loses,
    pairs the four-axis rule flags and the two-axis rule does not"""
    tot = dict(covered=0, four=0, two=0, lost_four=0, lost_two=0, wider=0)
    for bx, by in QM.bins_of(W, H):
        cov, four, two = QM.covered(rec, bx, by), QM.four_axes(rec, bx, by), QM.two_axes(rec, bx, by)
        tot["covered"] += int(cov.sum()); tot["four"] += int(four.sum()); tot["two"] += int(two.sum())
        tot["lost_four"] += int((cov & ~four).sum()); tot["lost_two"] += int((cov & ~two).sum())
        tot["wider"] += int((four & ~two).sum())
    return tot


def _check(rec, W, H, what, min_covered):
    t = _counts(rec, W, H)
    print("\nquadrant masks %-34s covered %6d  two axes %6d  four axes %6d" % (what, t["covered"], t["two"], t["four"]), end="")
    assert t["covered"] >= min_covered, (what, t)
    assert t["lost_four"] == 0 and t["lost_two"] == 0, (what, t)
    assert t["wider"] == 0 and t["four"] < t["two"], (what, t)      # strictly tighter: the code under test is the new rule
    return t


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("seed", [3, 11, 29])
def test_no_covered_quadrant_is_lost_on_the_coverage_scenes(oracle, size, seed):
    W, H = size
    cam, splats = BR.coverage_scene(W, H, [(0, 0, W, H)], seed=seed, per_region=400, giants=True)
    data, pos = make_scene(oracle, splats)
    v, p, vp = cam.f32()
    rec, bbox, raw = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
    rec = np.asarray(rec, _f32).reshape(-1, 8)
    vis = np.asarray(raw, _f32).reshape(-1, 12)[:, 11] == 1
    assert vis.sum() > 300
    _check(rec[vis], W, H, "coverage scene %dx%d seed %d" % (W, H, seed), min_covered=2000)


def _record(cx, cy, a, b, theta):
    """the record of an ellipse with semi-axes a, b (pixels) at angle theta: u = 2 major / |major|^2, w = 2 minor / |minor|^2"""
    c, s = np.cos(theta), np.sin(theta)
    return [cx, cy, 2.0 / a * c, 2.0 / a * s, -2.0 / b * s, 2.0 / b * c, -1.0, 0.0]


def corner_records(W, H, seed, count=1500):
    """Small splats whose outline passes a quadrant's corner pixel centre at +-45 degrees of their own axes (vPosition on a
    diagonal), within 1e-3 px inside or outside, the quadrant lying on the far side of that pixel: the diagonal test decides,
    at its threshold."""
    rng = np.random.default_rng(seed)
    out, aimed = [], []
    for _ in range(count):
        a = float(np.exp(rng.uniform(np.log(0.8), np.log(30.0))))
        b = a * float(rng.uniform(0.05, 1.0))
        theta = float(rng.uniform(0.0, 2 * np.pi))
        u, w = _record(0, 0, a, b, theta)[2:4], _record(0, 0, a, b, theta)[4:6]
        sw = float(rng.choice([-1.0, 1.0]))                       # which diagonal: n = (1, sw) / sqrt 2
        sn = float(rng.choice([-1.0, 1.0]))                       # on which side of the centre
        n = np.array([u[0] + sw * w[0], u[1] + sw * w[1]]) * sn    # v . (1, sw) grows along +n in pixel space
        # the quadrant's corner pixel nearest the splat: its first column / row where n points into the quadrant
        px = 8 * int(rng.integers(0, W // 8)) + (0 if n[0] > 0 else 7)
        py = 8 * int(rng.integers(0, H // 8)) + (0 if n[1] > 0 else 7)
        # vPosition of that pixel: sqrt 2 (1, sw) sn, radius 2, moved t pixels in or out; d = vx a / 2 u^ + vy b / 2 w^
        d0 = np.sqrt(0.5) * np.array([a * np.cos(theta) + sw * -b * np.sin(theta), a * np.sin(theta) + sw * b * np.cos(theta)]) * sn
        t = float(rng.choice([0.0, 1e-5, 1e-4, 1e-3])) * float(rng.choice([-1.0, 1.0]))
        d = d0 * (1.0 + t / np.hypot(*d0))
        out.append(_record(px + 0.5 - d[0], py + 0.5 - d[1], a, b, theta))
        aimed.append((px, py))
    return np.array(out, dtype=_f32), aimed


def cancelling_records(W, H, seed, count=1200):
    """|ux| ~ |wx| (and |uy| ~ |wy|): near-isotropic splats at 45 degrees to the pixel grid, so that a component of u + w or of
    u - w nearly cancels"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        a = float(np.exp(rng.uniform(np.log(0.8), np.log(60.0))))
        b = a * (1.0 + float(rng.choice([0.0, 1e-7, -1e-7, 1e-4, -1e-3, 0.02])))
        theta = np.pi / 4 + np.pi / 2 * int(rng.integers(0, 4)) + float(rng.choice([0.0, 1e-7, -1e-6, 1e-3]))
        out.append(_record(rng.uniform(-a, W + a), rng.uniform(-a, H + a), a, b, theta))
    return np.array(out, dtype=_f32)


def clamp_records(W, H, seed, count=600):
    """axes at and just under the projection's 1024-pixel clamp, the minor one from the thinnest the projection makes to the
    clamp itself, centres up to an axis length away from the frame"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        a = 1024.0 * float(rng.choice([1.0, 1.0 - 2.0 ** -20, 0.99, 0.7]))
        b = min(a, float(np.exp(rng.uniform(np.log(0.78), np.log(1024.0)))))
        theta = float(rng.uniform(0.0, 2 * np.pi))
        r = float(rng.uniform(0.0, 1.05)) * a
        out.append(_record(W / 2 + r * np.cos(theta) + rng.uniform(-40, 40), H / 2 + r * np.sin(theta) + rng.uniform(-40, 40), a, b, theta))
    return np.array(out, dtype=_f32)


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
def test_no_covered_quadrant_is_lost_at_the_diagonals(size):
    W, H = size
    for seed in (1, 2):
        rec = corner_records(W, H, seed)[0]
        t = _check(rec, W, H, "corners %dx%d seed %d" % (W, H, seed), min_covered=3000)
        # ... and it has teeth: without the slack and 0.002 more, covered pairs are lost
        lost = sum(int((QM.covered(rec, bx, by) & ~QM.four_axes(rec, bx, by, cp=2.0 * np.sqrt(2.0) - 0.002)).sum()) for bx, by in QM.bins_of(W, H))
        assert lost > 20, (lost, t)
        _check(cancelling_records(W, H, seed), W, H, "cancelling %dx%d seed %d" % (W, H, seed), min_covered=3000)
        _check(clamp_records(W, H, seed), W, H, "clamp %dx%d seed %d" % (W, H, seed), min_covered=3000)


def test_the_corner_family_sits_on_the_threshold():
    """the aimed pixel of every corner record: vPosition on a diagonal, |vPosition| = 2 (1 + t / |d|) with |t| <= 1e-3 px and
    |d|^2 = (a^2 + b^2) / 2 >= 0.32, so within 3.6e-3 of 2 (plus the f32 rounding of the record and of q)"""
    W, H = 96, 96
    rec, aimed = corner_records(W, H, 1, count=400)
    inside = 0
    for rc, (px, py) in zip(rec, aimed):
        q = float(coverage_q(rc, np.array([px]), np.array([py]))[0, 0])
        assert abs(np.sqrt(q) - 2.0) <= 3.6e-3 + 1e-4, (rc, px, py, q)
        inside += q <= 4.0
    assert 0.25 * len(rec) <= inside <= 0.75 * len(rec), inside

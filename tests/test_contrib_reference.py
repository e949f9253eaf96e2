"""The contribution specification (tests/contrib_reference.py) pinned before anything trusts it: hand cases, the slack of its
bounds against f32 runs of the device's recurrence on C1, its teeth against three passes that are subtly wrong, and the
order-independence of the accumulated integers.  No GPU: everything is fed by the oracle."""
import numpy as np
import pytest

import blend_reference as BR
import contrib_reference as CR
from test_oracle_render import make_scene


def _project(oracle, cam, data, pos, W, H):
    v, p, vp = cam.f32()
    rec, bbox, raw = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
    return rec, bbox, oracle.sort(vp, pos)[0], W, H


def _built(oracle, cam, splats, W, H):
    return _project(oracle, cam, *make_scene(oracle, splats), W, H)


@pytest.fixture(scope="module")
def c1(oracle, scenes):
    """C1 at poses 3 and 40: the two views, their f32 simulations, and the reference of both accumulated"""
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H, n = cfg["width"], cfg["height"], cfg["n"]
    _, data, pos = scenes("C1")
    views = [_project(oracle, gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"]), data, pos, W, H) for k in (3, 40)]
    sims = [CR.simulate(*v, n) for v in views]
    return views, sims, CR.contrib_reference(views, n), n


# ---- hand cases --------------------------------------------------------------------------------------------------------
def test_one_opaque_splat(oracle):
    W = H = 65
    cam, to_world = BR.front_view(W, H)
    view = _built(oracle, cam, BR.stack(to_world, 32.5, 32.5, 1, 20.0, (255, 255, 255, 255)), W, H)
    rec = view[0]
    ref = CR.contrib_reference([view], 1)
    q = BR.coverage_q(rec[0], np.arange(W), np.arange(H))
    assert 100 < (q <= 4).sum() < W * H and ref["pixels"][0] == (q <= 4).sum() and ref["frames"] == 1
    B = np.exp2(BR.exponent(q, rec[0, 6]).astype(np.float64))
    assert q[32, 32] == q.min() and ref["peak"][0] == B[32, 32] and B[32, 32] > 0.99       # alone, T = 1: w = B, largest at the centre pixel
    assert np.isclose(ref["weight"][0], (B[q <= 4] * 2.0 ** 24).sum(), rtol=1e-12)
    sim = CR.simulate(*view, 1)
    assert sim[2][0] == ref["pixels"][0] and max(CR.excess(sim, ref)) <= 1.0


@pytest.mark.parametrize("swap", [False, True])
def test_two_colocated_splats_the_back_one_is_scaled_by_T(oracle, swap):
    W = H = 65
    cam, to_world = BR.front_view(W, H)
    a = BR.stack(to_world, 32.5, 32.5, 1, 20.0, (255, 255, 255, 128))
    b = BR.stack(to_world, 32.5, 32.5, 1, 20.0, (255, 255, 255, 128), dz0=0.5)
    view = _built(oracle, cam, b + a if swap else a + b, W, H)
    front, back = (1, 0) if swap else (0, 1)
    assert view[2].tolist() == [front, back]
    ref = CR.contrib_reference([view], 2)
    rec = view[0]
    qf, qb = (BR.coverage_q(rec[i], np.arange(W), np.arange(H)) for i in (front, back))
    Bf = np.where(qf <= 4, np.exp2(BR.exponent(qf, rec[front, 6]).astype(np.float64)), 0.0)
    Bb = np.where(qb <= 4, np.exp2(BR.exponent(qb, rec[back, 6]).astype(np.float64)), 0.0)
    assert np.isclose(ref["weight"][front], Bf.sum() * 2.0 ** 24, rtol=1e-12)
    assert np.isclose(ref["weight"][back], ((1.0 - Bf) * Bb).sum() * 2.0 ** 24, rtol=1e-12)
    assert ref["peak"][back] == ((1.0 - Bf) * Bb).max() < 0.3 < ref["peak"][front]
    assert ref["pixels"][front] == (qf <= 4).sum() and ref["pixels"][back] == (qb <= 4).sum()


def test_a_splat_behind_T_zero_has_pixels_and_nothing_else(oracle):
    """the 4100-entry grey stack with a small splat behind its centre: in f32 T is exactly 0 there in front of that last splat"""
    W, H = BR.STACK_FRAME
    cam, splats, last = CR.hidden_stack_scene(4100)
    view = _built(oracle, cam, splats, W, H)
    assert view[2][-1] == last and view[2][0] == 0
    weight, peak, pixels = CR.simulate(*view, len(splats))
    assert 50 < pixels[last] < 400 and weight[last] == 0 and peak[last] == 0.0
    assert weight[0] > 0 and pixels[0] == W * H
    # (the stack's own bright splat covers the frame: where the stack's B is at most 1/2, T sticks at the smallest denormal)
    assert pixels[last - 1] == W * H and weight[last - 1] == 0 and peak[last - 1] <= np.float32(2.0 ** -149)
    ref = CR.contrib_reference([view], len(splats))
    assert ref["pixels"][last] == pixels[last] and ref["weight"][last] < 1e-100 and ref["peak"][last] < 1e-100
    assert max(CR.excess((weight, peak, pixels), ref)) <= 1.0 and np.array_equal(pixels, ref["pixels"])


# ---- slack -------------------------------------------------------------------------------------------------------------
def test_f32_runs_of_the_recurrence_lie_inside_the_bounds(c1):
    views, sims, ref, n = c1
    both = CR.combine(*sims)
    assert np.array_equal(both[2], ref["pixels"]) and ref["frames"] == 2
    assert max(CR.excess(both, ref)) <= 1.0
    exact = CR.contrib_reference(views, n, e_exp=0.0)          # a correctly rounded exponential needs no E_EXP
    assert max(CR.excess(both, exact)) <= 1.0
    for ulps in (1, -1):
        moved = CR.combine(*[CR.simulate(*v, n, exp_ulps=ulps) for v in views])
        assert max(CR.excess(moved, ref)) <= 1.0
    # the scene has what the bounds are for: splats never listed, splats seen in one view only, and deep lists
    assert (ref["pixels"] == 0).sum() > 100 and (ref["pixels"] > 0).sum() > 1000
    assert ((sims[0][2] > 0) != (sims[1][2] > 0)).sum() > 10
    # and the bounds are tight enough to mean something: a few quanta per covered pixel
    seen = ref["pixels"] > 0
    assert (ref["weight_bound"][seen] / ref["pixels"][seen]).max() < 64.0


# ---- teeth -------------------------------------------------------------------------------------------------------------
def test_three_wrong_passes_leave_the_bounds(c1):
    views, sims, ref, n = c1
    one = CR.contrib_reference(views[:1], n)
    assert max(CR.excess(sims[0], one)) <= 1.0
    no_T = CR.simulate(*views[0], n, no_T=True)               # w taken as B without T
    assert np.array_equal(no_T[2], one["pixels"]) and CR.excess(no_T, one)[0] > 1.0
    as_sum = CR.simulate(*views[0], n, peak_sum=True)         # peak accumulated as a sum
    assert CR.excess(as_sum, one)[1] > 1.0 and CR.excess(as_sum, one)[0] <= 1.0
    at_39 = CR.simulate(*views[0], n, q_max=3.9)              # coverage decided at 3.9
    assert not np.array_equal(at_39[2], one["pixels"]) and CR.excess(at_39, one)[0] > 1.0


def test_two_views_in_either_order_give_identical_integers(c1):
    views, sims, ref, n = c1
    ab, ba = CR.combine(sims[0], sims[1]), CR.combine(sims[1], sims[0])
    for x, y in zip(ab, ba):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    r = CR.contrib_reference(views[::-1], n)
    assert np.array_equal(r["pixels"], ref["pixels"])

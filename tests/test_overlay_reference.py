"""The overlay specification (tests/overlay_reference.py) pinned before anything trusts it: a hand-computed pixel, the empty and
the full selection, linearity in mix, the slack of its bounds against f32 runs of the device's recurrence on C1 and their teeth
against a wrong exponential, and the trimmed walk's bits.  No GPU: everything is fed by the oracle."""
import numpy as np
import pytest

import blend_reference as BR
import overlay_reference as OR
from test_oracle_render import make_scene

TINT, MIX = (1.0, 0.5, 0.0), 0.5


def _project(oracle, cam, data, pos, W, H):
    v, p, vp = cam.f32()
    rec, bbox, raw = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
    return rec, bbox, raw, oracle.sort(vp, pos)[0]


@pytest.fixture(scope="module")
def c1(oracle, scenes):
    """C1 at pose 3: the oracle's view, the blend reference, the reference of every second splat and its f32 simulation"""
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H, n = cfg["width"], cfg["height"], cfg["n"]
    _, data, pos = scenes("C1")
    view = _project(oracle, gh.orbit_camera(3, width=W, height=H, fx=cfg["fx"]), data, pos, W, H)
    blend = BR.blend_reference(*view, W, H)
    fb = blend["rgba"].astype(np.float32)
    sel = np.arange(n) % 2 == 0
    ref = OR.overlay_reference(*view, sel, W, H)
    sim = OR.simulate(*view, sel, W, H, fb, TINT, MIX)
    return view, (W, H, n), blend, fb, sel, ref, sim


def test_three_fragments_by_hand(oracle):
    """three co-located splats, front to back: not selected, selected (red), selected (blue)"""
    W = H = 65
    cam, to_world = BR.front_view(W, H)
    splats = (BR.stack(to_world, 32.5, 32.5, 1, 20.0, (10, 200, 30, 128)) + BR.stack(to_world, 32.5, 32.5, 1, 20.0, (255, 0, 0, 128), dz0=0.5) +
              BR.stack(to_world, 32.5, 32.5, 1, 14.0, (0, 0, 255, 200), dz0=1.0))
    rec, bbox, raw, order = _project(oracle, cam, *make_scene(oracle, splats), W, H)
    assert order.tolist() == [0, 1, 2]
    ref = OR.overlay_reference(rec, bbox, raw, order, [False, True, True], W, H)
    q = [BR.coverage_q(rec[i], np.arange(W), np.arange(H)) for i in range(3)]
    B = [np.where(q[i] <= 4, np.exp2(BR.exponent(q[i], rec[i, 6]).astype(np.float64)), 0.0) for i in range(3)]
    w1 = (1.0 - B[0]) * B[1]
    w2 = (1.0 - B[0]) * (1.0 - B[1]) * B[2]
    assert np.allclose(ref["S"], w1 + w2, rtol=1e-13, atol=0) and ref["S"][32, 32] > 0.4
    red, blue = np.float32(255) * (np.float32(1) / np.float32(255)), np.float32(255) * (np.float32(1) / np.float32(255))
    assert np.allclose(ref["C"][..., 0], w1 * float(red), rtol=1e-13, atol=0) and not ref["C"][..., 1].any()
    assert np.allclose(ref["C"][..., 2], w2 * float(blue), rtol=1e-13, atol=0)
    assert np.array_equal(ref["maybe"], (q[1] <= 4) | (q[2] <= 4)) and np.array_equal(ref["sel_kept"], (q[1] <= 4).astype(int) + (q[2] <= 4))
    assert np.array_equal(ref["surely"], ref["maybe"])
    # the overlay is the frame with the two selected splats drawn in lerp(c, tint, mix): compose against the blend of that scene
    fb = BR.blend_reference(rec, bbox, raw, order, W, H)["rgba"]
    want = fb.copy()
    for wk, c in ((w1, (1.0, 0.0, 0.0)), (w2, (0.0, 0.0, 1.0))):
        for ch in range(3):
            want[..., ch] += wk * (MIX * (TINT[ch] - c[ch]))
    assert np.allclose(OR.compose(fb, ref, TINT, MIX), want, rtol=0, atol=1e-14)
    # the one pixel, spelled out
    y = x = 32
    S = (1 - B[0][y, x]) * B[1][y, x] + (1 - B[0][y, x]) * (1 - B[1][y, x]) * B[2][y, x]
    assert abs(ref["S"][y, x] - S) < 1e-15 and 0.0 < ref["S_bound"][y, x] < 1e-5


def test_empty_selection_gives_cover_zero(c1):
    view, (W, H, n), blend, fb, _, _, _ = c1
    ref = OR.overlay_reference(*view, np.zeros(n, bool), W, H)
    assert not ref["S"].any() and not ref["C"].any() and not ref["maybe"].any() and not ref["surely"].any()
    assert np.array_equal(OR.compose(fb, ref, TINT, MIX), fb.astype(np.float64))
    S, out = OR.simulate(*view, np.zeros(n, bool), W, H, fb, TINT, MIX)
    assert not S.any() and np.array_equal(out.view(np.uint32), fb.view(np.uint32))
    assert np.array_equal(ref["T"], blend["T"]) and np.array_equal(ref["kept"], blend["kept"])


def test_full_selection_is_the_frame(c1):
    view, (W, H, n), blend, _, _, _, _ = c1
    ref = OR.overlay_reference(*view, np.ones(n, bool), W, H)
    assert np.abs(ref["S"] - blend["rgba"][..., 3]).max() <= 4e-16 * 64        # S = sum of w; alpha = 1 - T: the same number but for f64 roundings
    assert np.array_equal(ref["C"], blend["rgba"][..., :3])
    assert np.array_equal(ref["maybe"], blend["kept"] > 0)
    # mix = 1 paints every splat with the tint: the colour becomes tint * alpha
    out = OR.compose(blend["rgba"], ref, TINT, 1.0)
    assert np.allclose(out[..., :3], np.asarray(TINT)[None, None, :] * ref["S"][..., None], rtol=0, atol=1e-13)
    assert np.array_equal(out[..., 3], blend["rgba"][..., 3])


def test_linear_in_mix(c1):
    view, (W, H, n), blend, fb, sel, ref, _ = c1
    one = OR.delta(ref, TINT, 1.0)
    assert one.any() and not OR.delta(ref, TINT, 0.0).any()
    for mix in (0.25, 0.5, 0.75):
        assert np.array_equal(OR.delta(ref, TINT, mix), mix * one)
    assert np.allclose(OR.compose(fb, ref, TINT, 0.5), 0.5 * (OR.compose(fb, ref, TINT, 0.0) + OR.compose(fb, ref, TINT, 1.0)), rtol=0, atol=1e-15)
    # without a selected fragment nothing moves, whatever the mix
    assert not one[~ref["maybe"]].any() and (~ref["maybe"]).sum() > 1000 and ref["maybe"].sum() > 1000


def test_bounds_have_slack_and_teeth(c1):
    view, (W, H, n), blend, fb, sel, ref, sim = c1
    assert np.array_equal(ref["surely"], ref["maybe"])                      # C1 has no pixel at which T * B underflows
    assert np.array_equal(sim[0] > 0, ref["maybe"])
    rs, rd = OR.excess(sim[0], sim[1], fb, ref, TINT, MIX)
    assert rs <= 0.5 and rd <= 1.0, (rs, rd)                                 # (delta's last term is one rounding of the result: no slack to have)
    for ulps in (1, -1):
        S, out = OR.simulate(*view, sel, W, H, fb, TINT, MIX, exp_ulps=ulps)
        rs, rd = OR.excess(S, out, fb, ref, TINT, MIX)
        assert rs <= 0.5 and rd <= 1.0, (ulps, rs, rd)
    for ulps in (16, -16):                                                   # an exponential four bits short is outside
        S, out = OR.simulate(*view, sel, W, H, fb, TINT, MIX, exp_ulps=ulps)
        rs, rd = OR.excess(S, out, fb, ref, TINT, MIX)
        assert rs > 1.0 and rd > 1.0, (ulps, rs, rd)
    # a pass that tints a splat too many is outside, a pass that forgets T is outside
    wrong = sel.copy()
    wrong[np.nonzero(~sel)[0][:50]] = True
    S, out = OR.simulate(*view, wrong, W, H, fb, TINT, MIX)
    assert OR.excess(S, out, fb, ref, TINT, MIX)[0] > 1.0 or not np.array_equal(S > 0, ref["maybe"])


def test_the_trimmed_walk_gives_the_same_bits(c1):
    view, (W, H, n), blend, fb, sel, ref, sim = c1
    few = np.zeros(n, bool)
    few[view[3][:40]] = True                                                # the 40 nearest splats: the walk ends early in every list
    a = OR.simulate(*view, few, W, H, fb, TINT, MIX)
    b = OR.simulate(*view, few, W, H, fb, TINT, MIX, stop_after_last=True)
    assert a[0].any() and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    mix0 = OR.simulate(*view, sel, W, H, fb, TINT, 0.0)
    assert np.array_equal(mix0[1].view(np.uint32), fb.view(np.uint32)) and np.array_equal(mix0[0].view(np.uint32), sim[0].view(np.uint32))

"""The colour specification (tests/blend_reference.py) pinned before anything trusts it: its values against three
statements that share no code with it, the slack of its bound against f32 runs of the device's recurrence, its teeth
against three compositors that are subtly wrong, and the scenes of tests/test_gpu_blend.py for what they must contain.
No GPU: everything is fed by the oracle."""
import json
import os

import numpy as np
import pytest

import bin_reference as BIN
import blend_reference as BR
from test_oracle_render import make_scene, overlap_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _project(oracle, cam, data, pos, W, H):
    v, p, vp = cam.f32()
    rec, bbox, raw = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
    return rec, bbox, raw, oracle.sort(vp, pos)[0]


def _built(oracle, cam, splats, W, H):
    return _project(oracle, cam, *make_scene(oracle, splats), W, H)


@pytest.fixture(scope="module")
def c1(oracle, scenes):
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H = cfg["width"], cfg["height"]
    _, data, pos = scenes("C1")
    args = _project(oracle, gh.orbit_camera(3, width=W, height=H, fx=cfg["fx"]), data, pos, W, H)
    return args + (W, H), BR.blend_reference(*args, W, H)


# ---- values ----------------------------------------------------------------------------------------------------------
def test_values_are_the_oracles_mode_1(oracle, c1):
    (rec, bbox, raw, order, W, H), ref = c1
    img = oracle.render(order, raw, rec, bbox, W, H, mode=1).astype(np.float64)
    assert np.abs(img - ref["rgba"]).max() <= 1e-6
    assert BR.excess(img, ref) <= 1.0                       # ... and the oracle lies inside the bound
    assert ref["kept"].max() > 10 and (ref["kept"] == 0).any() and np.all(ref["seen"] <= ref["kept"])
    assert ref["mask"].mean() < 0.01
    # the bound is what the flat tolerance is not: two orders of magnitude under 2e-4 on this frame
    assert ref["bound"].max() < 5e-6
    win = (192, 160, 256, 256)
    sub = BR.blend_reference(rec, bbox, raw, order, W, H, win)
    for k in ("rgba", "bound", "kept", "seen", "mask"):
        assert np.array_equal(sub[k], ref[k][160:416, 192:448]), k


def test_values_are_the_independent_f64_composites(oracle):
    cases, (W, H, fx, fy) = overlap_cases(oracle)
    for case in cases:
        rec, bbox, raw = oracle.project(case["data"], case["view"], case["proj"], fx, fy, W, H)
        order = oracle.sort(case["vp"], case["pos"])[0]
        ref = BR.blend_reference(rec, bbox, raw, order, W, H)
        err = np.abs(ref["rgba"] - case["want"]).max(axis=2)
        err[case["edge"]] = 0.0
        assert err.max() < 1e-4, err.max()
        assert ref["kept"].max() >= 3


def test_values_are_the_executed_shaders_blend_sequences():
    """shader_golden.json's blend_sequences are usable from Python as they stand: u32 bit patterns of (vPosition.xy,
    colour.rgba) per fragment and of the blended destination; the recurrence is fed q and log2(opacity) directly."""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "shader_golden.json")))
    f32 = lambda words: np.array(words, dtype=np.uint32).view(np.float32)
    assert len(g["blend_sequences"]) == 24
    for seq in g["blend_sequences"]:
        px = BR.Pixels(1, 1)
        for words in seq["fragments"]:
            f = f32(words)
            q = BR._fma(f[1], f[1], f[0] * f[0]).reshape(1, 1)
            px.add((slice(0, 1), slice(0, 1)), q, np.log2(f[5].astype(np.float64)).astype(np.float32), f[2:5])
        got = px.result()["rgba"][0, 0]
        assert np.abs(got - f32(seq["dst"]).astype(np.float64)).max() <= 1e-6, (got, f32(seq["dst"]))


def test_rgba8_rounding_is_the_headers():
    src = open(os.path.join(ROOT, "gsplat.js_amd", "csrc", "gsr_internal.h")).read()
    assert "x = fminf(fmaxf(x, 0.0f), 1.0f);" in src and "return (uint32_t)(x * 255.0f + 0.5f);" in src
    x = np.array([-1.0, 0.0, 0.4 / 255, 0.00196, 0.00197, 0.5, 1.0 - 2.0 ** -24, 1.0, 1.5], dtype=np.float32)
    assert BR.to_rgba8(x).tolist() == [0, 0, 0, 0, 1, 128, 255, 255, 255]
    v = np.random.default_rng(3).random(100000).astype(np.float32)
    assert np.abs(BR.to_rgba8(v).astype(np.int64) - np.floor(v.astype(np.float64) * 255.0 + 0.5)).max() <= 1


# ---- slack -----------------------------------------------------------------------------------------------------------
def test_f32_runs_of_the_recurrence_lie_inside_the_bound(c1):
    args, ref = c1
    exact = BR.simulate_f32(*args)
    assert BR.excess(exact, BR.blend_reference(*args, e_exp=0.0)) <= 1.0     # a correctly rounded exponential needs no E_EXP
    for ulps in (1, -1):
        assert BR.excess(BR.simulate_f32(*args, exp_ulps=ulps), ref) <= 1.0
    assert BR.excess(BR.simulate_f32(*args, exp_ulps="random", rng=np.random.default_rng(1)), ref) <= 1.0
    assert np.all(BR.bound_early(ref, 1e-4) == ref["bound"] + 1e-4)


# ---- teeth -----------------------------------------------------------------------------------------------------------
def _directed(oracle):
    """T = 0.14 behind a wide splat, then the faintest splat the format has (alpha 1 / 255: its outer fragments weigh
    e^-4 / 255 = 7e-5 times T, so 1e-5; nothing lighter than 3.6e-5 exists behind T = 0.5), then two splats of different colour"""
    W, H = 64, 64
    cam, to_world = BR.front_view(W, H)
    splats = BR.stack(to_world, 32.0, 32.0, 1, 200.0, (255, 255, 255, 220))
    splats += BR.stack(to_world, 32.0, 32.0, 1, 12.0, (250, 120, 30, 1), dz0=0.5)
    splats += BR.stack(to_world, 30.0, 33.0, 1, 20.0, (255, 0, 0, 60), dz0=1.0)
    splats += BR.stack(to_world, 33.0, 30.0, 1, 20.0, (0, 0, 255, 60), dz0=1.5)
    return _built(oracle, cam, splats, W, H) + (W, H)


def test_the_bound_sees_what_the_flat_tolerance_does_not(oracle):
    args = _directed(oracle)
    rec, bbox, raw, order, W, H = args
    assert order.tolist() == [0, 1, 2, 3]
    ref = BR.blend_reference(*args)
    assert BR.excess(BR.simulate_f32(*args), ref) <= 1.0
    # a fragment of weight 1e-5 removed
    gone = BR.simulate_f32(*args, drop={1})
    d = np.abs(gone.astype(np.float64) - ref["rgba"])
    q1 = BR.coverage_q(rec[1], np.arange(W), np.arange(H))
    T0 = BR.blend_reference(rec, bbox, raw, order[:1], W, H)["T"]
    w1 = np.where(q1 <= 4, T0 * np.exp2(BR.exponent(q1, rec[1, 6]).astype(np.float64)), 0.0)
    rim = (q1 <= 4) & (w1 < 2e-5)                                     # its outer pixels: weight 1e-5 .. 2e-5
    assert rim.sum() > 20 and w1[rim].min() > 9e-6 and 0.1 < T0[rim].min() < T0[rim].max() < 0.2
    assert d[rim].max() < 1e-4                                        # invisible at the flat 2e-4 ...
    assert np.all((d[rim] > ref["bound"][rim]).any(axis=1))           # ... and outside the bound on every one of those pixels
    # two adjacent fragments of different colour swapped
    swapped = (rec, bbox, raw, np.array([0, 1, 3, 2], dtype=order.dtype), W, H)
    assert BR.excess(BR.simulate_f32(*swapped), ref) > 1.0
    # one splat's coverage decided at another threshold: its fragments with 3.9 < q <= 4 flip
    assert ((q1 > 3.9) & (q1 <= 4.0)).any()
    only = (rec, bbox, raw, np.array([1], dtype=order.dtype), W, H)
    flipped = BR.simulate_f32(*only, q_max=3.9)
    assert BR.excess(flipped, BR.blend_reference(*only)) > 1.0
    assert np.abs(flipped - BR.simulate_f32(*only)).max() < 2e-4


# ---- the scenes of the GPU tests ----------------------------------------------------------------------------------------
def test_coverage_scenes_hold_the_cases_a_tight_staging_mask_would_lose(oracle):
    for (W, H, giants) in ((640, 480, False), (322, 241, True)):
        cam, splats = BR.coverage_scene(W, H, [(0, 0, W, H)], seed=5, per_region=1200, giants=giants)
        rec, bbox, raw, order = _built(oracle, cam, splats, W, H)
        assert np.all(rec[raw[:, 11] == 1, 6] <= np.log2(0.5) + 1e-3)             # alpha <= 0.5: T never reaches 0
        assert BR.small_quadrant_pairs(rec, bbox, order, W, H) >= 300
        ref = BR.blend_reference(rec, bbox, raw, order, W, H)
        assert ref["T"].min() > 1e-6
        covered = ref["kept"] > 0
        assert np.array_equal(covered, ref["rgba"][..., 3] > 0)
        if giants:
            assert covered.all()
        else:
            assert 0.1 < covered.mean() < 0.9 and (ref["kept"] == 1).sum() > 10000
        vis = raw[:, 11] == 1
        length = np.maximum(np.hypot(raw[vis, 2], raw[vis, 3]), np.hypot(raw[vis, 4], raw[vis, 5]))
        width = np.minimum(np.hypot(raw[vis, 2], raw[vis, 3]), np.hypot(raw[vis, 4], raw[vis, 5]))
        assert length.max() > 1023.0 and width.min() < 0.5 and (length / width).max() > 1000.0   # needles up to the clamp
        off = vis & ((rec[:, 0] < 0) | (rec[:, 0] > W) | (rec[:, 1] < 0) | (rec[:, 1] > H)) & (bbox[:, 0] <= bbox[:, 2]) & (bbox[:, 1] <= bbox[:, 3])
        assert off.sum() >= 20                                                     # centred off screen, reaching in


@pytest.mark.parametrize("kind", ["grey", "red", "dark", "near", "corner"])
def test_stack_scenes(oracle, kind):
    W, H = BR.STACK_FRAME
    for length in (BR.STACK_LENGTHS if kind == "grey" else (BR.STACK_LENGTH[kind],)):
        cam, splats = BR.stack_scene(kind, length)
        assert len(splats) == length
        rec, bbox, raw, order = _built(oracle, cam, splats, W, H)
        starts, _ = BIN.bin_lists_reference(bbox, order, W, H)
        assert np.diff(starts).tolist() == [length] * 9
        if length > 600 and kind != "grey":
            ref = BR.blend_reference(rec, bbox, raw, order, W, H)
            T = ref["T"]
            if kind in ("red", "dark"):
                assert T[32:64, 32:64].max() < 2.0 ** -150     # the central bin: under the smallest f32, every pixel of it
            elif kind == "near":     # in front of the bright splat T passes 1e-6 inside the frame
                front = BR.blend_reference(rec, bbox, raw, order[:(length - 1) // 2 + 21], W, H)["T"]
                assert front.min() < 1e-6 < front.max() and ((front > 5e-7) & (front < 2e-6)).sum() > 50
            else:                    # the corner pixels of the central bin see the bright splat alone; their quadrants are otherwise saturated
                assert ref["kept"][32, 32] == 1 and ref["kept"][63, 63] == 1 and ref["rgba"][32, 32, 0] > 0.5
                quad = ref["kept"][32:40, 32:40]
                assert (quad == length).sum() == 63 and T[32:40, 32:40].flatten()[1:].max() < 2.0 ** -60   # (2^-27 * colour is the test)


def test_item_scene_fills_its_bins_exactly(oracle):
    W, H = BR.ITEM_FRAME
    cam, splats = BR.item_scene()
    rec, bbox, raw, order = _built(oracle, cam, splats, W, H)
    starts, _ = BIN.bin_lists_reference(bbox, order, W, H)
    assert np.diff(starts).tolist() == list(BR.ITEM_COUNTS) + [0] * (24 - len(BR.ITEM_COUNTS))

"""Registration on the GPU: gsr_register and the pure gsr_rigid_* functions (gsr_match.cpp over k_match.hip) against
tests/register_reference.py bit for bit -- the transform, the status, the number of steps and, with the history, every step's
pairs and rms -- on the noiseless scenario and on the same one with floaters inside the cloud; the result applied to the scene
once and checked against the known partners; the two early ends; and the target left as it was."""
import math

import numpy as np
import pytest

import register_reference as rr

pytestmark = pytest.mark.gpu

W, H = 128, 96
STATUS = {rr.CONVERGED: "converged", rr.MAX_ITERATIONS: "max_iterations", rr.TOO_FEW: "too_few"}
_WANT = {}


def _want(floaters, max_iterations=12):
    if (floaters, max_iterations) not in _WANT:
        src, tgt, _ = rr.scenario(floaters)
        _WANT[(floaters, max_iterations)] = rr.register(src, tgt, rr.RADIUS, None, max_iterations=max_iterations, tolerance=2.0 ** -40)
    return _WANT[(floaters, max_iterations)]


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


@pytest.fixture(scope="module")
def pair(gh):
    a, b = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    yield a, b
    a.dispose()
    b.dispose()


def _arrays(p, seed=1):
    """(data, positions, rotations, scales) around the positions p"""
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    data[:, 0:3] = p.view(np.uint32)
    rot = rng.normal(0, 1, (n, 4)).astype(np.float32)
    scl = rng.uniform(0.01, 0.1, (n, 3)).astype(np.float32)
    return data.reshape(-1), p.reshape(-1), rot.reshape(-1), scl.reshape(-1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def _same(M, info, want, what):
    wM, winfo = want
    print(what, info)
    assert info["status"] == STATUS[winfo["status"]] and info["iterations"] == winfo["iterations"] and info["pairs"] == winfo["pairs"], (what, info, winfo)
    assert np.array_equal(_bits(M), _bits(wM)), (what, M, wM)
    assert _bits([info["rms"]])[0] == _bits([winfo["rms"]])[0] and _bits([info["delta"]])[0] == _bits([winfo["delta"]])[0], (what, info, winfo)
    if "step_pairs" in info:
        assert info["step_pairs"].tolist() == winfo["step_pairs"], what
        assert np.array_equal(_bits(info["step_rms"]), _bits(winfo["step_rms"])), what


@pytest.mark.parametrize("floaters", [False, True], ids=["noiseless", "floaters"])
def test_register_equals_the_reference_bit_for_bit(pair, floaters):
    a, b = pair
    src, tgt, _ = rr.scenario(floaters)
    a.set_scene_arrays(*_arrays(src))
    b.set_scene_arrays(*_arrays(tgt, seed=2))
    want = _want(floaters)
    M, info = a.register(b, rr.RADIUS, max_iterations=12, history=True)
    _same(M, info, want, "history")
    M, info = a.register(b, rr.RADIUS, max_iterations=12)
    assert "step_pairs" not in info
    _same(M, info, want, "no history")
    if not floaters:
        assert info["status"] == "converged" and info["pairs"] == rr.PARTNERS and info["rms"] <= math.sqrt(3.0) * 2.0 ** -23
    # from the result: one more step changes nothing worth a step
    M2, info2 = a.register(b, rr.RADIUS, transform=M, max_iterations=3)
    _same(M2, info2, rr.register(src, tgt, rr.RADIUS, M, max_iterations=3), "restart")
    assert np.array_equal(a.read_scene()[1], src.reshape(-1))          # the scene was never written


def test_rigid_functions_equal_the_reference_bit_for_bit(gh):
    src, tgt, _ = rr.scenario(True)
    M = rr.IDENTITY.copy()
    for step in range(4):
        idx, d2, _ = rr.match(src, tgt, rr.RADIUS, M)
        pairs, s16 = rr.sums(src, tgt, idx, d2, M)
        D, rms = rr.rigid_solve(pairs, s16)
        gD, grms = gh.rigid_solve({"pairs": pairs, "sum": s16})
        assert np.array_equal(_bits(gD), _bits(D)) and _bits([grms])[0] == _bits([rms])[0], step
        M2 = rr.rigid_compose(D, M)
        assert np.array_equal(_bits(gh.rigid_compose(D, M)), _bits(M2)), step
        q, t = rr.rigid_decompose(M2)
        gq, gt = gh.rigid_decompose(M2)
        assert np.array_equal(_bits(gq), _bits(q)) and np.array_equal(_bits(gt), _bits(t)), step
        M = M2
    for angle, axis in ((3.1, (1, 0.01, 0)), (3.1, (0, 1, 0.01)), (3.1, (0.01, 0, 1))):            # Shepperd's other three branches
        R, t = rr.motion(angle, axis, (1.0, -2.0, 0.5))
        Mb = np.concatenate([R, t[:, None]], axis=1)
        q, tt = rr.rigid_decompose(Mb)
        gq, gt = gh.rigid_decompose(Mb)
        assert np.array_equal(_bits(gq), _bits(q)) and np.array_equal(_bits(gt), _bits(tt))
    with pytest.raises(gh.GsplatError):
        gh.rigid_solve({"pairs": 2, "sum": np.zeros(16)})
    bad = np.zeros(16)
    bad[3] = np.nan
    with pytest.raises(gh.GsplatError):
        gh.rigid_solve({"pairs": 9, "sum": bad})


def test_the_result_applied_once_pairs_every_partner(gh, pair):
    a, b = pair
    src, tgt, partner = rr.scenario(False)
    a.set_scene_arrays(*_arrays(src))
    b.set_scene_arrays(*_arrays(tgt, seed=2))
    M, info = a.register(b, rr.RADIUS, max_iterations=12)
    assert info["status"] == "converged"
    q, t = gh.rigid_decompose(M)
    a.scene_rotate(q)
    a.scene_translate(t)
    # Each residual at the fit is at most sqrt(900) times the rms bound sqrt(3) * 2^-23, about 6.2e-6 (one pair cannot carry more
    # than the whole sum of squares); the two f32 stores of rotate and translate add at most sqrt(3) * 2^-22 (half an ulp of a
    # coordinate below 4, per store and axis).  Together below 2^-17 = 7.6e-6, and the target's smallest spacing is above 2^-16
    # (register_reference.scenario asserts it): a match within 2^-17 is THE partner.
    assert math.sqrt(900.0) * math.sqrt(3.0) * 2.0 ** -23 + math.sqrt(3.0) * 2.0 ** -22 < 2.0 ** -17
    idx, d2, _, minfo = a.match(b, 2.0 ** -17)
    print(minfo, float(np.sqrt(d2[:rr.PARTNERS].max())))
    assert np.array_equal(idx[:rr.PARTNERS], partner.astype(np.uint32))
    assert (idx[rr.PARTNERS:] == rr.NONE).all() and minfo["matched"] == rr.PARTNERS


def test_too_few_and_max_iterations(pair):
    a, b = pair
    src, tgt, _ = rr.scenario(False)
    a.set_scene_arrays(*_arrays(src))
    b.set_scene_arrays(*_arrays(tgt, seed=2))
    far = np.array([1.0, 0.0, 0.0, 500.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0])          # a start that matches nothing
    M, info = a.register(b, rr.RADIUS, transform=far, history=True)
    assert info["status"] == "too_few" and info["iterations"] == 1 and info["pairs"] == 0 and info["rms"] == math.inf and info["delta"] == math.inf
    assert np.array_equal(_bits(M), _bits(far)) and info["step_pairs"].tolist() == [0]
    _same(M, info, rr.register(src, tgt, rr.RADIUS, far), "too few")
    M, info = a.register(b, rr.RADIUS, max_iterations=1, history=True)
    assert info["status"] == "max_iterations" and info["iterations"] == 1
    _same(M, info, _want(False, 1), "one step")
    M, info = a.register(b, rr.RADIUS, max_iterations=12, tolerance=0.0)                    # a tolerance of zero is allowed
    _same(M, info, rr.register(src, tgt, rr.RADIUS, None, max_iterations=12, tolerance=0.0), "tolerance 0")


def test_the_target_renders_the_same_frame_before_and_after(gh, pair):
    a, b = pair
    src, tgt, _ = rr.scenario(False)
    a.set_scene_arrays(*_arrays(src))
    b.set_scene_arrays(*_arrays(tgt, seed=2))
    cam = gh.orbit_camera(3, width=W, height=H, fx=120.0)
    sel = np.arange(1500) % 4 == 1
    b.set_selection(sel)

    def frame():
        b.set_camera(cam)
        b._check(b._L.gsr_render(b._ctx))
        return b.lastDepthIndex().copy(), b.readPixelsFloat().copy()

    before = frame()
    a.register(b, rr.RADIUS, max_iterations=4)
    a.match(b, rr.RADIUS, sums=True)
    a.select_match(b, rr.RADIUS, hi=rr.RADIUS)
    assert np.array_equal(b.readPixelsFloat().view(np.uint32), before[1].view(np.uint32))   # the last frame is still there
    after = frame()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1].view(np.uint32), before[1].view(np.uint32))
    assert np.array_equal(b.selection(), sel) and b.hidden_count() == 0
    assert np.array_equal(b.read_scene()[1], tgt.reshape(-1))

"""The specification of SH colour that follows the scene (tests/sh_follow_reference.py), checked against itself without a GPU:
the threshold recount against a brute-force renumbering, the f64 frame against the inverse of the composed map, and the reason
the feature exists -- a scene and a camera moved by the same rigid motion keep their colours, to within the f32 evaluation's own
error, with the frame and do not without it."""
import numpy as np
import pytest

import sh_follow_reference as ref

N = 600
QUAT = (0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214)
QUAT2 = (-0.5, 0.5, 0.5, 0.5)


def _brute_force(band, keep):
    """renumber the kept splats one by one and look where each old threshold's splats went"""
    new_index, k = {}, 0
    for i, kept in enumerate(keep):
        if kept:
            new_index[i] = k
            k += 1
    out = []
    for b in band:
        below = [new_index[i] for i in new_index if i <= b]      # kept splats that were at or below the old threshold
        out.append(max(below) if below else -1)                   # the new threshold is the last of them
    return out


def _masks(n):
    rng = np.random.default_rng(5)
    yield "scattered", rng.random(n) < 0.4
    yield "every splat survives", np.ones(n, dtype=bool)
    yield "nothing survives", np.zeros(n, dtype=bool)
    m = np.zeros(n, dtype=bool)
    m[100:350] = True
    yield "an index range", m


@pytest.mark.parametrize("band", [(-1, -1, -1), (-1, 200, 400), (199, 199, 199), (199, 199, 450), (199, 300, N - 1), (199, N, N + 7),
                                  (N - 1, N - 1, N - 1), (0, 1, 2)])
def test_recount_equals_a_brute_force_renumbering(band):
    for name, keep in _masks(N):
        got = ref.recount_bands(band, keep)
        assert list(got) == _brute_force(band, keep), (name, band)
        tex = [np.arange(8 * (N - (band[0] + 1)), dtype=np.uint32) + np.uint32(ch << 24) for ch in range(3)]
        out, nb, count = ref.compact_sh(tex, band, keep)
        rows = [i for i in range(N) if keep[i] and i > band[0]]
        assert count == len(rows)
        if count:
            assert list(nb) == list(got)
            for ch in range(3):   # row by row: the words of the old row, at the row the renumbering gives the splat
                want = np.concatenate([tex[ch][8 * (i - band[0] - 1):8 * (i - band[0])] for i in rows])
                assert np.array_equal(out[ch], want)
        else:
            assert list(nb) == [-1, -1, -1] and all(t.size == 0 for t in out)


def test_no_sh_splat_survives_clears_the_state():
    keep = np.zeros(N, dtype=bool)
    keep[:200] = True                      # exactly the prefix without SH
    tex = [np.ones(8 * (N - 200), dtype=np.uint32)] * 3
    out, nb, count = ref.compact_sh(tex, (199, 300, 400), keep)
    assert count == 0 and list(nb) == [-1, -1, -1]


def test_frame_is_the_inverse_of_the_composed_map():
    s = (1.25, 0.5, 2.0)                   # condition number 4
    L = ref.frame_after((("rotate", QUAT), ("translate", (1, 2, 3)), ("scale", s), ("rotate", QUAT2)))
    M = ref.rotation_matrix(QUAT2) @ np.diag(s) @ ref.rotation_matrix(QUAT)
    assert np.linalg.cond(M) <= 10
    inv = np.linalg.inv(M)
    assert np.abs(L - inv).max() <= 1e-12 * np.abs(inv).max()
    assert np.array_equal(ref.frame_after(()), ref.IDENTITY)


def _sh_scene(gh):
    rng = np.random.default_rng(17)
    pos = (rng.standard_normal((N, 3)) * 1.5).astype(np.float32)
    band = np.array([99, 249, 399], dtype=np.int32)
    count = N - 100
    tex = []
    for _ in range(3):
        c = rng.standard_normal((count * 8, 2)) * 0.35
        tex.append(np.ascontiguousarray(gh.pack_half2x16(c[:, 0], c[:, 1]), dtype=np.uint32))
    return pos, band, tex


def test_colours_are_invariant_under_a_rigid_motion_of_scene_and_camera(oracle):
    import gsplat_hip as gh
    pos, band, tex = _sh_scene(gh)
    cam = gh.orbit_camera(33, width=640, height=480)
    cam.update(640, 480)
    view = cam.f32()[0]
    sh = np.arange(N) > band[0]
    base = ref.colours(oracle, tex, band, pos, view)
    # the f32 specification's own error: against the same polynomial in f64, no transform anywhere
    own = float(np.abs(base[sh].astype(np.float64) - ref.colours_f64(tex, band, pos, view)[sh]).max())
    assert 0 < own < 1e-5
    bound = 4 * own   # the 3x3 product and the f32 rounding of the rotated positions add a few roundings of the same size
    # the scene rotated as k_scene_rotate rotates it (f64 products, left-to-right sums, f32 stores), the camera with it: V' = V . R^T
    R = ref.rotation_matrix(QUAT)
    p64 = pos.astype(np.float64)
    moved = np.stack([(R[k, 0] * p64[:, 0] + R[k, 1] * p64[:, 1]) + R[k, 2] * p64[:, 2] for k in range(3)], axis=1).astype(np.float32)
    V = np.asarray(view, dtype=np.float32).reshape(4, 4).T.astype(np.float64)      # (column-major in memory)
    Rt = np.eye(4)
    Rt[:3, :3] = R.T
    view2 = np.ascontiguousarray((V @ Rt).T.astype(np.float32).reshape(-1))
    frame = ref.frame_rotate(ref.IDENTITY, QUAT)
    follow = float(np.abs(ref.colours(oracle, tex, band, moved, view2, frame)[sh].astype(np.float64) - base[sh]).max())
    stale = float(np.abs(ref.colours(oracle, tex, band, moved, view2)[sh].astype(np.float64) - base[sh]).max())
    print("f32 specification against f64: %.3g; rotated with the frame: %.3g (bound %.3g); rotated without: %.3g" % (own, follow, bound, stale))
    assert follow <= bound
    assert stale > bound          # the defect: the object turns and its lighting does not
    assert stale > 0.05


def test_identity_frame_is_todays_direction():
    rng = np.random.default_rng(3)
    pos = rng.standard_normal((50, 3)).astype(np.float32)
    view = np.eye(4, dtype=np.float32).reshape(-1)
    view[12:15] = (0.25, -0.5, 4.0)
    a = ref.directions_f32(pos, view)
    assert np.array_equal(a.view(np.uint32), ref.directions_f32(pos, view, ref.IDENTITY).view(np.uint32))
    d = pos - ref.camera_position_f32(view)
    want = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    assert np.array_equal(a.view(np.uint32), want.astype(np.float32).view(np.uint32))

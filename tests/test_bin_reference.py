"""The bin-list reference (tests/bin_reference.py) checked on the CPU, so that a wrong reference is found before it meets a
kernel: against a three-loop brute force on boxes at every edge a bin has, against the oracle's own count of (splat,
tile) pairs at bin granularity, and against the two properties every list has by construction."""
import numpy as np
import pytest

import bin_reference as B


def _random_boxes(rng, n, W, H):
    """n boxes inside W x H: random ones, ones ending exactly on the last pixel of a bin or starting on the first, 1-px
    boxes, boxes on the last (partial) bin row and column, whole-screen boxes; every fifth invisible (x0 > x1 or y0 > y1)."""
    x0 = rng.integers(0, W, n); x1 = np.minimum(x0 + rng.integers(0, 100, n), W - 1)
    y0 = rng.integers(0, H, n); y1 = np.minimum(y0 + rng.integers(0, 100, n), H - 1)
    bb = np.stack([x0, y0, x1, y1], axis=1).astype(np.int32)
    kind = rng.integers(0, 8, n)
    for i in range(n):
        b = bb[i]
        if kind[i] == 0:      # ends on px 31 of a bin, in x and in y
            b[2] = min(b[0] // 32 * 32 + 31 + 32 * int(rng.integers(0, 3)), W - 1)
            b[3] = min(b[1] // 32 * 32 + 31 + 32 * int(rng.integers(0, 3)), H - 1)
        elif kind[i] == 1:    # starts on px 0 of a bin
            b[0] = b[0] // 32 * 32; b[1] = b[1] // 32 * 32
        elif kind[i] == 2:    # one pixel
            b[2] = b[0]; b[3] = b[1]
        elif kind[i] == 3:    # touches the last column and the last row
            b[2] = W - 1; b[3] = H - 1
        elif kind[i] == 4:    # lies inside the last partial bin column / row
            b[0] = (W - 1) // 32 * 32; b[2] = W - 1; b[1] = (H - 1) // 32 * 32; b[3] = H - 1
        elif kind[i] == 5 and i % 3 == 0:
            b[:] = (0, 0, W - 1, H - 1)
    inv = np.arange(n) % 5 == 2
    bb[inv & (np.arange(n) % 2 == 0), 2] = bb[inv & (np.arange(n) % 2 == 0), 0] - 1
    bb[inv & (np.arange(n) % 2 == 1), 3] = bb[inv & (np.arange(n) % 2 == 1), 1] - 1
    return bb


@pytest.mark.parametrize("W,H", [(64, 64), (333, 201), (1000, 712), (97, 33), (32, 31)])
@pytest.mark.parametrize("seed", [1, 2])
def test_reference_equals_the_three_loop_brute_force(W, H, seed):
    rng = np.random.default_rng(seed * 1000 + W)
    n = 400
    bb = _random_boxes(rng, n, W, H)
    di = rng.permutation(n).astype(np.uint32)
    vis = (bb[:, 0] <= bb[:, 2]) & (bb[:, 1] <= bb[:, 3])
    assert 0 < (~vis).sum() < n and (bb[vis, 2] % 32 == 31).sum() > 10 and (bb[vis, 0] % 32 == 0).sum() > 10
    assert (bb[vis, 2] == W - 1).any() and (bb[vis, 3] == H - 1).any() and ((bb[:, 0] == bb[:, 2]) & (bb[:, 1] == bb[:, 3])).any()
    bands = [None, (0, W), (0, 32), (W - 1, W), (31, 33), (40, min(W, 200)), (W // 2, W // 2 + 1), (32, min(64, W))]
    for band in bands:
        ws, wl = B.bin_lists_brute_force(bb, di, W, H, band)
        gs, gl = B.bin_lists_reference(bb, di, W, H, band)
        assert B.first_difference(gs, gl, ws, wl, bb) is None, (band, B.first_difference(gs, gl, ws, wl, bb))
        assert gs.dtype == np.uint32 and gl.dtype == np.uint32 and gs.size == ws.size and gs[-1] == gl.size
        lo, hi, nby = B.bin_grid(W, H, band)
        assert gs.size == (hi - lo) * nby + 1
        # the splats of the lists are the ones the reference counts as entering the context
        assert B.visible_reference(bb, W, H, band) == np.unique(gl).size


def test_edges_of_a_bin_by_hand():
    """Boxes ending on px 31 stay in their bin, boxes starting on px 32 do not reach back, a band's edge cuts a box."""
    bb = np.array([[0, 0, 31, 31], [32, 0, 32, 0], [31, 31, 32, 32], [5, 5, 4, 9], [0, 40, 95, 40], [64, 0, 95, 63]], dtype=np.int32)
    di = np.array([5, 4, 3, 2, 1, 0], dtype=np.uint32)
    starts, lst = B.bin_lists_reference(bb, di, 96, 64)
    lists = [lst[starts[b]:starts[b + 1]].tolist() for b in range(6)]
    assert lists == [[2, 0], [2, 1], [5], [4, 2], [4, 2], [5, 4]]
    starts, lst = B.bin_lists_reference(bb, di, 96, 64, band=(40, 60))     # column 1 only
    assert [lst[starts[b]:starts[b + 1]].tolist() for b in range(2)] == [[2, 1], [4, 2]]
    assert B.visible_reference(bb, 96, 64) == 5 and B.visible_reference(bb, 96, 64, band=(40, 60)) == 3
    starts, lst = B.bin_lists_reference(bb[3:4], np.zeros(1, dtype=np.uint32), 96, 64)
    assert not starts.any() and lst.size == 0
    assert "bin 0:" in B.first_difference(*B.bin_lists_reference(bb, di, 96, 64), *B.bin_lists_reference(bb, di[::-1], 96, 64), bb)


@pytest.mark.parametrize("name,k", [("C1", 3), ("C2", 13)])
def test_total_is_the_oracles_pair_count_at_bin_granularity(oracle, scenes, name, k):
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS[name]
    W, H = cfg["width"], cfg["height"]
    rows, data, pos = scenes(name)
    cam = gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"])
    v, p, vp = cam.f32()
    _, obbox, _ = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
    odi, _, _ = oracle.sort(vp, pos)
    starts, lst = B.bin_lists_reference(obbox, odi, W, H)
    V, D = oracle.tile_stats(obbox, tile=32)
    assert starts[-1] == D == lst.size and B.visible_reference(obbox, W, H) == V > 0
    # every bin's entries are a subsequence of depthIndex: ranks strictly ascending inside a bin
    rank = np.empty(odi.size, dtype=np.int64)
    rank[odi] = np.arange(odi.size)
    rk = rank[lst]
    first_of_bin = np.zeros(rk.size + 1, dtype=bool)
    first_of_bin[starts] = True
    assert np.all((np.diff(rk) > 0) | first_of_bin[1:rk.size])
    # band lists are the full frame's lists of the band's columns
    nbx, nby = -(-W // 32), -(-H // 32)
    for band in [(0, 32), (W // 3 + 5, W // 2 + 7), (W - 40, W)]:
        lo, hi, _ = B.bin_grid(W, H, band)
        bs, bl = B.bin_lists_reference(obbox, odi, W, H, band)
        for row in range(nby):
            for col in range(lo, hi):
                a, b = row * nbx + col, row * (hi - lo) + col - lo
                assert np.array_equal(lst[starts[a]:starts[a + 1]], bl[bs[b]:bs[b + 1]]), (band, row, col)

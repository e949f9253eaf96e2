"""tests/hide_reference.py checked on the CPU: the folds, the word edges, hide_bbox against a filter of the full frame's lists,
compact, and that the H the GPU tests use is neither vacuous nor everything (the seed is fixed HERE, from the oracle's projection)."""
import numpy as np
import pytest

import bin_reference as B
import hide_reference as HR
import select_reference as SR

NAME, POSES = "C1", (3, 40)
W, H = 640, 480
TINY = (1, 31, 32, 33, 1023, 1024, 1025)
BOX = (-1.0, 2.5, -0.75, 3.0, -2.0, 1.0)          # tests/test_gpu_select.py's box: about half of C1
SEED = 5


def test_the_four_folds():
    S = np.array([0, 0, 1, 1], bool)
    P = np.array([0, 1, 0, 1], bool)
    assert HR.fold(S, P, "replace").tolist() == [False, True, False, True]
    assert HR.fold(S, P, "add").tolist() == [False, True, True, True]
    assert HR.fold(S, P, "subtract").tolist() == [False, False, True, False]
    assert HR.fold(S, P, "intersect").tolist() == [False, False, False, True]
    assert HR.OPS == ("replace", "add", "subtract", "intersect")
    # the three calls are that fold with their operands in place
    assert np.array_equal(HR.hide_selected(S, P), S | P) and np.array_equal(HR.hide_selected(S, P, "subtract"), S & ~P)
    assert np.array_equal(HR.hidden_set(S, None), np.zeros(4, bool)) and np.array_equal(HR.hidden_set(S, None, "add"), S)   # NULL: the empty set
    assert np.array_equal(HR.hidden_set(S, P, "intersect"), S & P)
    assert np.array_equal(HR.select_hidden(S, P), P) and np.array_equal(HR.select_hidden(S, P, "add"), S | P)
    out = HR.fold(S, P, "replace")
    out[:] = True
    assert P.tolist() == [False, True, False, True]           # a copy, not a view


@pytest.mark.parametrize("n", TINY)
def test_word_edges(n):
    rng = np.random.default_rng(n)
    Hs = rng.random(n) < 0.5
    Hs[-1] = True                                             # the last splat: the highest live bit
    words = HR.pack(Hs)
    assert words.dtype == np.uint32 and words.size == -(-n // 32)
    assert np.array_equal(HR.unpack(words, n), Hs)
    live = n - 32 * (words.size - 1)
    assert int(words[-1]) >> live == 0 and (int(words[-1]) >> (live - 1)) & 1    # the tail is 0, the last bit where it belongs
    assert sum(bin(int(w)).count("1") for w in words) == int(Hs.sum())
    ones = np.full(words.size + 3, 0xFFFFFFFF, np.uint32)     # host words with every bit set, and more of them than needed
    assert HR.drop_tail(ones, n).all() and HR.drop_tail(ones, n).size == n
    assert np.array_equal(HR.pack(HR.drop_tail(ones, n)), HR.pack(np.ones(n, bool)))
    keep = rng.random(n) < 0.6
    Hc = HR.compact(Hs, keep)
    assert Hc.size == int(keep.sum()) and int(Hc.sum()) == int((Hs & keep).sum())
    new = np.cumsum(keep) - 1                                 # the new index of every kept splat
    for i in np.nonzero(keep)[0][:: max(1, n // 50)]:
        assert Hc[new[i]] == Hs[i]
    assert HR.pack(Hc).size == -(-Hc.size // 32)


def test_hide_bbox():
    bbox = np.array([[0, 0, 5, 5], [1, 1, 0, 0], [10, 10, 40, 40]], np.int32)
    out = HR.hide_bbox(bbox, [True, False, True])
    assert out.tolist() == [[1, 1, 0, 0], [1, 1, 0, 0], [1, 1, 0, 0]] and bbox[0].tolist() == [0, 0, 5, 5]
    assert not SR.listed(out).any()
    assert np.array_equal(HR.hide_bbox(bbox, np.zeros(3, bool)), bbox)


@pytest.fixture(scope="module")
def c1(oracle, scenes):
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS[NAME]
    assert (cfg["width"], cfg["height"]) == (W, H) and cfg["n"] % 32 == 16
    _, data, pos = scenes(NAME)
    views = {}
    for k in POSES:
        cam = gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"])
        v, p, vp = cam.f32()
        rec, bbox, _ = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
        views[k] = (rec, bbox, oracle.sort(vp, pos)[0])
    return cfg["n"], pos, views


def test_the_tests_hidden_set_is_not_vacuous(c1):
    """H removes at least a quarter and at most three quarters of the splats the unhidden frame lists, at both poses; whole bins
    lose everything and other bins mix hidden and listed splats"""
    n, pos, views = c1
    Hs = HR.test_set(n, pos, BOX, SEED)
    assert np.array_equal(Hs, HR.test_set(n, pos, BOX, SEED)) and n // 2 < Hs.sum() < n
    for k in POSES:
        rec, bbox, order = views[k]
        listed = SR.listed(bbox)
        gone = int((listed & Hs).sum())
        print("pose", k, "listed", int(listed.sum()), "of them hidden", gone)
        assert 0.25 * listed.sum() <= gone <= 0.75 * listed.sum(), (k, gone, int(listed.sum()))
        starts, lst = B.bin_lists_reference(bbox, order, W, H)
        hs, hl = B.bin_lists_reference(HR.hide_bbox(bbox, Hs), order, W, H)
        full, left = np.diff(starts.astype(np.int64)), np.diff(hs.astype(np.int64))
        assert ((full > 0) & (left == 0)).any(), (k, "no bin lost everything")
        assert ((left > 0) & (left < full)).sum() > 10, (k, "no bin mixes hidden and listed splats")


@pytest.mark.parametrize("band", [None, (192, 416)], ids=["full", "band"])
def test_hidden_boxes_are_the_full_lists_filtered(c1, band):
    n, pos, views = c1
    Hs = HR.test_set(n, pos, BOX, SEED)
    for k in POSES:
        rec, bbox, order = views[k]
        starts, lst = B.bin_lists_reference(bbox, order, W, H, band)
        want = HR.filter_lists(starts, lst, Hs)
        got = B.bin_lists_reference(HR.hide_bbox(bbox, Hs), order, W, H, band)
        assert B.first_difference(got[0], got[1], want[0], want[1]) is None
        assert 0 < got[1].size < lst.size and not Hs[got[1]].any()
        assert B.visible_reference(HR.hide_bbox(bbox, Hs), W, H, band) == int((SR.listed(bbox, band) & ~Hs).sum())
        assert 0 < HR.tile_entries(HR.hide_bbox(bbox, Hs), W, H, band) < HR.tile_entries(bbox, W, H, band)
    small = np.array([[0, 0, 40, 40], [33, 0, 70, 10], [1, 1, 0, 0], [600, 400, 639, 479]], np.int32)
    order = np.array([3, 1, 0, 2], np.uint32)
    Hs = np.array([False, True, False, False])
    a = B.bin_lists_brute_force(HR.hide_bbox(small, Hs), order, W, H)
    b = HR.filter_lists(*B.bin_lists_brute_force(small, order, W, H), Hs)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and 1 not in a[1].tolist()
    assert HR.tile_entries(small, W, H) == 9 + 3 + 0 + 3 * 5 and HR.tile_entries(HR.hide_bbox(small, Hs), W, H) == 9 + 15


def test_the_python_host_packs_the_same_layout():
    """the host's words are the specification's: what set_hidden sends and hidden() unpacks"""
    import gsplat_hip as gh
    assert callable(gh.HIPRenderer.set_hidden) and callable(gh.HIPRenderer.hidden)
    for n in TINY:
        Hs = np.random.default_rng(n + 1).random(n) < 0.5
        assert np.array_equal(gh.pack_selection(Hs), HR.pack(Hs)) and np.array_equal(gh.unpack_selection(HR.pack(Hs), n), Hs)

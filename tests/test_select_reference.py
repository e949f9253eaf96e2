"""tests/select_reference.py on hand-made cases that separate the definitions: the centre pixel rule on a pixel edge, a centre
off the image whose box is visible, listed or not, band or not, regions with bytes and strides, the ops and the tail bits."""
import numpy as np

import select_reference as SR


def _rec(centres):
    rec = np.zeros((len(centres), 8), dtype=np.float32)
    rec[:, :2] = centres
    return rec


def test_centre_exactly_on_a_pixel_edge_belongs_to_the_pixel_it_starts():
    rec = _rec([(10.0, 5.0), (np.nextafter(np.float32(10.0), np.float32(0)), 5.0), (9.5, 5.999)])
    bbox = np.array([[8, 3, 12, 7]] * 3, dtype=np.int32)
    assert SR.centre_pick(rec, bbox, (10, 5, 11, 6)).tolist() == [True, False, False]      # pixel (10, 5) is [10, 11) x [5, 6)
    assert SR.centre_pick(rec, bbox, (9, 5, 10, 6)).tolist() == [False, True, True]
    assert SR.centre_pick(rec, bbox, (0, 0, 10, 5)).tolist() == [False, False, False]      # x1 and y1 are exclusive


def test_centre_off_the_image_never_selects_though_its_box_is_visible():
    rec = _rec([(-0.5, 4.0), (-0.0, 4.0), (640.0, 4.0), (3.0, float("nan")), (1e20, 4.0)])
    bbox = np.array([[0, 2, 3, 6], [0, 2, 3, 6], [636, 2, 639, 6], [0, 0, 5, 5], [0, 0, 639, 9]], dtype=np.int32)
    whole = (0, 0, 640, 480)
    assert SR.centre_pick(rec, bbox, whole).tolist() == [False, True, False, False, False]  # (-0.0 floors to pixel 0)


def test_listed_means_a_box_and_on_a_band_a_box_that_touches_it():
    rec = _rec([(40.0, 40.0)] * 4)
    bbox = np.array([[30, 30, 50, 50], [1, 30, 0, 50], [30, 1, 50, 0], [10, 30, 31, 50]], dtype=np.int32)
    assert SR.listed(bbox).tolist() == [True, False, False, True]
    assert SR.listed(bbox, band=(32, 64)).tolist() == [True, False, False, False]          # columns 10..31 miss the band [32, 64)
    assert SR.listed(bbox, band=(0, 32)).tolist() == [True, False, False, True]
    assert SR.centre_pick(rec, bbox, (32, 32, 64, 64)).tolist() == [True, False, False, True]
    assert SR.centre_pick(rec, bbox, (32, 32, 64, 64), band=(32, 64)).tolist() == [True, False, False, False]


def test_region_bytes_rows_and_stride():
    rec = _rec([(10.5, 20.5), (11.5, 20.5), (10.5, 21.5), (11.5, 21.5)])
    bbox = np.array([[0, 0, 99, 99]] * 4, dtype=np.int32)
    rect = (10, 20, 12, 22)
    mask = np.array([[0, 7, 1], [1, 0, 1]], dtype=np.uint8)                                  # stride 3: the third byte of a row is padding
    assert SR.centre_pick(rec, bbox, rect, mask).tolist() == [False, True, True, False]
    assert SR.centre_pick(rec, bbox, rect).tolist() == [True] * 4
    index = np.full((30, 30), SR.NONE, dtype=np.uint32)
    index[20, 10], index[20, 11], index[21, 10], index[21, 11], index[22, 11] = 3, 2, 2, 0, 1
    assert SR.hit_pick(index, 4, rect).tolist() == [True, False, True, True]                # splat 1's pixel lies outside
    assert SR.hit_pick(index, 4, rect, mask).tolist() == [False, False, True, False]
    (x0, y0, x1, y1), m = SR.disc(20.0, 20.0, 3.0, stride_pad=5)
    assert (x0, y0, x1, y1) == (17, 17, 23, 23) and m.shape == (6, 11) and np.all(m[:, 6:] == 255)
    assert m[0, 0] == 0 and m[3, 3] == 255 and m[:, :6].sum() // 255 == 32                   # the 6 x 6 square without its corners


def test_ops_packing_and_tail_bits():
    rng = np.random.default_rng(5)
    for n in (1, 31, 32, 33, 1023, 1024, 1025, 10_000):
        S, P = rng.random(n) < 0.5, rng.random(n) < 0.3
        w = SR.pack(S)
        assert w.dtype == np.uint32 and w.size == -(-n // 32)
        assert np.array_equal(SR.unpack(w, n), S)
        assert int(sum(bin(int(v)).count("1") for v in w)) == int(S.sum())
        if n % 32:
            assert int(w[-1]) >> (n % 32) == 0                                               # bits at and above n
            assert int(SR.pack(np.ones(n, bool))[-1]) == (1 << (n % 32)) - 1
        for i in (0, n - 1):
            one = np.zeros(n, bool); one[i] = True
            assert int(SR.pack(one)[i >> 5]) == 1 << (i & 31)
        assert np.array_equal(SR.apply_op(S, P, "replace"), P)
        assert np.array_equal(SR.apply_op(S, P, "add"), S | P)
        assert np.array_equal(SR.apply_op(S, P, "subtract"), S & ~P)
        assert np.array_equal(SR.apply_op(S, P, "intersect"), S & P)
    import gsplat_hip as gh                                                                  # the host's packing is the reference's
    S = rng.random(1025) < 0.5
    assert np.array_equal(gh.pack_selection(S), SR.pack(S)) and np.array_equal(gh.unpack_selection(SR.pack(S), 1025), S)


def test_box_pick_is_inclusive_in_f64_on_f32_positions():
    third = np.float32(0.7)                                                                  # 0.699999988..., below the f64 0.7
    pos = np.array([[third, 0, 0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [np.nan, 0, 0]], dtype=np.float32)
    assert SR.box_pick(pos, (float(third), 1, 0, 1, 0, 1)).tolist() == [True, False, True, False]
    assert SR.box_pick(pos, (0.7, 1, 0, 1, 0, 1)).tolist() == [False, False, True, False]      # the bound is not rounded to f32
    assert SR.box_pick(pos, (0, 1, 0, 1, 0, np.nextafter(1.0, 0.0))).tolist() == [True, True, False, False]


def test_c1_regions_separate_the_definitions(oracle, scenes):
    """On C1 the large regions pick neither nothing nor everything, visible splats with an off-image centre exist, and CENTRE differs
    from 'the box meets the region': an all-zeros, an all-ones or a box-overlap kernel cannot equal this reference."""
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H = cfg["width"], cfg["height"]
    _, data, _ = scenes("C1")
    for k in (3, 40):
        cam = gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"])
        v, p, _ = cam.f32()
        rec, bbox, _ = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
        vis = SR.listed(bbox)
        whole = SR.centre_pick(rec, bbox, (0, 0, W, H))
        assert 0 < whole.sum() < vis.sum() < cfg["n"]                                        # visible, centre off the image
        rect = (200, 150, 330, 270)
        got = SR.centre_pick(rec, bbox, rect)
        overlap = vis & (bbox[:, 0] < rect[2]) & (bbox[:, 2] >= rect[0]) & (bbox[:, 1] < rect[3]) & (bbox[:, 3] >= rect[1])
        assert 0 < got.sum() < overlap.sum() and not np.any(got & ~overlap)
        drect, dmask = SR.disc(317, 243, 70)
        d = SR.centre_pick(rec, bbox, drect, dmask)
        assert 0 < d.sum() < SR.centre_pick(rec, bbox, drect).sum()
        # the centre pixel of a listed splat lies in its own box whenever it lies in the image: it is in exactly one bin's list
        X, Y = np.floor(rec[:, 0]), np.floor(rec[:, 1])
        assert np.all((bbox[whole, 0] <= X[whole]) & (X[whole] <= bbox[whole, 2]) & (bbox[whole, 1] <= Y[whole]) & (Y[whole] <= bbox[whole, 3]))

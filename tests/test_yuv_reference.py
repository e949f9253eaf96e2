"""The Y'CbCr definition itself (tests/yuv_reference.py), on the CPU: the BT.709 bar values, the ranges, neutrality of greys, a
float inverse, edge replication, the background and the layout arithmetic.  tests/test_gpu_yuv_delivery.py holds the device to
this reference byte for byte."""
import numpy as np
import pytest

import yuv_reference as yr


def _flat(rgb, a=255, size=(4, 6)):
    img = np.zeros(size + (4,), dtype=np.uint8)
    img[..., :3] = rgb
    img[..., 3] = a
    return img


# BT.709 limited-range bars at 100 %: Y = 16 + 219 * (kr R + kg G + kb B), Cb = 128 + 224 * (B - Y') / 1.8556, Cr = 128 + 224 * (R - Y') / 1.5748
BARS = {"white": ((255, 255, 255), (235, 128, 128)), "black": ((0, 0, 0), (16, 128, 128)), "red": ((255, 0, 0), (63, 102, 240)),
        "green": ((0, 255, 0), (173, 42, 26)), "blue": ((0, 0, 255), (32, 240, 118))}


@pytest.mark.parametrize("name", sorted(BARS))
def test_limited_range_bars(name):
    rgb, want = BARS[name]
    Y, Cb, Cr = yr.planes(_flat(rgb))
    for plane, w in zip((Y, Cb, Cr), want):
        assert plane.min() == plane.max() and abs(int(plane[0, 0]) - w) <= 1, (name, int(plane[0, 0]), w)
    if name in ("white", "black"):
        assert (int(Y[0, 0]), int(Cb[0, 0]), int(Cr[0, 0])) == want


def test_full_range_spans_all_codes():
    Y, Cb, Cr = yr.planes(_flat((0, 0, 0)), full_range=True)
    assert (Y[0, 0], Cb[0, 0], Cr[0, 0]) == (0, 128, 128)
    Y, Cb, Cr = yr.planes(_flat((255, 255, 255)), full_range=True)
    assert (Y[0, 0], Cb[0, 0], Cr[0, 0]) == (255, 128, 128)
    assert yr.planes(_flat((0, 0, 255)), full_range=True)[1][0, 0] == 255 and yr.planes(_flat((255, 0, 0)), full_range=True)[2][0, 0] == 255
    assert yr.planes(_flat((255, 255, 0)), full_range=True)[1][0, 0] <= 1 and yr.planes(_flat((0, 255, 255)), full_range=True)[2][0, 0] <= 1


@pytest.mark.parametrize("full_range", [False, True])
def test_every_grey_is_neutral(full_range):
    img = np.zeros((2, 512, 4), dtype=np.uint8)
    v = np.repeat(np.arange(256, dtype=np.uint8), 2)
    img[..., 0] = img[..., 1] = img[..., 2] = v
    img[..., 3] = 255
    Y, Cb, Cr = yr.planes(img, full_range)
    assert (Cb == 128).all() and (Cr == 128).all()
    assert (np.diff(Y[0].astype(int)) >= 0).all() and Y.min() == (0 if full_range else 16) and Y.max() == (255 if full_range else 235)
    for row in (yr.LIMITED, yr.FULL):
        assert sum(row[2]) == 0 and sum(row[3]) == 0
    assert sum(yr.FULL[1]) == 256 and sum(yr.LIMITED[1]) == 220


@pytest.mark.parametrize("full_range", [False, True])
def test_float_inverse_recovers_flat_colours(full_range):
    rng = np.random.default_rng(5)
    worst = 0.0
    for rgb in list(rng.integers(0, 256, size=(200, 3))) + [v[0] for v in BARS.values()]:
        Y, Cb, Cr = yr.planes(_flat(tuple(int(c) for c in rgb)), full_range)
        back = np.clip(np.rint(yr.to_rgb_float(Y, Cb, Cr, full_range)), 0, 255)     # what an 8-bit decoder shows
        worst = max(worst, float(np.abs(back - np.asarray(rgb, dtype=np.float64)).max()))
    assert worst <= 2.0, worst


def test_odd_sizes_replicate_the_edge():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, size=(5, 7, 4), dtype=np.uint8)
    img[..., 3] = 255
    padded = np.concatenate([img, img[:, -1:]], axis=1)
    padded = np.concatenate([padded, padded[-1:]], axis=0)
    Y, Cb, Cr = yr.planes(img)
    Yp, Cbp, Crp = yr.planes(padded)
    assert Y.shape == (5, 7) and Cb.shape == (3, 4) and Yp.shape == (6, 8)
    assert np.array_equal(Y, Yp[:5, :7]) and np.array_equal(Cb, Cbp) and np.array_equal(Cr, Crp)
    one = np.array([[[200, 10, 30, 255]]], dtype=np.uint8)
    Y1, Cb1, Cr1 = yr.planes(one)
    Yf, Cbf, Crf = yr.planes(_flat((200, 10, 30)))
    assert Y1.shape == Cb1.shape == (1, 1) and (Y1[0, 0], Cb1[0, 0], Cr1[0, 0]) == (Yf[0, 0], Cbf[0, 0], Crf[0, 0])


def test_background():
    bg = (255, 128, 7)
    clear = _flat((0, 0, 0), a=0)
    assert np.array_equal(yr.over_background(clear, bg)[0, 0], bg)                 # a = 0: the background itself
    solid = _flat((9, 200, 77), a=255)
    assert np.array_equal(yr.over_background(solid, bg)[0, 0], (9, 200, 77))       # a = 255: untouched
    half = _flat((100, 100, 100), a=128)
    assert np.array_equal(yr.over_background(half, bg)[0, 0], (100 + 127, 100 + (127 * 128 + 127) // 255, 100 + (127 * 7 + 127) // 255))
    assert np.array_equal(yr.over_background(_flat((250, 250, 250), a=0), (255, 255, 255))[0, 0], (255, 255, 255))   # never above 255
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(6, 8, 4), dtype=np.uint8)
    assert np.array_equal(yr.over_background(img), img[..., :3])                   # the default adds nothing
    for got, want in zip(yr.planes(clear, background=bg), yr.planes(_flat(bg))):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("W,H", [(1920, 1080), (640, 480), (1001, 713), (33, 17), (1, 1), (2, 1), (1, 2)])
def test_layout(W, H):
    Wc, Hc = (W + 1) // 2, (H + 1) // 2
    nv, i4, rg = yr.layout(W, H, "nv12"), yr.layout(W, H, "i420"), yr.layout(W, H, "rgba8")
    assert nv["bytes"] == i4["bytes"] == W * H + 2 * Wc * Hc and rg["bytes"] == W * H * 4
    assert nv["planes"] == [(0, W, H), (W * H, 2 * Wc, Hc)]
    assert i4["planes"] == [(0, W, H), (W * H, Wc, Hc), (W * H + Wc * Hc, Wc, Hc)]
    for lay in (nv, i4, rg):
        assert lay["trailer"] % 4 == 0 and 0 <= lay["trailer"] - lay["bytes"] < 4
        end = 0
        for off, stride, rows in lay["planes"]:
            assert off == end                                                      # tightly packed
            end = off + stride * rows
        assert end == lay["bytes"]
    if W % 2 == 0 and H % 2 == 0:
        assert nv["bytes"] * 2 == W * H * 3                                        # 1.5 bytes per pixel
    rng = np.random.default_rng(W + H)
    img = rng.integers(0, 256, size=(min(H, 40), min(W, 50), 4), dtype=np.uint8)
    h, w = img.shape[:2]
    a, b = yr.payload(img, "nv12"), yr.payload(img, "i420")
    assert a.size == b.size == yr.layout(w, h, "nv12")["bytes"] and np.array_equal(a[:w * h], b[:w * h])
    n = ((w + 1) // 2) * ((h + 1) // 2)
    assert np.array_equal(a[w * h::2], b[w * h:w * h + n]) and np.array_equal(a[w * h + 1::2], b[w * h + n:])

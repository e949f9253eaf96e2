"""Splat data, the part that is pure arithmetic: the histogram's edge rule of include/gsplat_hip.h as tests/attr_reference.py states
it, on seeded data with values planted exactly on every edge and one ulp to either side -- the edges are nondecreasing and end at
hi, what the histogram shows is what a range selects for every pair of edges, the counters add up to the count, and the planted
values are where a plain floor((v - lo) / w) goes wrong, so the rule is shown to matter."""
import numpy as np
import pytest

import attr_reference as ar

BINS = (1, 2, 7, 64, 257, 4096)
RANGES = ((0.1, 1.3), (-3.7, 11.9), (0.0, 255.0), (1e-3, 1e-3 * (1 + 2.0 ** -40)))   # the last: a few thousand ulps wide, edges repeat


def _planted(lo, hi, bins, seed=5):
    e = ar.edges(lo, hi, bins)
    rng = np.random.default_rng(seed + bins)
    span = hi - lo
    v = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), rng.uniform(lo - 0.25 * span, hi + 0.25 * span, 4000),
                        [np.nan, np.inf, -np.inf, -0.0, 0.0, lo, hi]])
    return rng.permutation(v), e


@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("bins", BINS)
def test_edges_are_nondecreasing_and_end_at_hi(lo, hi, bins):
    e = ar.edges(lo, hi, bins)
    assert e.size == bins + 1 and e[0] == lo and e[bins] == hi
    assert np.all(np.diff(e) >= 0)
    w = (np.float64(hi) - np.float64(lo)) / np.float64(bins)
    for k in (0, bins // 2, bins - 1):
        assert e[k] == min(np.float64(lo) + np.float64(k) * w, np.float64(hi))


@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("bins", BINS)
def test_what_the_histogram_shows_is_what_the_range_selects(lo, hi, bins):
    v, e = _planted(lo, hi, bins)
    counts, outside = ar.histogram(v, lo, hi, bins)
    count, nan, _, _ = ar.stats(v)
    assert int(counts.sum()) + sum(outside) == count == v.size and outside[2] == nan
    cum = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    # gsr_select_attr(edge(a), edge(b)) on every splat, counted: the values v with edge(a) <= v < edge(b)
    if bins <= 64:
        for a in range(bins):
            for b in range(a + 1, bins + 1):
                assert int(ar.select(v, e[a], e[b]).sum()) == cum[b] - cum[a], (a, b)
    else:
        # the same count for ALL pairs at once: sorted, the values below a bound are a prefix, so select(edge(a), edge(b)) counts
        # below[b] - below[a] (edge(a) <= edge(b)); checked against select() itself on a sample of pairs
        s = np.sort(v[~np.isnan(v)])
        below = np.searchsorted(s, e, side="left")
        sel = below[None, :] - below[:, None] if bins <= 257 else None
        rng = np.random.default_rng(bins)
        for a, b in [(0, bins), (0, 1), (bins - 1, bins)] + [tuple(sorted(rng.choice(bins + 1, 2, replace=False))) for _ in range(40)]:
            assert int(ar.select(v, e[a], e[b]).sum()) == below[b] - below[a]
        if sel is not None:
            want = cum[None, :] - cum[:, None]
            iu = np.triu_indices(bins + 1, 1)
            assert np.array_equal(sel[iu], want[iu])
        else:
            assert np.array_equal(below - below[0], cum)   # every (a, b) is the difference of two of these


def test_a_plain_floor_disagrees_on_the_planted_values():
    bites = 0
    for lo, hi in RANGES:
        for bins in BINS:
            v, e = _planted(lo, hi, bins)
            inside = v[ar.select(v, lo, hi)]
            w = (np.float64(hi) - np.float64(lo)) / np.float64(bins)
            naive = np.minimum(np.floor((inside - lo) / w), bins - 1).astype(np.int64)
            rule = np.searchsorted(e[:bins], inside, side="right") - 1
            assert np.all(e[rule] <= inside) and np.all((rule == bins - 1) | (e[np.minimum(rule + 1, bins)] > inside))
            bites += int((naive != rule).sum())
    assert bites > 0, "floor((v - lo) / w) agrees everywhere: the planted values do not test the rule"


def test_scope_nan_and_scale_extremes():
    data = np.zeros(8 * 5, dtype=np.uint32)
    data[7::8] = [0x01020304, 0xff000000, 0x00ff0000, 0x0000ff00, 0x800000ff]
    assert ar.attr_value("red", data=data).tolist() == [4, 0, 0, 0, 255]
    assert ar.attr_value("opacity", data=data).tolist() == [1, 255, 0, 0, 128]
    scl = np.array([1, 2, 3, np.nan, 1, 1, -0.0, 0.0, 5, np.inf, 1, 2, -np.inf, 0, 1], dtype=np.float32)
    mn, mx = ar.attr_value("scale_min", scales=scl), ar.attr_value("scale_max", scales=scl)
    assert mn[0] == 1 and mx[0] == 3 and np.isnan(mn[1]) and np.isnan(mx[1]) and mn[2] == 0 and mx[2] == 5 and mx[3] == np.inf and mn[4] == -np.inf
    sel, hid = ar.pack([1, 1, 0, 0, 1]), ar.pack([0, 1, 0, 0, 0])
    assert ar.in_scope(5, 3, sel, hid).tolist() == [True, False, False, False, True]
    assert ar.in_scope(5, 1, None, hid).tolist() == [False] * 5 and ar.in_scope(5, 2, sel, None).tolist() == [True] * 5
    assert ar.stats(mn) == (5, 1, -np.inf, 1.0) and ar.stats(mn, np.zeros(5, bool)) == (0, 0, np.inf, -np.inf)

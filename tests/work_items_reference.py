"""What a frame's compositor WORK LIST must be: a plain numpy statement of the finalize step of the binning stage, written from
its specification and not from the kernel (bin_finalize_body, k_bin.hip), so that a device build is
compared with the operation and never with another device build.  Inputs are the oracle's only (oracle.project, oracle.sort,
bin_reference.bin_lists_reference) and the compositor plan (pinned by tests/test_blend_plan.py); no device read-back is one.

    The frame's figures are sums over the splats whose pixel box is not empty and, in a band context, meets the band's
    pixels [32 lo, 32 hi) (lo, hi: the band's bin columns):
        V       their number
        D       sum of nt, the 16x16 tiles of the box: columns clipped to the band's 2 lo .. 2 hi - 1, rows not clipped
        otiles  sum of (op8 min(nt, 4096)) >> 4, op8 the opacity byte (data word 7 >> 24)
        omass   sum of (op8 trunc(area)) >> 8, area = min(0.77f sqrt(m2 n2), 65535) in f32, m2 / n2 the squared lengths of
                the splat's axes (raw[:, 2:6]).  In a band context the footprint is NOT clipped to the band.
    Every f32 operation but the square root is reproducible (no contraction); the device's square root is documented to 1 ulp,
    that is within 1.5 ulp of the correctly rounded root s.  So omass is an INTERVAL: trunc(area) at s - 2 ulp and at
    s + 2 ulp, summed to [omass_lo, omass_hi]; the device's sum must lie in it.

    The cut: E = min(sum of the bins' entries, 2^32 - 1), mass = omass 256 // 255,
        dense      otiles 4096 >= long_tau 255 npix  and  2 D >= long_tiles_x2 V
        heavy      mass >= long_mass_min E
        long_from  2^32 - 1 for the whole-bin sentinel or long_policy 0;  0 for long_policy > 0;  otherwise, when mass > 0 and
                   (dense or heavy or long_tau_bin): min(0xfffffff0, ceil(tb 1024 E / mass)), tb = long_tau_bin or 8 if dense else 60
        seg_len    min(max(E // seg_target_items // 256 * 256, seg_min), max(8192, seg_min)); the sentinel passes through
        a bin of c entries: nf = 0 if c >= long_from else min(c // seg_len, 63) full segments, r = c - nf seg_len, and a last
        segment iff r > 0 or nf == 0 (an empty bin is one item).
    bin_start / seg_start are the exclusive scans (totals in element nbins); fits = entries <= capacity and items <= max_items;
    a frame that does not fit publishes no items and all starts zero.  Items are (bin | seg << 16, first, end, seg_start[bin] |
    nseg << 25).  by_size = plan.items_by_size or mxbin >= long_from: then the items' classes -- partial_class(seg_len) for a
    full segment, partial_class(r) for a last one -- never increase along the list, in any order inside a class; otherwise the
    list is every full segment in raster order (bin, then segment) and then every last segment in raster order."""
import numpy as np

BIN_PX = 32
TILE = 16
FIN_LAYERS = 64                   # segments per bin at most
SEG_LEN_MAX = 8192
WHOLE_BIN_FROM = 1 << 30          # a minimum segment length from here on is the whole-bin sentinel
U32_MAX = 0xffffffff
LONG_FROM_MAX = 0xfffffff0
SQRT_ULPS = 2                     # 1.5 ulp of the correctly rounded root (1 ulp documented for the instruction), rounded up


def partial_class(r):
    """size class of r entries: r below 4; from there four classes per power of two, 63 at most (from 65536 on)"""
    r = np.asarray(r, dtype=np.int64)
    e = np.floor(np.log2(np.maximum(r, 1).astype(np.float64))).astype(np.int64)      # exact: r < 2^53
    e = np.where((np.int64(1) << e) > r, e - 1, e)                                     # (and guarded all the same)
    big = np.minimum(63, (e - 1) * 4 + ((r >> np.maximum(e - 2, 0)) & 3))
    return np.where(r < 4, r, big)


def _steps(s, k):
    """s moved k f32 steps up (k > 0) or down, not below zero"""
    to = np.float32(np.inf) if k > 0 else np.float32(0.0)
    for _ in range(abs(k)):
        s = np.nextafter(s, to, dtype=np.float32)
    return s


def frame_figures(data, obbox, raw, W, H, band=None):
    """dict(V, D, otiles, omass_lo, omass_hi, uncertain): the frame's figures; `uncertain` counts the splats whose trunc(area)
    differs between the interval's ends"""
    nbx = -(-W // BIN_PX)
    lo, hi = (0, nbx) if band is None else (band[0] // BIN_PX, min((band[1] + BIN_PX - 1) // BIN_PX, nbx))
    bb = np.asarray(obbox, dtype=np.int64).reshape(-1, 4)
    x0, y0, x1, y1 = bb[:, 0], bb[:, 1], bb[:, 2], bb[:, 3]
    vis = (x0 <= x1) & (y0 <= y1) & ~((x1 < lo * BIN_PX) | (x0 >= hi * BIN_PX))
    x0, y0, x1, y1 = x0[vis], y0[vis], x1[vis], y1[vis]
    cols = np.minimum(x1 // TILE, hi * 2 - 1) - np.maximum(x0 // TILE, lo * 2) + 1
    nt = cols * (y1 // TILE - y0 // TILE + 1)
    op8 = (np.asarray(data, dtype=np.uint32).reshape(-1, 8)[:, 7] >> 24).astype(np.int64)[vis]
    ax = np.asarray(raw, dtype=np.float32).reshape(-1, 12)[:, 2:6][vis]
    f = np.float32
    m2 = ax[:, 0] * ax[:, 0] + ax[:, 1] * ax[:, 1]            # f32, one operation at a time
    n2 = ax[:, 2] * ax[:, 2] + ax[:, 3] * ax[:, 3]
    s = np.sqrt(m2 * n2, dtype=np.float32)                    # correctly rounded
    assert m2.dtype == np.float32 and s.dtype == np.float32 and np.all(np.isfinite(s))

    def area(root):
        return np.minimum(f(0.77) * root, f(65535.0)).astype(np.int64)      # truncation of a non-negative f32

    a_lo, a_hi = area(_steps(s, -SQRT_ULPS)), area(_steps(s, SQRT_ULPS))
    return dict(V=int(vis.sum()), D=int(nt.sum()), otiles=int(((op8 * np.minimum(nt, 4096)) >> 4).sum()),
                omass_lo=int(((op8 * a_lo) >> 8).sum()), omass_hi=int(((op8 * a_hi) >> 8).sum()), uncertain=int((a_lo != a_hi).sum()))


def _field(plan, name):
    return int(plan[name])


def cut(counts, figures, plan, capacity):
    """The cut of the bins' entry counts under `figures` (V, D, otiles, omass: one value, not the interval) and the plan: a dict of
    E, mxbin, mass, dense, heavy, long_from, seg_len, by_size, fits, n_items, bin_start, seg_start (as published: zero when the frame
    does not fit), entries / items_needed, and the expected items in raster order with their classes (items, classes, is_last)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    nbins = c.size
    V, D, otiles, omass = (int(figures[k]) for k in ("V", "D", "otiles", "omass"))
    seg_min = _field(plan, "seg_len")
    whole = seg_min >= WHOLE_BIN_FROM
    entries = int(c.sum())
    E = min(entries, U32_MAX)
    mxbin = int(c.max()) if nbins else 0
    mass = omass * 256 // 255
    dense = otiles * 4096 >= _field(plan, "long_tau") * 255 * _field(plan, "npix") and 2 * D >= _field(plan, "long_tiles_x2") * V
    heavy = mass >= _field(plan, "long_mass_min") * E
    policy, tau_bin = _field(plan, "long_policy"), _field(plan, "long_tau_bin")
    long_from = U32_MAX
    if not whole:
        if policy > 0:
            long_from = 0
        elif policy < 0 and mass > 0 and (dense or heavy or tau_bin):
            tb = tau_bin if tau_bin else 8 if dense else 60
            long_from = min(LONG_FROM_MAX, -(-(tb * 1024 * E) // mass))
    seg_len = seg_min
    if not whole:
        seg_len = min(max(E // _field(plan, "seg_target_items") // 256 * 256, seg_min), max(SEG_LEN_MAX, seg_min))
    by_size = bool(_field(plan, "items_by_size")) or mxbin >= long_from
    nf = np.where(c >= long_from, 0, np.minimum(c // seg_len, FIN_LAYERS - 1))
    r = c - nf * seg_len
    part = (r > 0) | (nf == 0)
    nseg = nf + part
    bin_start = np.zeros(nbins + 1, dtype=np.int64)
    seg_start = np.zeros(nbins + 1, dtype=np.int64)
    np.cumsum(c, out=bin_start[1:])
    np.cumsum(nseg, out=seg_start[1:])
    n_items = int(seg_start[-1])
    fits = entries <= int(capacity) and n_items <= _field(plan, "max_items")
    # the expected items, raster order: bin, then segment
    b = np.repeat(np.arange(nbins, dtype=np.int64), nseg)
    k = np.arange(n_items, dtype=np.int64) - seg_start[b]
    last_of_bin = k + 1 == nseg[b]
    first = bin_start[b] + k * seg_len
    end = np.where(last_of_bin, bin_start[b] + c[b], bin_start[b] + (k + 1) * seg_len)
    items = np.stack([b | (k << 16), first, end, seg_start[b] | (nseg[b] << 25)], axis=1)
    is_last = k == nf[b]                      # the bin's last segment (a full segment k < nf is not one, even when it ends the bin)
    classes = np.where(is_last, partial_class(r[b]), partial_class(seg_len))
    assert items.size == 0 or items.max() <= U32_MAX
    if not fits:
        bin_start[:] = 0
        seg_start[:] = 0
    return dict(E=E, mxbin=mxbin, mass=mass, dense=bool(dense), heavy=bool(heavy), long_from=int(long_from), seg_len=int(seg_len), by_size=by_size,
                fits=bool(fits), n_items=n_items if fits else 0, items_needed=n_items, entries=entries, bin_start=bin_start.astype(np.uint32),
                seg_start=seg_start.astype(np.uint32), nf=nf, r=r, nseg=nseg, items=items.astype(np.uint32), classes=classes, is_last=is_last,
                whole_bins=0 if whole else int((c >= long_from).sum()), cut_bins=int((nseg > 1).sum()))


def cut_interval(counts, figures, plan, capacity):
    """cut() at both ends of the optical mass interval: (at omass_lo, at omass_hi)"""
    return tuple(cut(counts, dict(figures, omass=figures[k]), plan, capacity) for k in ("omass_lo", "omass_hi"))


def input_condition(counts, at_lo, at_hi):
    """None when the interval of the optical mass decides nothing -- `heavy` agrees at both ends and no bin's count lies between
    the two long_from -- else a sentence.  A condition on a test's inputs, computed on the CPU."""
    c = np.asarray(counts, dtype=np.int64)
    a, b = sorted((at_lo["long_from"], at_hi["long_from"]))
    if at_lo["heavy"] != at_hi["heavy"]:
        return "heavy differs between the ends of the optical mass interval"
    n = int(((c >= a) & (c < b)).sum())
    return None if n == 0 else "%d bins hold between %d and %d entries: the optical mass interval decides their cut" % (n, a, b)


def expected_sequence(want):
    """the items in the order the list must have without by_size: the full segments in raster order, then the last segments"""
    return np.concatenate([want["items"][~want["is_last"]], want["items"][want["is_last"]]])


def _rows_sorted(a):
    a = np.asarray(a, dtype=np.uint32).reshape(-1, 4)
    return a[np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]


def item_invariants(items, nbins, capacity, max_items):
    """What the compositor relies on of every item, from the items alone: None, or a sentence naming the first item that breaks it"""
    it = np.asarray(items, dtype=np.int64).reshape(-1, 4)
    b, seg, slot0, nseg = it[:, 0] & 0xffff, it[:, 0] >> 16, it[:, 3] & ((1 << 25) - 1), it[:, 3] >> 25
    for name, bad in (("bin < nbins", b >= nbins), ("seg < nseg <= 64", (seg >= nseg) | (nseg > FIN_LAYERS)),
                      ("first <= end <= capacity", (it[:, 1] > it[:, 2]) | (it[:, 2] > capacity)), ("slot0 + nseg <= max_items", slot0 + nseg > max_items)):
        if bad.any():
            i = int(np.argmax(bad))
            return "item %d %r breaks %s" % (i, it[i].tolist(), name)
    # one (slot0, nseg) per bin, and the bins' slot ranges disjoint
    ub, at = np.unique(b, return_index=True)
    if not (np.array_equal(slot0, slot0[at][np.searchsorted(ub, b)]) and np.array_equal(nseg, nseg[at][np.searchsorted(ub, b)])):
        return "the items of one bin disagree on its partial slots"
    o = np.argsort(slot0[at], kind="stable")
    s, n = slot0[at][o], nseg[at][o]
    over = s[1:] < s[:-1] + n[:-1]
    if over.any():
        i = int(np.argmax(over))
        return "bins %d and %d share partial slots (%d + %d, %d)" % (ub[o][i], ub[o][i + 1], s[i], n[i], s[i + 1])
    return None


def check_work_list(items, seg_start, want, nbins, capacity, max_items):
    """The device's list against cut()'s answer `want`: None, or a sentence naming what differs."""
    it = np.asarray(items, dtype=np.uint32).reshape(-1, 4)
    if it.shape[0] != want["n_items"]:
        return "%d items instead of %d" % (it.shape[0], want["n_items"])
    if not np.array_equal(np.asarray(seg_start, dtype=np.uint32), want["seg_start"]):
        return "seg_start differs, first at bin %d" % int(np.argmax(np.asarray(seg_start) != want["seg_start"]))
    if not want["fits"]:
        return None
    bad = item_invariants(it, nbins, capacity, max_items)
    if bad:
        return bad
    got_s, want_s = _rows_sorted(it), _rows_sorted(want["items"])
    if not np.array_equal(got_s, want_s):
        i = int(np.argmax((got_s != want_s).any(axis=1)))
        return "the item set differs: expected %r, got %r" % (want_s[i].tolist(), got_s[i].tolist())
    if want["by_size"]:
        o = np.argsort(want["items"][:, 0], kind="stable")                    # word 0 names an item
        cls = want["classes"][o][np.searchsorted(want["items"][:, 0][o], it[:, 0])]
        up = np.diff(cls) > 0
        if up.any():
            i = int(np.argmax(up))
            return "heaviest first: item %d of class %d stands in front of item %d of class %d" % (i, cls[i], i + 1, cls[i + 1])
    else:
        seq = expected_sequence(want)
        if not np.array_equal(it, seq):
            i = int(np.argmax((it != seq).any(axis=1)))
            return "raster order: item %d is %r, expected %r" % (i, it[i].tolist(), seq[i].tolist())
    return None


def canonical(items):
    """the list with the items of every run of one class sorted by their first word: what two contexts must agree on"""
    it = np.asarray(items, dtype=np.uint32).reshape(-1, 4)
    if not it.shape[0]:
        return it
    cls = partial_class(it[:, 2].astype(np.int64) - it[:, 1].astype(np.int64))
    run = np.concatenate([[0], np.cumsum(np.diff(cls) != 0)])
    return it[np.lexsort((it[:, 0], run))]

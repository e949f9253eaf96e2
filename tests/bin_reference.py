"""What a frame's bin lists must BE: a plain numpy statement of the binning stage, written from its specification and not
from the kernels (k_bin.hip), so that a device build is compared with the operation and never with another device build.

    Bins are 32 x 32 px, nbx = ceil(W / 32), nby = ceil(H / 32), row-major.  A context with the band [x0, x1) owns the bin
    columns x0 // 32 .. (x1 + 31) // 32 - 1 (no further than nbx - 1), numbered from 0 inside the band.  A splat with the
    inclusive pixel box (bx0, by0, bx1, by1) -- oracle.project's bbox; invisible when bx0 > bx1 or by0 > by1 -- enters
    every owned bin whose column lies in bx0 // 32 .. bx1 // 32 and whose row lies in by0 // 32 .. by1 // 32.  Bin b's list
    is those splats' indices in the order of depthIndex.  starts is the exclusive scan of the list lengths, starts[nbins]
    the total.

Vectorised: the (splat, bin) pairs are expanded in depth order, then sorted by bin with a stable sort (a radix sort when
the bin numbers fit 16 bits, which they do up to the largest framebuffer, 256 x 256 bins)."""
import numpy as np

BIN_PX = 32


def bin_grid(W, H, band=None):
    """(first owned bin column, one past the last, bin rows) of a context"""
    nbx, nby = -(-W // BIN_PX), -(-H // BIN_PX)
    if band is None:
        return 0, nbx, nby
    return band[0] // BIN_PX, min((band[1] + BIN_PX - 1) // BIN_PX, nbx), nby


def _rects(obbox, W, H, band):
    """per splat (in index order): first / last owned column relative to the band, first / last row, and whether it enters a bin"""
    lo, hi, nby = bin_grid(W, H, band)
    bb = np.asarray(obbox, dtype=np.int64).reshape(-1, 4)
    visible = (bb[:, 0] <= bb[:, 2]) & (bb[:, 1] <= bb[:, 3])
    cx0 = np.maximum(bb[:, 0] // BIN_PX, lo) - lo
    cx1 = np.minimum(bb[:, 2] // BIN_PX, hi - 1) - lo
    ry0, ry1 = bb[:, 1] // BIN_PX, bb[:, 3] // BIN_PX
    enters = visible & (cx0 <= cx1) & (ry0 <= ry1)
    return cx0, cx1, ry0, ry1, enters, hi - lo, nby


def visible_reference(obbox, W, H, band=None):
    """How many splats enter at least one of the context's bins (a full-frame context: the visible ones)."""
    return int(_rects(obbox, W, H, band)[4].sum())


def bin_lists_reference(obbox, depth_index, W, H, band=None):
    """(starts uint32[nbins + 1], list uint32[total]) of the context (W, H, band) for the boxes obbox[n, 4] and the order depth_index[n]."""
    cx0, cx1, ry0, ry1, enters, w, nby = _rects(obbox, W, H, band)
    nbins = max(w, 0) * nby
    di = np.asarray(depth_index, dtype=np.int64).reshape(-1)
    di = di[enters[di]]                                  # the splats that enter a bin, front to back
    bw = cx1[di] - cx0[di] + 1
    cnt = bw * (ry1[di] - ry0[di] + 1)
    total = int(cnt.sum())
    first = np.cumsum(cnt) - cnt
    owner = np.repeat(np.arange(di.size), cnt)           # pair -> its splat's place in the depth order (ascending)
    k = np.arange(total, dtype=np.int64) - first[owner]  # pair -> its number inside the splat's rectangle, row-major
    s, ow = di[owner], bw[owner]
    b = (ry0[s] + k // ow) * w + cx0[s] + k % ow
    assert total == 0 or (0 <= b.min() and b.max() < nbins)
    b = b.astype(np.uint16 if nbins <= 65536 else np.int64)
    order = np.argsort(b, kind="stable")                 # by bin; inside a bin the depth order stays
    starts = np.zeros(nbins + 1, dtype=np.int64)
    np.cumsum(np.bincount(b, minlength=nbins), out=starts[1:])
    assert starts[-1] == total < 2 ** 32
    return starts.astype(np.uint32), s[order].astype(np.uint32)


def bin_lists_brute_force(obbox, depth_index, W, H, band=None):
    """The same specification as three loops (splats front to back, rows, columns); for small inputs."""
    lo, hi, nby = bin_grid(W, H, band)
    w = hi - lo
    lists = [[] for _ in range(w * nby)]
    for i in depth_index:
        x0, y0, x1, y1 = (int(v) for v in obbox[int(i)])
        if x0 > x1 or y0 > y1:
            continue
        for row in range(y0 // BIN_PX, y1 // BIN_PX + 1):
            for col in range(x0 // BIN_PX, x1 // BIN_PX + 1):
                if lo <= col < hi:
                    lists[row * w + (col - lo)].append(int(i))
    starts = np.zeros(w * nby + 1, dtype=np.uint32)
    starts[1:] = np.cumsum([len(entries) for entries in lists])
    return starts, np.array([i for entries in lists for i in entries], dtype=np.uint32)


def first_difference(starts, lst, want_starts, want_list, obbox=None):
    """None when the lists are equal, else a sentence naming the first bin that differs, its expected and actual entries
    and the box of the first splat that is missing, extra or out of place."""
    starts, want_starts = np.asarray(starts, dtype=np.int64), np.asarray(want_starts, dtype=np.int64)
    if starts.shape != want_starts.shape:
        return "bins: %d instead of %d" % (starts.size - 1, want_starts.size - 1)
    if np.array_equal(starts, want_starts) and np.array_equal(lst, want_list):
        return None
    for b in range(starts.size - 1):
        got, want = lst[starts[b]:starts[b + 1]], want_list[want_starts[b]:want_starts[b + 1]]
        if starts[b] != want_starts[b] or not np.array_equal(got, want):
            m = min(got.size, want.size)
            at = int(np.argmax(got[:m] != want[:m])) if m and (got[:m] != want[:m]).any() else m
            splat = int(want[at]) if at < want.size else int(got[at])
            box = None if obbox is None else [int(v) for v in np.asarray(obbox).reshape(-1, 4)[splat]]
            return ("bin %d: start %d (expected %d), %d entries (expected %d); first difference at entry %d: expected %s, got %s; "
                    "splat %d has the box %s" % (b, starts[b], want_starts[b], got.size, want.size, at, want[max(at - 2, 0):at + 3].tolist(),
                                                 got[max(at - 2, 0):at + 3].tolist(), splat, box))
    return "totals differ: %d instead of %d" % (starts[-1], want_starts[-1])

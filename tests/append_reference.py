"""The exact specification of growing the scene (include/gsplat_hip.h, "growing the scene"), over oracle.SceneState.  No arithmetic
anywhere: rows are gathered with integer indices and concatenated, so every word keeps its bits (NaN payloads and -0.0 included).

    duplicate(state, sel)            rows idx = flatnonzero(sel), ascending, copied behind the last row: row n + j = row idx[j]
    append_selected(state, src, sel) the same with the rows read from `src` (sel over src's splats)
    append_arrays(state, ...)        the rows as they are behind the last row
    each returns (first, count) and leaves the state in place with n + count splats; rows [0, n) keep their bits.
    selection_after(n, first, count) the selection afterwards: exactly the new rows
    hidden_after(H, count)           the hidden set afterwards: the old bits and a clear tail
    contrib_after(arrays, count)     the accumulators afterwards: the old rows' values and zeros
    capacity_after(capacity, need)   the capacity rule: unchanged while need fits, else max(need, capacity + capacity // 2), capped
    erase(state, sel)                the rows where sel is false, in order (gsr_scene_erase_selected): the inverse used by the tests"""
import numpy as np

import edit_reference as er

MAX_ROWS = 0x7fffffff // 8      # the upload's limit
FIELDS = (("data", 8), ("positions", 3), ("rotations", 4), ("scales", 3))


def _extend(state, sub):
    first = state.n
    for name, k in FIELDS:
        old = getattr(state, name)[:k * state.n]
        setattr(state, name, np.concatenate([old, getattr(sub, name)[:k * sub.n].astype(old.dtype, copy=False)]))
    state.n = first + sub.n
    return first, sub.n


def duplicate(state, sel):
    return append_selected(state, state, sel)


def append_selected(state, src, sel):
    sel = np.asarray(sel, dtype=bool).reshape(-1)
    assert sel.size == src.n
    return _extend(state, er.sub_state(src, np.flatnonzero(sel)))


def append_arrays(state, data, positions, rotations, scales):
    sub = er.sub_state(state, np.zeros(0, dtype=np.int64))
    sub.positions = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1)
    sub.n = sub.positions.size // 3
    sub.data = np.ascontiguousarray(data, dtype=np.uint32).reshape(-1)[:8 * sub.n]
    sub.rotations = np.ascontiguousarray(rotations, dtype=np.float32).reshape(-1)
    sub.scales = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
    assert sub.data.size == 8 * sub.n and sub.rotations.size == 4 * sub.n and sub.scales.size == 3 * sub.n
    return _extend(state, sub)


def selection_after(n, first, count):
    i = np.arange(n)
    return (i >= first) & (i < first + count)


def hidden_after(hidden, count):
    return np.concatenate([np.asarray(hidden, dtype=bool).reshape(-1), np.zeros(count, dtype=bool)])


def contrib_after(arrays, count):
    return tuple(np.concatenate([a, np.zeros(count, dtype=a.dtype)]) for a in arrays)


def capacity_after(capacity, need):
    return capacity if need <= capacity else min(max(need, capacity + capacity // 2), MAX_ROWS)


def erase(state, sel):
    sel = np.asarray(sel, dtype=bool).reshape(-1)
    assert sel.size == state.n
    keep = er.sub_state(state, np.flatnonzero(~sel))
    for name, _ in FIELDS:
        setattr(state, name, getattr(keep, name))
    state.n = keep.n
    return state.n

"""The exact specification of editing the selection (include/gsplat_hip.h, "editing the selection"): the selected splats, transformed
as a Scene holding only them would be.  No new arithmetic: the selected rows of an oracle.SceneState are gathered into a sub-state,
the oracle's own translate / rotate / scale (the reference's loops, src/core/Scene.ts:182-305) run on it, and the rows are scattered
back.  A pivot is the three-step sequence on that sub-state: translate(-pivot), the operation, translate(+pivot)."""
import numpy as np

from oracle import oracle as O


def sub_state(state, idx):
    """A SceneState holding only the rows `idx` of `state` (copies)."""
    idx = np.asarray(idx, dtype=np.int64)
    sub = O.SceneState(np.zeros(0, dtype=np.uint8))
    sub.n = int(idx.size)
    sub.data = np.ascontiguousarray(state.data[:8 * state.n].reshape(-1, 8)[idx]).reshape(-1)
    sub.positions = np.ascontiguousarray(state.positions.reshape(-1, 3)[idx]).reshape(-1)
    sub.rotations = np.ascontiguousarray(state.rotations.reshape(-1, 4)[idx]).reshape(-1)
    sub.scales = np.ascontiguousarray(state.scales.reshape(-1, 3)[idx]).reshape(-1)
    return sub


def apply(state, sel, op, args, pivot=None):
    """state.<op>(args) on the splats where sel is true, in place; every other row keeps its bits.  op: "translate", "rotate", "scale"."""
    assert op in ("translate", "rotate", "scale")
    sel = np.asarray(sel, dtype=bool).reshape(-1)
    assert sel.size == state.n
    idx = np.flatnonzero(sel)
    if not idx.size:
        return state
    sub = sub_state(state, idx)
    if pivot is not None:
        p = np.asarray(pivot, dtype=np.float64).reshape(3)
        sub.translate(-p)
    getattr(sub, op)(args)
    if pivot is not None:
        sub.translate(p)
    state.data[:8 * state.n].reshape(-1, 8)[idx] = sub.data.reshape(-1, 8)
    state.positions.reshape(-1, 3)[idx] = sub.positions.reshape(-1, 3)
    state.rotations.reshape(-1, 4)[idx] = sub.rotations.reshape(-1, 4)
    state.scales.reshape(-1, 3)[idx] = sub.scales.reshape(-1, 3)
    return state


def paint(state, sel, rgba, byte_mask):
    """data[8i + 7] = (data[8i + 7] & ~byte_mask) | (rgba & byte_mask) for the selected i, in place."""
    sel = np.asarray(sel, dtype=bool).reshape(-1)
    assert sel.size == state.n
    word = state.data[:8 * state.n].reshape(-1, 8)[:, 7]
    m = np.uint32(byte_mask & 0xffffffff)
    word[sel] = (word[sel] & ~m) | (np.uint32(rgba & 0xffffffff) & m)
    return state


def bounds(positions, sel):
    """(count, min f32[3], max f32[3]) of the selected centres.  A value enters min only through x < min and max only through
    x > max: a NaN is counted and never enters the box; nothing selected is (0, +inf, -inf)."""
    pos = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    sel = np.asarray(sel, dtype=bool).reshape(-1)
    assert sel.size == pos.shape[0]
    p = pos[sel]
    with np.errstate(invalid="ignore"):
        mn = np.where(np.isnan(p), np.float32(np.inf), p).min(axis=0, initial=np.float32(np.inf)).astype(np.float32)
        mx = np.where(np.isnan(p), np.float32(-np.inf), p).max(axis=0, initial=np.float32(-np.inf)).astype(np.float32)
    return int(p.shape[0]), mn, mx

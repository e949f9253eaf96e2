"""Hidden splats, the specification in numpy ("Hidden splats").

    The hidden set H is one bit per splat, in the selection's layout (select_reference.pack).  The four calls fold sets:
        gsr_hide_selected   H = H op S          gsr_hidden_set   H = H op P (P the host's)
        gsr_select_hidden   S = S op H          gsr_read_hidden  H
    with op REPLACE A = B, ADD A |= B, SUBTRACT A &= ~B, INTERSECT A &= B.
    The frame: a hidden splat fails the culls as if its pixel box were empty.  With bbox the ORACLE's boxes of the whole scene,
    hide_bbox(bbox, H) gives every member of H the invisible box; every specification the project has (bin_reference,
    blend_reference, depth_reference, select_reference, contrib_reference, overlay_reference) then describes the hidden frame
    unchanged, fed with those boxes and the UNCHANGED depth order (a hidden splat is still sorted).
    A compaction that keeps the splats of `keep`, in order, carries H along: compact(H, keep) = H[keep]."""
import numpy as np

import select_reference as SR

OPS = SR.OPS
INVISIBLE = (1, 1, 0, 0)          # the box of a culled splat, x0 > x1 (oracle.c: ORC_INVISIBLE; k_project.hip: BBOX_INVISIBLE_*)
pack, unpack = SR.pack, SR.unpack


def fold(A, B, op):
    """A op B on bool arrays: the one fold all three calls use"""
    return SR.apply_op(A, B, op)


def hide_selected(H, S, op="add"):
    return fold(H, S, op)


def hidden_set(H, P, op="replace"):
    """P: bool[n], or None for the empty set"""
    H = np.asarray(H, dtype=bool)
    return fold(H, np.zeros(H.size, bool) if P is None else P, op)


def select_hidden(S, H, op="replace"):
    return fold(S, H, op)


def drop_tail(words, n):
    """host words -> the set they name: bits at and above n are dropped, words behind ceil(n / 32) ignored"""
    w = np.asarray(words, dtype=np.uint32).reshape(-1)[:-(-n // 32)]
    return unpack(w, n) if n else np.zeros(0, bool)


def hide_bbox(bbox, H):
    """the boxes of the hidden frame: a copy of bbox[n, 4] with the invisible box at every member of H"""
    out = np.array(bbox, dtype=np.int32).reshape(-1, 4)
    out[np.asarray(H, dtype=bool)] = INVISIBLE
    return out


def compact(H, keep):
    """H after a compaction that keeps the splats of `keep` in order: H'[new index of i] = H[i]"""
    H, keep = np.asarray(H, dtype=bool), np.asarray(keep, dtype=bool)
    assert H.shape == keep.shape
    return H[keep]


def filter_lists(starts, lst, H):
    """bin lists with the entries that are members of H taken out, order kept: (starts, list)"""
    starts = np.asarray(starts, dtype=np.int64)
    lst = np.asarray(lst, dtype=np.uint32)
    stay = ~np.asarray(H, dtype=bool)[lst]
    before = np.concatenate([[0], np.cumsum(stay)])
    return before[starts].astype(np.uint32), lst[stay]


def tile_entries(bbox, W, H, band=None):
    """gsr_timings.tile_entries: the 16 x 16 tiles the listed splats' boxes overlap, inside the context's bin columns (band: whole bins)"""
    bb = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)
    lo = 0 if band is None else band[0] // 32
    hi = -(-W // 32) if band is None else min((band[1] + 31) // 32, -(-W // 32))
    vis = SR.listed(bb, band)
    tx0, tx1 = np.maximum(bb[:, 0] // 16, lo * 2), np.minimum(bb[:, 2] // 16, hi * 2 - 1)
    return int(((tx1 - tx0 + 1) * (bb[:, 3] // 16 - bb[:, 1] // 16 + 1))[vis].sum())


def test_set(n, positions, box, seed):
    """the H of the tests: a seeded random half of the splats, united with the splats inside `box`"""
    rng = np.random.default_rng(seed)
    return (rng.random(n) < 0.5) | SR.box_pick(positions, box)


test_set.__test__ = False

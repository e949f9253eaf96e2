"""The compositor plan (plan_blend, k_blend.hip) asked directly: no context, no device.

plan_blend is the one function that picks the compositor's kernel (one or two waves per 16x16 tile, the fold of a bin's
segments fused or separate), its persistent grid and the work-item policy k_bin_finalize is handed; alloc_bins sizes the work
items, the partials and the arrival masks from its answer, launch_bin and launch_blend launch by it.  gsr_debug_blend_plan hands
that answer out for the bins and pixels of a band, a list capacity, a CU count, the kind of context, early termination, the
work items already allocated and the nine knobs.  The tests assert properties of the answers, not a second copy of the function,
over band grids of 1 .. 65536 bins (4096 is the last that takes two waves per tile), both kinds of context, early termination
on and off, every knob unset and set, list capacities from the ABI's minimum to its maximum, 0 / 1 / 256 CUs, and an item table
that is sized afresh or already larger than the need.
"""
import ctypes
import itertools

import numpy as np
import pytest

FIELDS = ("waves_per_tile", "fused", "separate_fold", "whole_bin", "threads", "grid", "queue_start", "seg_len", "seg_target_items",
          "max_items", "partial_slots", "items_by_size", "long_policy", "seg_len_long", "long_tau", "long_tiles_x2", "long_tau_bin",
          "long_mass_min", "npix", "saturate")
PLAN = np.dtype([(f, np.int32 if f in ("items_by_size", "long_policy") else np.uint32) for f in FIELDS])
INPUTS = ("nbins", "npix", "capacity", "cus", "throughput", "early_out", "allocated", "fuse_combine", "saturate", "items_by_size",
          "long_items", "long_tau", "blend_sub", "seg_target", "blend_grid", "seg_len")
UNSET = dict(fuse_combine=1, saturate=1, items_by_size=-1, long_items=-1, long_tau=0, blend_sub=0, seg_target=0, blend_grid=0, seg_len=0)
WHOLE_BIN_FROM = 1 << 30          # is_whole_bin (gsr_internal.h): a minimum length from here on means one work item per bin
NBINS = (1, 2, 32, 2040, 4095, 4096, 4097, 8160, 65536)     # (2040: 1080p, 8160: 4K)
CAPACITIES = (1024,) + tuple(max(6 * n + (1 << 20), 1 << 22) for n in (0, 4000, 1_000_000, 5_000_000)) + (0xfffffff0,)
ABOVE_ANY_NEED = 1 << 25          # > 65536 + 0xfffffff0 / 256 + 16


def default_capacity(n):
    """the list a context allocates for a new scene of n splats (alloc_bins)"""
    return max(6 * n + (1 << 20), 1 << 22)


def bind(L):
    fn = L.gsr_debug_blend_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_int,
                   ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    return fn


def plan_of(L, **inputs):
    """the plan of one set of inputs (knobs not named are unset)"""
    args = dict(UNSET, cus=256, throughput=0, early_out=0, allocated=0)
    args.update(inputs)
    out = np.zeros(1, dtype=PLAN)
    assert bind(L)(*[int(args[k]) for k in INPUTS], out.ctypes.data) == PLAN.itemsize
    return out[0]


@pytest.fixture(scope="module")
def ask():
    import gsplat_hip
    fn = bind(gsplat_hip.load_library())

    def plans(rows):
        """rows: dicts of INPUTS -> (inputs as a dict of int64 arrays, plans as one structured array)"""
        out = np.zeros(len(rows), dtype=PLAN)
        at = out.ctypes.data
        for i, r in enumerate(rows):
            assert fn(*[r[k] for k in INPUTS], at + i * PLAN.itemsize) == PLAN.itemsize
        return {k: np.array([r[k] for r in rows], dtype=np.int64) for k in INPUTS}, out

    return plans


def _rows(axes):
    names = list(axes)
    return [dict(zip(names, v)) for v in itertools.product(*axes.values())]


def _check(i, p):
    """every property the issue of the plan states, over the rows of one sweep"""
    f = {k: p[k].astype(np.int64) for k in FIELDS}
    thr, early = i["throughput"] != 0, i["early_out"] != 0
    # a pinned knob always wins
    for knob, field in (("blend_sub", "waves_per_tile"), ("seg_target", "seg_target_items"), ("blend_grid", "grid")):
        pinned = i[knob] != 0
        assert np.all(f[field][pinned] == i[knob][pinned]), knob
    pinned = (i["seg_len"] != 0) & ~early
    assert np.all(f["seg_len"][pinned] == i["seg_len"][pinned])
    pinned = i["items_by_size"] >= 0
    assert np.all(f["items_by_size"][pinned] == i["items_by_size"][pinned])
    pinned = (i["long_items"] >= 0) & ~early
    assert np.all(f["long_policy"][pinned] == i["long_items"][pinned])
    assert np.all(f["long_tau_bin"] == i["long_tau"]) and np.all(f["fused"] == i["fuse_combine"]) and np.all(f["saturate"] == i["saturate"])
    assert np.all(f["npix"] == i["npix"])
    # waves per tile: unpinned, two iff one frame at a time and at most 4096 bins
    free = i["blend_sub"] == 0
    assert np.all((f["waves_per_tile"][free] == 2) == (~thr[free] & (i["nbins"][free] <= 4096)))
    two = f["waves_per_tile"] == 2
    assert np.all(two | (f["waves_per_tile"] == 1))
    # threads and grid
    assert np.all(f["threads"] == 256 * f["waves_per_tile"])
    free = i["blend_grid"] == 0
    assert np.all(f["grid"][free] == np.where(two, 3, 7)[free] * np.maximum(i["cus"], 1)[free])      # (7 per CU in either kind of context)
    free = (i["seg_len"] == 0) & ~early
    assert np.all(f["seg_len"][free & two] >= 1024) and np.all(f["seg_len"][free & ~two] == 512)
    # early termination: whole bins, whatever GSR_SEG_LEN says
    assert np.all(f["whole_bin"] == early)
    assert np.all(f["seg_len"][early] >= WHOLE_BIN_FROM) and np.unique(f["seg_len"][early]).size <= 1 and np.all(f["long_policy"][early] == 0)
    assert np.all(f["partial_slots"][early] == 0) and np.all(f["separate_fold"][early] == 0)
    # otherwise: segments of whole 256-entry chunks
    assert np.all(f["seg_len"][~early] % 256 == 0) and np.all(f["seg_len"][~early] >= 256) and np.all(f["seg_len"][~early] < WHOLE_BIN_FROM)
    assert np.all(f["partial_slots"][~early] == f["max_items"][~early])
    free = (i["long_items"] < 0) & ~early
    assert np.all(f["long_policy"][free] == np.where(i["saturate"][free] != 0, -1, 0))
    # items
    need = i["nbins"] + i["capacity"] // f["seg_len"] + 16
    assert np.all(f["max_items"] >= need) and np.all(f["max_items"] >= i["allocated"])
    assert np.all(f["max_items"][i["allocated"] == 0] == need[i["allocated"] == 0])       # sized afresh: exactly the need
    assert np.all(f["max_items"][i["allocated"] >= need] == i["allocated"][i["allocated"] >= need])
    assert np.all(f["queue_start"] == np.minimum(f["max_items"], f["grid"]))
    # fold
    assert np.all(f["separate_fold"] == ((f["fused"] == 0) & (f["whole_bin"] == 0)))
    # the per-kind figures of DESIGN.md section 3
    assert np.all(f["long_tau"] == np.where(thr, 120, 340)) and np.all(f["long_tiles_x2"] == np.where(thr, 6, 9))
    assert np.all(f["long_mass_min"] == np.where(thr, 0, 12)) and np.all(f["seg_len_long"] == 32768)
    free = i["seg_target"] == 0
    assert np.all(f["seg_target_items"][free] == np.where(thr, 1300, 5000)[free])
    free = i["items_by_size"] < 0
    assert np.all(f["items_by_size"][free] == np.where(thr, 0, 1)[free])


def test_every_knob_unset_and_set(ask):
    rows = _rows(dict(nbins=(1, 2040, 4096, 4097, 65536), npix=(1920 * 1080,), capacity=(default_capacity(700_000),), cus=(256,), throughput=(0, 1),
                      early_out=(0, 1), allocated=(0,), fuse_combine=(1, 0), saturate=(1, 0), items_by_size=(-1, 0, 1), long_items=(-1, 0, 1), long_tau=(0, 40),
                      blend_sub=(0, 1, 2), seg_target=(0, 777), blend_grid=(0, 3), seg_len=(0, 256, 2048)))
    _check(*ask(rows))


def test_every_size(ask):
    rows = _rows(dict(nbins=NBINS, npix=(32 * 32, 8192 * 8192), capacity=CAPACITIES, cus=(0, 1, 256), throughput=(0, 1), early_out=(0, 1),
                      allocated=(0, ABOVE_ANY_NEED), fuse_combine=(1,), saturate=(1,), items_by_size=(-1,), long_items=(-1,), long_tau=(0,),
                      blend_sub=(0, 1, 2), seg_target=(0,), blend_grid=(0, 3), seg_len=(0, 256, 2048)))
    _check(*ask(rows))


def test_an_item_table_only_grows(ask):
    """allocated items below the need are raised to it, above it kept: the table is never shrunk by a plan that is not sized afresh"""
    need = 2040 + default_capacity(700_000) // 1024 + 16
    rows = _rows(dict(nbins=(2040,), npix=(1920 * 1080,), capacity=(default_capacity(700_000),), cus=(256,), throughput=(0,), early_out=(0,),
                      allocated=(1, need - 1, need, need + 1), **{k: (v,) for k, v in UNSET.items()}))
    i, p = ask(rows)
    assert list(p["max_items"]) == [need, need, need, need + 1]
    _check(i, p)

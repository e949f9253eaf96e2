"""The binning plan (plan_bins, k_bin.hip) asked directly: no context, no device.

plan_bins is the one function that picks the binning stage's form and sizes its grids, LDS and tables; alloc_bins
allocates by its answer and launch_bin launches by it.  gsr_debug_bin_plan hands that answer out for a grid of bins, a
splat count, a list capacity, a CU count, a front-end width and the knobs.  The tests here assert properties of the
answers, not a second copy of the function:

  * every case of tests/test_gpu_bin_lists.py whose id names a form gets that form (the case list is imported);
  * over every grid of 1..256 x 1..256 bins -- a band enters the plan only as its width in bin columns, so this is every
    framebuffer and every band the ABI accepts --, both front-end widths (the kind of context, or GSR_FRONT_WAVES), every
    value of GSR_BIN_TWO_LEVEL and GSR_BIN_BIG and list capacities on both sides of 2^30: what a wrong plan would break.
"""
import ctypes
import re

import numpy as np
import pytest

import bin_reference as B
import test_gpu_bin_lists as cases

FORMS = ("finalize only", "fused wide", "fused narrow", "separate finalize", "large grid", "two level")
FINALIZE_ONLY, FUSED_WIDE, FUSED_NARROW, SEPARATE_FINALIZE, LARGE_GRID, TWO_LEVEL = range(6)
FIELDS = ("form", "nbins", "groups", "steps_per_wave", "rounds", "blocks", "sx", "sy", "w", "h", "count_slices", "count_rows",
          "count_lds", "scatter_lds", "extra_wg", "table_rows", "table_cols", "ncx", "ncy", "ncells", "cell_grid", "chunks")
PLAN = np.dtype([(f, np.int32 if f in ("nbins", "sx", "sy", "w", "h", "ncx", "ncy", "ncells") else np.uint32) for f in FIELDS])
SCAT_LDS_BUDGET = 150 * 1024      # what set_scatter_lds_attribute raises the scatter kernels to (+ 1 KiB static)
COUNT_LDS_MAX = 48 * 1024         # k_bin_count's counters, per row slice
WIDE, NARROW = 16, 8
CUS = 256


@pytest.fixture(scope="module")
def ask():
    import gsplat_hip
    fn = gsplat_hip.load_library().gsr_debug_bin_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_uint,
                   ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_uint, ctypes.c_void_p]

    def plans(grids, n, capacity, front_waves, two_level=-1, big=2, rounds=0, cell_grid=0):
        """the plans of `grids` ((nbxb, nby) pairs) as one structured array"""
        out = np.zeros(len(grids), dtype=PLAN)
        at = out.ctypes.data
        for i, (w, h) in enumerate(grids):
            assert fn(w, h, n, capacity, CUS, front_waves, two_level, big, rounds, cell_grid, at + i * PLAN.itemsize) == PLAN.itemsize
        return out

    return plans


def _default_capacity(n):
    return max(6 * n + (1 << 20), 1 << 22)


def _named(id):
    """what a case id of test_gpu_bin_lists.py says about the plan: {field: value}, 'one_level': True"""
    want = {}
    if "two level" in id:
        want["form"] = TWO_LEVEL
        m = re.search(r"k_cell_scatter1<(\d)>", id)
        if m:
            want["groups"] = int(m.group(1))
    elif "k_bin_scatter_narrow<8>" in id:
        want.update(form=FUSED_NARROW, groups=8, steps_per_wave=4)
    elif re.search(r"k_bin_scatter<(\d),true>", id):
        want.update(form=FUSED_WIDE, groups=int(re.search(r"k_bin_scatter<(\d),true>", id).group(1)), steps_per_wave=2)
    elif "k_bin_scatter<4,false>" in id:
        want.update(form=SEPARATE_FINALIZE, groups=4, steps_per_wave=2)
    elif re.search(r"k_bin_scatter_big<4,(\d)>", id):
        want.update(form=LARGE_GRID, groups=4, steps_per_wave=int(re.search(r"k_bin_scatter_big<4,(\d)>", id).group(1)))
    elif "one level" in id:
        want["one_level"] = True
        if "4 groups" in id:
            want["groups"] = 4
    m = re.search(r"(\d+) rounds?\b", id)
    if m:
        want["rounds"] = int(m.group(1))
    m = re.search(r"sliced (\d)x(\d)", id)
    if m:
        want.update(sx=int(m.group(1)), sy=int(m.group(2)))
    m = re.search(r"(\d) count slices", id)
    if m:
        want["count_slices"] = int(m.group(1))
    return want


def _form_cases():
    out = []
    for prm in cases.FORMS + cases.BOUNDS_FORMS:
        if _named(prm.id):
            out.append(pytest.param(prm.id, *prm.values, id=prm.id))
    return out


def test_most_case_ids_name_a_form():
    assert len(_form_cases()) >= len(cases.FORMS) + len(cases.BOUNDS_FORMS) - 4      # (all but the bands of one bin column at 1080p and the like)
    assert {_named(p.values[0]).get("form") for p in _form_cases()} >= {FUSED_WIDE, FUSED_NARROW, SEPARATE_FINALIZE, LARGE_GRID, TWO_LEVEL}


@pytest.mark.parametrize("id,scene,size,env,throughput,band", _form_cases())
def test_case_gets_the_form_its_id_names(ask, id, scene, size, env, throughput, band):
    import gsplat_hip
    lo, hi, nby = B.bin_grid(size[0], size[1], band)
    n = gsplat_hip.synth.CONFIGS[scene]["n"] if scene in gsplat_hip.synth.CONFIGS else {"mid": 60000, "big": 30000}[scene]   # (_scene_of)
    front = int(env.get("GSR_FRONT_WAVES", NARROW if throughput else WIDE))
    p = ask([(hi - lo, nby)], n, _default_capacity(n), front, int(env.get("GSR_BIN_TWO_LEVEL", -1)), int(env.get("GSR_BIN_BIG", 2)),
            int(env.get("GSR_BIN_ROUNDS", 0)))[0]
    want = _named(id)
    if want.pop("one_level", False):
        assert p["form"] in (FUSED_WIDE, FUSED_NARROW, SEPARATE_FINALIZE, LARGE_GRID), FORMS[p["form"]]
    for field, value in want.items():
        assert p[field] == value, (field, FORMS[p["form"]], p)
    assert p["nbins"] == (hi - lo) * nby


GRIDS = [(w, h) for h in range(1, 257) for w in range(1, 257)]


@pytest.mark.parametrize("capacity", [1 << 22, (1 << 30) - 1, 1 << 30, 0xfffffff0], ids=["4M", "2^30-1", "2^30", "max"])
@pytest.mark.parametrize("big", [0, 1, 2])
@pytest.mark.parametrize("two_level", [-1, 0, 1])
@pytest.mark.parametrize("front", [WIDE, NARROW])
def test_every_grid(ask, front, two_level, big, capacity):
    n = 700000
    p = ask(GRIDS, n, capacity, front, two_level, big)
    w, h = np.array(GRIDS, dtype=np.int64).T
    nbins = w * h
    form, groups = p["form"], p["groups"]
    one_level = (form >= FUSED_WIDE) & (form <= LARGE_GRID)
    two = form == TWO_LEVEL
    assert np.all(one_level | two) and np.all(p["nbins"] == nbins)
    # above 4096 bins no one-level sub-grid fits 8 groups beside a second workgroup: k_bin_scatter<8, false> and
    # k_bin_scatter_big<8, 2> would never be launched, so they do not exist
    assert np.all(groups[one_level & (nbins > 4096)] == 4)
    assert np.all((groups == 4) | (groups == 8))
    assert np.all(np.isin(form[nbins > 4096], (SEPARATE_FINALIZE, LARGE_GRID, TWO_LEVEL)))
    assert np.all(np.isin(form[nbins <= 4096], (FUSED_WIDE, FUSED_NARROW, TWO_LEVEL)))
    assert not np.any(form == (SEPARATE_FINALIZE if big else LARGE_GRID))
    # LDS
    assert np.all(p["scatter_lds"] <= SCAT_LDS_BUDGET) and np.all(p["scatter_lds"] > 0)
    assert np.all(p["count_lds"] <= COUNT_LDS_MAX)
    # the scatter's sub-grids cover the grid it holds in LDS (cells in the two-level form), the count's slices the rows
    gw, gh_ = np.where(two, p["ncx"], w), np.where(two, p["ncy"], h)
    sx, sy, sw, sh = (p[f].astype(np.int64) for f in ("sx", "sy", "w", "h"))
    assert np.all((sx >= 1) & (sy >= 1) & (sx * sw >= gw) & (sy * sh >= gh_) & ((sx - 1) * sw < gw) & ((sy - 1) * sh < gh_))
    cs, cr = p["count_slices"].astype(np.int64), p["count_rows"].astype(np.int64)
    assert np.all((cs >= 1) & (cs * cr >= gh_) & ((cs - 1) * cr < gh_))
    assert np.all(p["count_lds"].astype(np.int64) >= 4 * cr * gw)          # one counter per bin (cell) of a slice
    # cells, table, workgroups
    assert np.all(p["ncx"] == (w + 3) // 4) and np.all(p["ncy"] == (h + 3) // 4) and np.all(p["ncells"] == p["ncx"] * p["ncy"])
    assert np.all(p["table_rows"] >= 1) and np.all(p["table_cols"] >= 1) and np.all(p["table_rows"] == p["blocks"])
    assert np.all(p["table_cols"] == np.where(two, p["ncells"] + 1, nbins))
    assert np.all(p["table_rows"].astype(np.int64) * p["table_cols"] < 1 << 32)
    rounds = p["rounds"].astype(np.int64)
    assert np.all(p["blocks"] == -(-n // (2048 * rounds))) and np.all(rounds >= 1) and np.all(rounds[form != LARGE_GRID] == 1)
    assert np.all(p["extra_wg"] == (form != SEPARATE_FINALIZE))
    # two levels only where they apply; forced off they never run
    assert np.all(p["ncells"][two] <= 4096) and (capacity < 1 << 30 or not two.any())
    if two_level == 0:
        assert not two.any()
    if two_level == 1 and capacity < 1 << 30:
        assert np.all(two[p["ncells"] <= 4096])
    assert np.all(p["cell_grid"][two] == 4 * CUS) and np.all(p["chunks"][two] >= capacity // 2048 + p["ncells"][two] + 1)
    # narrow only on the fused 8-group form, and only when the front end is narrow
    narrow = form == FUSED_NARROW
    assert np.all(groups[narrow] == 8) and np.all(p["steps_per_wave"][narrow] == 4) and (front == NARROW or not narrow.any())
    assert np.all(p["steps_per_wave"][~narrow & (form != LARGE_GRID)] == 2)
    assert np.all(np.isin(p["steps_per_wave"][form == LARGE_GRID], (1, 2) if big == 2 else (2,)))


def test_no_splats_finalize_only(ask):
    p = ask([(60, 34), (120, 68), (256, 256)], 0, 1 << 22, WIDE)
    assert np.all(p["form"] == FINALIZE_ONLY) and np.all(p["blocks"] == 0)
    assert np.all(p["table_rows"].astype(np.int64) * p["table_cols"] >= 1) and np.all(p["nbins"] == (60 * 34, 120 * 68, 65536))


def test_knobs_keep_their_meaning(ask):
    g4k = [(120, 68)]
    assert ask(g4k, 5_000_000, 1 << 25, WIDE, two_level=0, big=1)[0]["rounds"] == 4           # by the scene's size (C4: 4 rounds, 611 workgroups)
    assert ask(g4k, 5_000_000, 1 << 25, WIDE, two_level=0, big=1)[0]["blocks"] == 611
    assert ask(g4k, 5_000_000, 1 << 25, WIDE, two_level=0, big=2, rounds=3)[0]["rounds"] == 3     # GSR_BIN_ROUNDS
    assert ask(g4k, 50_000_000, 1 << 25, WIDE, two_level=0, big=2)[0]["rounds"] == 8              # at most 8 by size
    assert ask(g4k, 5_000_000, 1 << 25, WIDE, rounds=3)[0]["rounds"] == 1                         # two levels: one round
    assert ask(g4k, 5_000_000, 1 << 25, WIDE, cell_grid=300)[0]["cell_grid"] == 300               # GSR_CELL_GRID

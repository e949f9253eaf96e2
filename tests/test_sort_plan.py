"""The sort plan (plan_sort, k_sort.hip) asked directly: no context, no device.

plan_sort is the one function that picks the radix sort's order (LSD or bucket), its width, whether the packed bin
rectangles travel with the keys and whether the frame runs on a band's survivors, and sizes the grids and the LDS of its
launches; sort_sizes, beside it, sizes the tables alloc_sort allocates.  build_frame_args asks plan_sort once per frame and
launch_sort launches by the answer.  gsr_debug_sort_plan / gsr_debug_sort_sizes hand the answers out; the tests here assert
properties of them -- what a wrong plan would break -- not a second copy of the function, over

  * n: 0, 1, around one block of 2048 keys, around the 3 << 20 thresholds, 20 M;
  * the rows the buffers were allocated for: n itself, and 20 M (a scene limitBox has cut down keeps its allocation);
  * both front-end widths, render and sort-only frames, band and full frames;
  * the largest-bucket word: 0, the limit 48 << 10, one above, and 0xffffffff (no frame has reported yet);
  * every value of GSR_SORT_ORDER, GSR_SORT_KPB and both halves of GSR_RECT_CARRY.

The LDS figures are compared with k_scatter's layout, restated here from the kernel's own declarations (cnt[waves][bins],
gdelta[bins], lstart[bins], wsum[3][bins / 64], lkey[keys], lidx[keys], four bytes each)."""
import ctypes
import itertools

import numpy as np
import pytest

NONE, LSD, BUCKET_WIDE, BUCKET_NARROW = range(4)
FIELDS = ("form", "carry", "band", "keys_per_block", "blocks", "waves", "lds_first", "lds_last", "local_grid", "proj_blocks")
PLAN = np.dtype([(f, np.uint32) for f in FIELDS])
INPUTS = ("n", "rows", "front", "render", "cull", "largest", "order", "kpb", "rc", "rcb")
WIDE, NARROW = 16, 8
BUCKET_MAX_N, BUCKET_LIMIT, KPB_SMALL_MAX = 3 << 20, 48 << 10, 3 << 20
NS = (0, 1, 2047, 2048, 2049, (3 << 20) - 1, 3 << 20, (3 << 20) + 1, 20_000_000)
LARGEST = (0, 48 << 10, (48 << 10) + 1, 0xffffffff)
KPBS = (0, 2048, 4096, 8192)


def scatter_lds(bits, keys, waves):
    bins = 1 << bits
    return 4 * (waves * bins + 2 * bins + 3 * (bins // 64) + 2 * keys)


@pytest.fixture(scope="module")
def lib():
    import gsplat_hip
    L = gsplat_hip.load_library()
    L.gsr_debug_sort_plan.restype = ctypes.c_int
    L.gsr_debug_sort_plan.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_uint,
                                      ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.gsr_debug_sort_sizes.restype = ctypes.c_int
    L.gsr_debug_sort_sizes.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def sweep(lib):
    """(inputs, plans): one row per combination of the inputs, as two structured arrays"""
    combos = [c for c in itertools.product(NS, (None, NS[-1]), (WIDE, NARROW), (0, 1), (0, 1), LARGEST, (-1, 0, 1), KPBS, (0, 1), (0, 1))]
    inp = np.zeros(len(combos), dtype=[(f, np.int64) for f in INPUTS])
    out = np.zeros(len(combos), dtype=PLAN)
    for i, (n, rows, *rest) in enumerate(combos):
        inp[i] = (n, n if rows is None else rows) + tuple(rest)
        assert lib.gsr_debug_sort_plan(*[int(v) for v in inp[i]], out.ctypes.data + i * PLAN.itemsize) == PLAN.itemsize
    return inp, out


def _sizes(lib, rows, kpb):
    z = (ctypes.c_ulonglong * 5)()
    assert lib.gsr_debug_sort_sizes(rows, kpb, z) == 5
    return dict(zip(("keys_per_block", "block_hist", "chunk_tab", "kept", "koff"), (int(v) for v in z)))


def test_an_empty_scene_sorts_nothing_and_blocks_cover_the_keys(sweep):
    inp, p = sweep
    n, kpb, blocks = inp["n"], p["keys_per_block"].astype(np.int64), p["blocks"].astype(np.int64)
    empty = n == 0
    assert np.all((p["form"] == NONE) == empty)
    for f in ("carry", "band", "blocks", "waves", "lds_first", "lds_last", "local_grid", "proj_blocks"):
        assert not p[f][empty].any(), f
    assert np.all(np.isin(p["form"][~empty], (LSD, BUCKET_WIDE, BUCKET_NARROW)))
    assert np.all(((blocks * kpb >= n) & (n > (blocks - 1) * kpb))[~empty])
    assert np.all(p["proj_blocks"][~empty] == -(-n[~empty] // 256))


def test_keys_per_block(sweep):
    inp, p = sweep
    assert np.all(np.isin(p["keys_per_block"], (2048, 4096, 8192)))
    pinned = inp["kpb"] != 0
    assert np.all(p["keys_per_block"][pinned] == inp["kpb"][pinned])
    # left to the plan it follows the rows allocated, not the frame's count: a context keeps its block size for a scene's life
    free = ~pinned
    assert np.all(p["keys_per_block"][free] == np.where(inp["rows"][free] <= KPB_SMALL_MAX, 2048, 4096))


def test_the_narrow_form_needs_width_8_blocks_of_2048_and_the_bucket_order(sweep):
    inp, p = sweep
    narrow = p["form"] == BUCKET_NARROW
    assert narrow.any()
    assert np.all(inp["front"][narrow] == NARROW) and np.all(p["keys_per_block"][narrow] == 2048)
    assert np.all((p["waves"] == NARROW) == narrow) and np.all(p["waves"][(p["form"] != NONE) & ~narrow] == WIDE)
    # ... and where all three hold it is taken: a throughput context with GSR_SORT_KPB=4096 runs wide, and the plan says so
    assert not np.any((p["form"] == BUCKET_WIDE) & (inp["front"] == NARROW) & (p["keys_per_block"] == 2048))


def test_the_bucket_order(sweep):
    inp, p = sweep
    bucket = (p["form"] == BUCKET_WIDE) | (p["form"] == BUCKET_NARROW)
    free = inp["order"] < 0
    assert not np.any(bucket & free & (inp["n"] > BUCKET_MAX_N))
    assert not np.any(bucket & free & (inp["largest"] > BUCKET_LIMIT))
    assert not np.any(bucket & free & (inp["largest"] == 0xffffffff))            # a scene's first frame
    live = inp["n"] > 0
    assert np.all(bucket[free & live & (inp["n"] <= BUCKET_MAX_N) & (inp["largest"] <= BUCKET_LIMIT)])
    assert np.all(bucket[live & (inp["order"] == 1)]) and np.all(p["form"][live & (inp["order"] == 0)] == LSD)      # the pin wins
    # render or sort-only, band or not, carried or not: none of them moves the order
    assert np.all((p["local_grid"] > 0) == bucket)


def test_carry_and_band(sweep):
    inp, p = sweep
    bucket = (p["form"] == BUCKET_WIDE) | (p["form"] == BUCKET_NARROW)
    carry, band = p["carry"] == 1, p["band"] == 1
    assert np.all(np.isin(p["carry"], (0, 1))) and np.all(np.isin(p["band"], (0, 1)))
    assert np.all(inp["render"][carry] == 1) and np.all(inp["rc"][carry] == 1)
    assert np.all(inp["rcb"][carry & bucket] == 1)
    assert np.all(carry[(inp["render"] == 1) & (inp["rc"] == 1) & (p["form"] == LSD)])        # what ships: carried in the LSD order
    assert np.all((inp["cull"][band] == 1) & (inp["render"][band] == 1) & (inp["n"][band] > 0))
    assert np.all(band[(inp["cull"] == 1) & (inp["render"] == 1) & (inp["n"] > 0)])


def test_lds_fits_what_the_attribute_raise_asks_for(sweep):
    inp, p = sweep
    kpb, waves = p["keys_per_block"].astype(np.int64), p["waves"].astype(np.int64)
    lsd, bucket = p["form"] == LSD, (p["form"] == BUCKET_WIDE) | (p["form"] == BUCKET_NARROW)
    # the raise: the formula at the widest block of the kernel's width -- 8192 keys at 16 waves, 2048 at 8
    raised = lambda bits: np.where(waves == NARROW, scatter_lds(bits, 2048, NARROW), scatter_lds(bits, 8192, WIDE))
    assert np.all(p["lds_first"][lsd] >= scatter_lds(8, kpb, waves)[lsd]) and np.all(p["lds_first"][lsd] <= raised(8)[lsd])
    assert np.all(p["lds_last"][lsd] >= scatter_lds(9, kpb, waves)[lsd]) and np.all(p["lds_last"][lsd] <= raised(9)[lsd])
    assert np.all(p["lds_first"][bucket] >= scatter_lds(9, kpb, waves)[bucket]) and np.all(p["lds_first"][bucket] <= raised(9)[bucket])
    assert not p["lds_last"][bucket].any()                   # one k_scatter pass; k_local_sort's LDS is static
    assert raised(9).max() <= 160 * 1024                     # a CU's LDS


def test_the_grid_of_the_local_sort_covers_every_chunk(sweep):
    inp, p = sweep
    bucket = (p["form"] == BUCKET_WIDE) | (p["form"] == BUCKET_NARROW)
    # 257 buckets, each up to one partial chunk of 4096 keys beyond its whole ones
    assert np.all(p["local_grid"][bucket] >= -(-inp["n"][bucket] // 4096) + 257)


@pytest.mark.parametrize("kpb", KPBS)
def test_allocation_sizes_hold_every_plan_of_their_rows(lib, sweep, kpb):
    inp, p = sweep
    for rows in NS:
        z = _sizes(lib, rows, kpb)
        assert z["keys_per_block"] == (kpb or (2048 if rows <= KPB_SMALL_MAX else 4096))
        # at least what the sizes were before they were computed from the kernels' constants
        assert z["chunk_tab"] >= 4 * (rows // 4096 + 260)
        assert z["block_hist"] >= max(-(-rows // z["keys_per_block"]), 1) * 512
        assert z["kept"] >= rows // 256 + 1 and z["koff"] >= rows // 256 + 2
        # every frame of up to `rows` splats in buffers allocated for them
        fits = (inp["rows"] == rows) & (inp["n"] <= rows) & (inp["kpb"] == kpb)
        assert fits.any()
        q = p[fits]
        assert np.all(q["keys_per_block"] == z["keys_per_block"])
        assert z["chunk_tab"] >= 4 * (1 + int(q["local_grid"].max()))
        assert z["block_hist"] >= int(q["blocks"].max()) * 512
        assert z["kept"] >= int(q["proj_blocks"].max()) + 1 and z["koff"] >= int(q["proj_blocks"].max()) + 2


def test_what_ships(lib):
    """the plans of the benchmarked contexts, by name: C3's 700 k splats, default and throughput, first frame and later ones"""
    def ask(n, front, largest, **kw):
        out = np.zeros(1, dtype=PLAN)
        assert lib.gsr_debug_sort_plan(n, n, front, 1, 0, largest, kw.get("order", -1), kw.get("kpb", 0), kw.get("rc", 1), kw.get("rcb", 0),
                                       out.ctypes.data) == PLAN.itemsize
        return out[0]
    first, later = ask(700000, WIDE, 0xffffffff), ask(700000, WIDE, 5000)
    assert (first["form"], first["carry"], first["blocks"]) == (LSD, 1, 342) and (later["form"], later["carry"], later["waves"]) == (BUCKET_WIDE, 0, 16)
    assert ask(700000, NARROW, 5000)["form"] == BUCKET_NARROW and ask(700000, NARROW, 5000, kpb=4096)["form"] == BUCKET_WIDE
    assert ask(700000, NARROW, 5000, rcb=1)["carry"] == 1 and ask(700000, WIDE, 5000, rc=0, order=0)["carry"] == 0
    assert ask(5_000_000, WIDE, 5000)["form"] == LSD and ask(5_000_000, WIDE, 5000)["keys_per_block"] == 4096

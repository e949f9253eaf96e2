"""Every bin list against an exact reference, in every form the binning stage can take.

The binning stage (k_bin.hip) is about a dozen kernel instantiations; plan_bins picks the form from the bin grid, the kind
of context and knobs, and launch_bin launches it (tests/test_bin_plan.py asks the plan itself, on the CPU).  Its result
has an exact integer specification (tests/bin_reference.py, checked on the CPU by tests/test_bin_reference.py), and every test here renders through the ordinary API and then
demands that `starts` and `list` equal that reference ENTRY FOR ENTRY -- the reference fed with the ORACLE's boxes and
depth order (oracle.project / oracle.sort), never with the device's own read-backs -- together with bin_totals(), the
frame's bin_entries and visible counts, depthIndex, and no overflow left pending.

Forms (one test id at least names each; which kernel a geometry reaches is plan_bins' answer: 8 groups
of steps fit two workgroups per CU up to 2408 bins; profiles/bin_lists_kernels.txt is the kernel table of one run of this
file, the proof that they ran):

    k_bin_count<16> + k_bin_scatter<8, true>          up to ~2400 bins, default context (640x480 ... 1920x1080)
    k_bin_count<8> + k_bin_scatter_narrow<8>          the same on a throughput context
    k_bin_scatter<4, true>                            2401 .. 4096 bins (2560x1440, 2560x1600), either kind of context
    k_bin_finalize + k_bin_scatter<4, false>          > 4096 bins, GSR_BIN_TWO_LEVEL=0 GSR_BIN_BIG=0          (knobs only)
    k_bin_starts + k_bin_scatter_big<4, 2> / <4, 1>   the same with GSR_BIN_BIG=1 / 2, GSR_BIN_ROUNDS 1 and > 1  (knobs only)
    sliced one level                                  6144x3216 (1 x 3 sub-grids, 2 count slices), 7680x4320 (2 x 2, 3 slices),
                                                      GSR_BIN_TWO_LEVEL=0                                      (knobs only)
    two level, k_cell_scatter1<8>                     > 4096 bins (3840x2160); forced on at 640x480, 1000x712
    two level, k_cell_scatter1<4>                     8192x8192 (64 x 64 cells)
    band contexts                                     inside one level 1080p, one level 4 groups, two level 4K; a band of
                                                      one bin column; bands that do not start or end on a cell

There is no k_bin_scatter<8, false> and no k_bin_scatter_big<8, 2>: both would need more than 4096 bins whose sub-grid still
fits 8 groups in 72 KiB, and make_slices returns the FEWEST sub-grids that fit 4 groups in 150 KiB, which for every grid of
1 .. 256 x 1 .. 256 bins (every framebuffer and band the ABI accepts) above 4096 bins leaves a sub-grid too large for 8
(tests/test_bin_plan.py asserts it of the plan for every such grid; the largest grid that takes 8 groups has 2408 bins).

Where the rectangles come from changes the code that runs in k_bin_count and in the sort: a context's first frame of a
scene sorts in the LSD order with the rectangles carried through the radix passes (rects_sorted), later frames in the
bucket order, where k_bin_count gathers them through depthIndex; GSR_SORT_ORDER=lsd GSR_RECT_CARRY=0 gathers in the LSD
order, GSR_RECT_CARRY=2 carries them through the bucket order's kernels.  So every context renders two poses or more.

The sort's narrow kernels (throughput contexts, bucket order) exist for 2048 keys per workgroup only, which is what
every scene of up to 3 << 20 splats gets (plan_sort, k_sort.hip): all the ragged sizes below reach them."""
import os

import numpy as np
import pytest

import bin_reference as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
KNOBS = ("GSR_BIN_TWO_LEVEL", "GSR_BIN_BIG", "GSR_BIN_ROUNDS", "GSR_RECT_CARRY", "GSR_SORT_ORDER", "GSR_FRONT_WAVES")
ONE_LEVEL = {"GSR_BIN_TWO_LEVEL": "0"}
TWO_LEVEL = {"GSR_BIN_TWO_LEVEL": "1"}
# where the rectangles come from (the default: carried in the first frame's LSD order, gathered in the bucket order behind it)
LSD_GATHER = {"GSR_SORT_ORDER": "lsd", "GSR_RECT_CARRY": "0"}
LSD_CARRY = {"GSR_SORT_ORDER": "lsd"}
BUCKET_CARRY = {"GSR_RECT_CARRY": "2"}


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


class Frame:
    """The oracle's statement of one (scene, pose, size): boxes, depth order, and the reference lists per band."""

    def __init__(self, oracle, data, pos, cam, W, H):
        v, p, vp = cam.f32()
        self.W, self.H = W, H
        self.obbox = oracle.project(data, v, p, cam.fx, cam.fy, W, H)[1]
        self.odi = oracle.sort(vp, pos)[0]
        self._lists = {}

    def lists(self, band=None):
        if band not in self._lists:
            self._lists[band] = B.bin_lists_reference(self.obbox, self.odi, self.W, self.H, band)
        return self._lists[band]

    def visible(self, band=None):
        return B.visible_reference(self.obbox, self.W, self.H, band)


@pytest.fixture(scope="module")
def frames(oracle):
    """one oracle projection and sort per (scene, pose, size), shared by every form that renders it"""
    cache = {}

    def get(key, data, pos, cam, W, H):
        if key not in cache:
            cache[key] = Frame(oracle, data, pos, cam, W, H)
        return cache[key]

    yield get
    cache.clear()


def _context(gh, monkeypatch, W, H, env=None, throughput=False, band=None, lib_path=None):
    """a context created under exactly the knobs of `env` (all knobs are read once, by gsr_create)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    r = gh.HIPRenderer(W, H, band=band, throughput=throughput, lib_path=lib_path)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return r


def _check(r, fr, band, what):
    """the context's last frame against the reference: lists, totals, counts, order"""
    want_s, want_l = fr.lists(band)
    starts, lst = r.bin_lists()
    diff = B.first_difference(starts, lst, want_s, want_l, fr.obbox)
    assert diff is None, (what, diff)
    assert np.array_equal(r.bin_totals().reshape(-1), np.diff(want_s.astype(np.int64))), what
    st = r.stats()
    assert st["bin_entries"] == int(want_s[-1]), (what, st["bin_entries"], int(want_s[-1]))
    assert st["visible"] == fr.visible(band), (what, st["visible"], fr.visible(band))
    assert np.array_equal(r.lastDepthIndex(), fr.odi), (what, "depthIndex")
    assert not r.overflow_pending() and st["dropped_frames"] == 0, (what, st)
    return st


def _render(r, cam):
    """the blocking render of the scene the context holds (a list overflow is repaired inside it: regrowth, same frame again)"""
    r.render(None, cam)


# ---------------------------------------------------------------------------
# the forms
# ---------------------------------------------------------------------------
def _scene_of(gh, scenes, name):
    """(key, data, positions, fx at width W, poses)"""
    if name in gh.synth.CONFIGS:                      # a benchmarked configuration, at its own size and the full-size tests' poses
        cfg = gh.synth.CONFIGS[name]
        _, data, pos = scenes(name)
        return data, pos, (lambda W: cfg["fx"] * W / cfg["width"]), {"C2": (13, 40), "C3": (21, 84), "C4": (50, 51)}[name]
    if name == "mid":                                 # 60 k splats of up to ~9 x 9 bins at 4K
        _, data, pos = scenes(60000, 77, sigma=1.2, s_lo=0.004, s_hi=0.09)
        return data, pos, (lambda W: 1132.0 * W / 1920.0), (4, 41)
    assert name == "big"                              # the large framebuffers' scene (test_large_framebuffer_sliced_binning)
    _, data, pos = scenes(30000, 33)
    return data, pos, (lambda W: 3600.0 * W / 6144.0), (17, 75)


def _case(id, scene, size, env=None, throughput=False, band=None):
    return pytest.param(scene, size, env or {}, throughput, band, id=id)


FORMS = [
    # one level, 8 groups: the 1080p chain of either kind of context
    _case("k_bin_count<16>+k_bin_scatter<8,true> C2 default", "C2", (1920, 1080)),
    _case("k_bin_count<8>+k_bin_scatter_narrow<8> C2 throughput", "C2", (1920, 1080), throughput=True),
    _case("k_bin_count<16>+k_bin_scatter<8,true> C3 default", "C3", (1920, 1080)),
    _case("k_bin_count<8>+k_bin_scatter_narrow<8> C3 throughput", "C3", (1920, 1080), throughput=True),
    _case("k_bin_scatter<8,true> 1080p lsd gather", "mid", (1920, 1080), LSD_GATHER),
    _case("k_bin_scatter<8,true> 1080p bucket carried", "mid", (1920, 1080), BUCKET_CARRY),
    _case("k_bin_scatter_narrow<8> 1080p lsd gather", "mid", (1920, 1080), LSD_GATHER, throughput=True),
    _case("k_bin_scatter_narrow<8> 1080p bucket carried", "mid", (1920, 1080), BUCKET_CARRY, throughput=True),
    _case("k_bin_scatter_narrow<8> 1000x712", "mid", (1000, 712), throughput=True),
    # one level, 4 groups, fused finalize: 2401 .. 4096 bins
    _case("k_bin_scatter<4,true> 2560x1440 default", "mid", (2560, 1440)),
    _case("k_bin_scatter<4,true> 2560x1440 throughput", "mid", (2560, 1440), throughput=True),
    _case("k_bin_scatter<4,true> 2560x1600 default", "mid", (2560, 1600)),
    _case("k_bin_scatter<4,true> 2560x1600 throughput", "mid", (2560, 1600), throughput=True),
    _case("k_bin_scatter<4,true> 2560x1440 lsd gather", "mid", (2560, 1440), LSD_GATHER),
    _case("k_bin_scatter<4,true> 2560x1440 bucket carried", "mid", (2560, 1440), BUCKET_CARRY, throughput=True),
    _case("k_bin_scatter<4,true> 2560x1440 C2 scene", "C2", (2560, 1440)),
    # one level above 4096 bins: knobs only
    _case("k_bin_finalize+k_bin_scatter<4,false> 4K", "mid", (3840, 2160), dict(ONE_LEVEL, GSR_BIN_BIG="0")),
    _case("k_bin_finalize+k_bin_scatter<4,false> 4K lsd gather", "mid", (3840, 2160), dict(ONE_LEVEL, GSR_BIN_BIG="0", **LSD_GATHER)),
    _case("k_bin_scatter_big<4,2> 4K rounds by size", "mid", (3840, 2160), dict(ONE_LEVEL, GSR_BIN_BIG="1")),
    _case("k_bin_scatter_big<4,2> 4K 3 rounds", "mid", (3840, 2160), dict(ONE_LEVEL, GSR_BIN_BIG="1", GSR_BIN_ROUNDS="3")),
    _case("k_bin_scatter_big<4,1> 4K 1 round", "mid", (3840, 2160), dict(ONE_LEVEL, GSR_BIN_BIG="2", GSR_BIN_ROUNDS="1")),
    _case("k_bin_scatter_big<4,1> 4K 5 rounds bucket carried", "mid", (3840, 2160), dict(ONE_LEVEL, GSR_BIN_BIG="2", GSR_BIN_ROUNDS="5", **BUCKET_CARRY)),
    # ... cut into sub-grids (blockIdx.y) and count row slices
    _case("sliced 1x3 sub-grids 2 count slices k_bin_scatter<4,false> 6144x3216", "big", (6144, 3216), dict(ONE_LEVEL, GSR_BIN_BIG="0")),
    _case("sliced 1x3 sub-grids k_bin_scatter_big<4,2> 6144x3216 2 rounds", "big", (6144, 3216), dict(ONE_LEVEL, GSR_BIN_BIG="1", GSR_BIN_ROUNDS="2")),
    _case("sliced 1x3 sub-grids k_bin_scatter_big<4,1> 6144x3216 lsd gather", "big", (6144, 3216), dict(ONE_LEVEL, GSR_BIN_BIG="2", **LSD_GATHER)),
    _case("sliced 2x2 sub-grids 3 count slices k_bin_scatter<4,false> 7680x4320", "big", (7680, 4320), dict(ONE_LEVEL, GSR_BIN_BIG="0")),
    _case("sliced 2x2 sub-grids k_bin_scatter_big<4,1> 7680x4320 2 rounds", "big", (7680, 4320), dict(ONE_LEVEL, GSR_BIN_ROUNDS="2")),
    # two level
    _case("two level k_cell_scatter1<8> C4", "C4", (3840, 2160)),
    _case("two level k_cell_scatter1<8> 4K", "mid", (3840, 2160)),
    _case("two level k_cell_scatter1<8> 4K lsd gather", "mid", (3840, 2160), LSD_GATHER),
    _case("two level k_cell_scatter1<8> 4K bucket carried", "mid", (3840, 2160), BUCKET_CARRY),
    _case("two level k_cell_scatter1<8> forced 640x480", "mid", (640, 480), TWO_LEVEL),
    _case("two level k_cell_scatter1<8> forced 1000x712 lsd", "mid", (1000, 712), dict(TWO_LEVEL, **LSD_CARRY)),
    _case("two level k_cell_scatter1<8> 6144x3216", "big", (6144, 3216)),
    _case("two level k_cell_scatter1<4> 8192x8192", "big", (8192, 8192)),
    _case("two level k_cell_scatter1<4> 8192x8192 lsd gather", "big", (8192, 8192), LSD_GATHER),
    # band contexts (columns numbered from the band's first; survivors only are sorted and binned; a band starts on a bin, by the ABI)
    _case("band in one level 1080p", "C2", (1920, 1080), band=(864, 1056)),
    _case("band in one level 1080p throughput unaligned", "C2", (1920, 1080), throughput=True, band=(512, 1230)),
    _case("band of one bin column 1080p", "C2", (1920, 1080), band=(960, 992)),
    _case("band of one bin column 1080p lsd gather", "C2", (1920, 1080), LSD_GATHER, band=(928, 950)),
    _case("band in one level 4 groups 2560x1440 (60 columns)", "mid", (2560, 1440), band=(192, 2100)),
    _case("band in one level 4 groups 2560x1440 throughput lsd", "mid", (2560, 1440), LSD_CARRY, throughput=True, band=(192, 2100)),
    _case("band in two level 4K not on cells (67 columns from 37)", "mid", (3840, 2160), band=(1184, 3300)),
    _case("band in two level 4K not on cells lsd gather", "mid", (3840, 2160), LSD_GATHER, band=(1184, 3300)),
    _case("band of one bin column two level forced 4K", "mid", (3840, 2160), TWO_LEVEL, band=(1952, 1984)),
    _case("band last partial column two level forced 1000x712", "mid", (1000, 712), TWO_LEVEL, band=(896, 1000)),
    _case("band in sliced one level 7680x4320", "big", (7680, 4320), dict(ONE_LEVEL, GSR_BIN_BIG="0"), band=(992, 7000)),
]


def _run_form(gh, scenes, frames, monkeypatch, scene, size, env, throughput, band, lib_path=None):
    W, H = size
    data, pos, fx_at, poses = _scene_of(gh, scenes, scene)
    r = _context(gh, monkeypatch, W, H, env, throughput, band, lib_path)
    r.set_raw_scene(data, pos)
    entries = []
    for k in poses:
        cam = gh.orbit_camera(k, 120, W, H, fx_at(W))
        _render(r, cam)
        fr = frames((scene, k, W, H), data, pos, cam, W, H)
        st = _check(r, fr, band, (scene, size, env, throughput, band, "pose %d" % k))
        entries.append(st["bin_entries"])
    bins = r.work_items()["bins"]
    lo, hi, nby = B.bin_grid(W, H, band)
    assert bins == (hi - lo) * nby
    assert min(entries) > 2 * bins or band is not None and min(entries) > 0     # lists worth comparing
    r.dispose()


@pytest.mark.parametrize("scene,size,env,throughput,band", FORMS)
def test_form_builds_the_reference_lists(gh, scenes, frames, monkeypatch, scene, size, env, throughput, band):
    _run_form(gh, scenes, frames, monkeypatch, scene, size, env, throughput, band)


BOUNDS_SITES = ["splat index of a rank", "rectangle inside the bin grid", "LDS cell of the scatter", "table row", "count cell"]


BOUNDS_FORMS = [
    _case("k_bin_scatter<4,true> 2560x1440", "mid", (2560, 1440)),
    _case("k_bin_scatter<4,true> 2560x1600 throughput", "mid", (2560, 1600), throughput=True),
    _case("sliced 1x3 k_bin_scatter<4,false> 6144x3216", "big", (6144, 3216), dict(ONE_LEVEL, GSR_BIN_BIG="0")),
    _case("sliced 2x2 k_bin_scatter_big<4,1> 7680x4320", "big", (7680, 4320), dict(ONE_LEVEL, GSR_BIN_ROUNDS="2")),
    _case("sliced 2x2 k_bin_scatter_big<4,2> 7680x4320", "big", (7680, 4320), dict(ONE_LEVEL, GSR_BIN_BIG="1")),
    _case("two level k_cell_scatter1<4> 8192x8192", "big", (8192, 8192)),
]


@pytest.mark.parametrize("scene,size,env,throughput,band", BOUNDS_FORMS)
def test_bounds_checked_build_of_the_rarely_run_forms(gh, scenes, frames, monkeypatch, scene, size, env, throughput, band):
    """The forms no other test runs, on the bounds-checked build of the library (tests/test_gpu_bounds.py): the same lists,
    and no index derived from device data outside what it indexes.  (First in the file's order of cases by name: pytest
    runs a module's tests in the order they are written, and this one is written after the forms -- a session that wants
    the checked build first selects it with -k bounds_checked.)"""
    import ctypes
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    _run_form(gh, scenes, frames, monkeypatch, scene, size, env, throughput, band, lib_path=BOUNDS_LIB)
    L = gh.load_library(BOUNDS_LIB)
    for name in ("bin", "sort", "blend"):
        buf = (ctypes.c_uint32 * 8)()
        assert getattr(L, "gsr_debug_bounds_" + name)(buf) == 0
        assert not any(buf), (name, list(buf), BOUNDS_SITES if name == "bin" else None)


# ---------------------------------------------------------------------------
# geometries where a ballot / lane-set scatter goes wrong
# ---------------------------------------------------------------------------
def _rows_with(rows, pos=None, scale=None, alpha=None):
    r = np.array(rows, dtype=np.uint8).reshape(-1, 32)
    if pos is not None:
        r[:, 0:12] = np.ascontiguousarray(pos, dtype=np.float32).view(np.uint8).reshape(-1, 12)
    if scale is not None:
        r[:, 12:24] = np.ascontiguousarray(np.broadcast_to(np.float32(scale), (r.shape[0], 3)), dtype=np.float32).view(np.uint8).reshape(-1, 12)
    if alpha is not None:
        r[:, 27] = alpha
    return r


def _positions(rows):
    return np.array(rows, dtype=np.uint8).reshape(-1, 32)[:, 0:12].copy().view(np.float32).reshape(-1, 3)


@pytest.mark.parametrize("size,n", [((640, 480), 20000), ((1000, 712), 6000)])
@pytest.mark.parametrize("kind", ["default", "throughput", "two level"])
def test_every_box_covers_the_whole_screen(gh, oracle, monkeypatch, size, n, kind):
    """Splats so large that the projection clamps their axes to 1024 px: every box is the screen, every lane of every
    column and row word of the scatter is set, the lists are visible x bins entries -- more than a new context's list
    buffer holds, so the first frame overflows once, the lists are regrown and the frame rendered again."""
    W, H = size
    rows = _rows_with(gh.synth.synth_rows(n, 91, 0.3, 0.004, 0.06), scale=60.0)
    data, pos = oracle.scene_pack(rows.reshape(-1))
    r = _context(gh, monkeypatch, W, H, TWO_LEVEL if kind == "two level" else None, kind == "throughput")
    r.set_raw_scene(data, pos)
    for i, k in enumerate((6, 7)):
        cam = gh.orbit_camera(k, 120, W, H, 1132.0)
        fr = Frame(oracle, data, pos, cam, W, H)
        vis = fr.obbox[:, 0] <= fr.obbox[:, 2]
        assert vis.sum() >= n - n // 50 and np.all(fr.obbox[vis] == (0, 0, W - 1, H - 1))      # the property the test is named for
        bins = -(-W // 32) * -(-H // 32)
        assert fr.lists()[0][-1] == int(vis.sum()) * bins > (1 << 22)
        _render(r, cam)
        st = _check(r, fr, None, (size, kind, k))
        assert st["overflow_frames"] == 1 and st["dropped_frames"] == 0, st                    # once, in the first frame
    r.dispose()


@pytest.mark.parametrize("kind", ["default", "throughput", "two level"])
def test_every_visible_splat_in_one_bin(gh, oracle, monkeypatch, kind):
    """A tiny blob of tiny splats in the middle of a bin (672x480: the screen's centre is the centre of bin (10, 7)): one
    bin of more than 64 x 256 entries, every other bin empty -- one column and one row bit for every lane, and a slot
    count that runs through all the steps of every group."""
    W, H, n = 672, 480, 20000
    rows = _rows_with(gh.synth.synth_rows(n, 92, 0.01, 0.0004, 0.001))
    data, pos = oracle.scene_pack(rows.reshape(-1))
    r = _context(gh, monkeypatch, W, H, TWO_LEVEL if kind == "two level" else None, kind == "throughput")
    r.set_raw_scene(data, pos)
    for k in (6, 7, 50):
        cam = gh.orbit_camera(k, 120, W, H, 1132.0)
        fr = Frame(oracle, data, pos, cam, W, H)
        bb = fr.obbox[fr.obbox[:, 0] <= fr.obbox[:, 2]]
        assert bb.shape[0] > 64 * 256
        assert np.all(bb[:, 0] // 32 == 10) and np.all(bb[:, 2] // 32 == 10) and np.all(bb[:, 1] // 32 == 7) and np.all(bb[:, 3] // 32 == 7)
        starts = fr.lists()[0]
        assert np.count_nonzero(np.diff(starts.astype(np.int64))) == 1
        _render(r, cam)
        _check(r, fr, None, (kind, k))
    r.dispose()


def _rank_scene(gh, oracle, V, cam, W, H, seed):
    """A scene of which exactly V splats are visible from `cam`, with invisible ones interleaved: behind every third visible
    splat (in index order) sits a twin moved 60 units along the view's y axis -- out of the frustum at the same depth, so the
    twin is its neighbour in the depth order too -- and in the middle of the scene a run of 2 x 2048 + 64 such twins of the
    visible splat of median depth: consecutive ranks (equal depths are ordered by index) that hold an empty workgroup.  The
    scene starts with 70 twins of its nearest visible splat."""
    pool = gh.synth.synth_rows(V + V // 2 + 2000, seed, 0.7, 0.004, 0.03).reshape(-1, 32)
    data, pos = oracle.scene_pack(pool.reshape(-1))
    v, p, vp = cam.f32()
    bb = oracle.project(data, v, p, cam.fx, cam.fy, W, H)[1]
    vis = np.flatnonzero((bb[:, 0] <= bb[:, 2]) & (bb[:, 1] <= bb[:, 3]))
    assert vis.size >= V
    keep = pool[vis[:V]]
    kp = _positions(keep)
    up = np.array([v[1], v[5], v[9]], dtype=np.float32) * np.float32(60.0)
    twins = _rows_with(keep, pos=kp + up)
    depth = kp.astype(np.float64) @ np.array([vp[2], vp[6], vp[10]], dtype=np.float64)
    median = int(np.argsort(depth, kind="stable")[V // 2])
    out = [twins[int(np.argmin(depth))]] * 70   # (a step and more of invisible ranks in front of the first visible one)
    for i in range(V):
        out.append(keep[i])
        if i % 3 == 0:
            out.append(twins[i])
        if i == V // 2:
            out.extend([twins[median]] * (2 * 2048 + 64))
    return np.stack(out).reshape(-1)


def _assert_rank_properties(fr, V):
    vis = (fr.obbox[:, 0] <= fr.obbox[:, 2]) & (fr.obbox[:, 1] <= fr.obbox[:, 3])
    assert int(vis.sum()) == V
    by_rank = vis[fr.odi]
    ranks = np.flatnonzero(by_rank)
    assert ranks[0] >= 64 and (V < 2 or np.mean(fr.odi[ranks] != ranks) > 0.9)     # invisible ranks in front; a splat's rank is not its index
    # the longest run of invisible ranks: holds a whole 64-rank step and a whole 2048-rank workgroup, with visible ranks on both sides
    edges = np.flatnonzero(np.diff(np.concatenate([[1], by_rank.astype(np.int8), [1]])))
    runs = edges.reshape(-1, 2)
    a, b = runs[np.argmax(runs[:, 1] - runs[:, 0])]
    assert -(-a // 2048) * 2048 + 2048 <= b, (a, b)
    if V >= 3:
        assert ranks[0] < a and b <= ranks[-1]


RANKS = [1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 3 * 2048 + 1]


@pytest.mark.parametrize("kind", ["default", "throughput", "throughput bucket", "two level", "band"])
@pytest.mark.parametrize("V", RANKS)
def test_visible_ranks_at_the_edges_of_steps_and_workgroups(gh, oracle, monkeypatch, V, kind):
    """Exactly V visible splats (the last step / workgroup full, one short, one over), invisible ranks among them and an
    empty workgroup in the middle of the order; on default and throughput contexts (the narrow sort and binning kernels,
    with the bucket order pinned and chosen by the context), two levels, and a band context whose survivors are the
    visible splats of its columns."""
    W, H = 640, 480
    cams = [gh.orbit_camera(k, 120, W, H, 1132.0) for k in (9, 10, 70)]
    rows = _rank_scene(gh, oracle, V, cams[0], W, H, 300 + V)
    data, pos = oracle.scene_pack(rows)
    env = {"throughput bucket": {"GSR_SORT_ORDER": "bucket"}, "two level": TWO_LEVEL}.get(kind)
    band = (160, 500) if kind == "band" else None
    r = _context(gh, monkeypatch, W, H, env, kind.startswith("throughput"), band)
    r.set_raw_scene(data, pos)
    for i, cam in enumerate(cams):
        fr = Frame(oracle, data, pos, cam, W, H)
        if i == 0:
            _assert_rank_properties(fr, V)
        _render(r, cam)
        _check(r, fr, band, (V, kind, i))
    r.dispose()


@pytest.mark.parametrize("order", ["bucket", None])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 5 * 2048 + 1])
def test_narrow_sort_at_ragged_sizes(gh, oracle, scenes, monkeypatch, n, order):
    """The 8-wave k_scatter / k_local_sort of throughput contexts at sizes that end a wave, a step or a workgroup exactly, one
    short and one over (2048 keys per workgroup, the narrow forms' only block size, is what every n here gets): depthIndex
    against the oracle bit for bit over three poses, the bucket order pinned, and left to the context (its first frame
    sorts in the LSD order) -- and the lists of each frame, which are built from that order."""
    W, H = 640, 480
    _, data, pos = scenes(n, 400 + n)
    r = _context(gh, monkeypatch, W, H, {"GSR_SORT_ORDER": order} if order else None, True)
    r.set_raw_scene(data, pos)
    for k in (0, 17, 63):
        cam = gh.orbit_camera(k, 120, W, H, 1132.0)
        _render(r, cam)
        fr = Frame(oracle, data, pos, cam, W, H)
        assert np.array_equal(r.lastDepthIndex(), fr.odi), (n, order, k)
        _check(r, fr, None, (n, order, k))
    r.dispose()


@pytest.mark.parametrize("size,scene_args,fx", [((333, 201), (20000, 21), 400.0), ((1000, 712), (60000, 77, 1.2, 0.004, 0.09), 1400.0)])
@pytest.mark.parametrize("kind", ["default", "throughput", "two level", "band"])
def test_boxes_on_bin_edges_and_partial_bins(gh, oracle, scenes, monkeypatch, size, scene_args, fx, kind):
    """Framebuffers whose last bin column and row are partial, and at least a hundred boxes each that end on the last pixel of
    a bin or start on its first, in x and in y, and that touch the last column / row."""
    W, H = size
    n, seed = scene_args[:2]
    kw = dict(zip(("sigma", "s_lo", "s_hi"), scene_args[2:]))
    _, data, pos = scenes(n, seed, **kw)
    band = ((W // 2 - 40) // 32 * 32, W) if kind == "band" else None
    r = _context(gh, monkeypatch, W, H, TWO_LEVEL if kind == "two level" else None, kind == "throughput", band)
    r.set_raw_scene(data, pos)
    for k in (9, 52):
        cam = gh.orbit_camera(k, 120, W, H, fx)
        fr = Frame(oracle, data, pos, cam, W, H)
        bb = fr.obbox[(fr.obbox[:, 0] <= fr.obbox[:, 2]) & (fr.obbox[:, 1] <= fr.obbox[:, 3])]
        assert W % 32 and H % 32
        for col, rem in ((2, 31), (0, 0), (3, 31), (1, 0)):
            assert (bb[:, col] % 32 == rem).sum() >= 100, (col, rem)
        assert (bb[:, 2] // 32 == (W - 1) // 32).sum() >= 10 and (bb[:, 3] // 32 == (H - 1) // 32).sum() >= 10
        _render(r, cam)
        _check(r, fr, band, (size, kind, k))
    r.dispose()

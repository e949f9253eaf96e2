"""The specification of the compositor's work list (tests/work_items_reference.py) pinned on the CPU, and the cases of
tests/test_gpu_work_items.py with the conditions they are chosen for.

  * cut() against a loop per bin, on random counts and figures and on the hand-made edges of every branch;
  * partial_class at its edges;
  * check_work_list, the checker the GPU module uses, rejects five wrong lists built from a right one;
  * frame_figures' V and D on C1 against bin_reference.visible_reference and the oracle's render_scene;
  * every case of the GPU module: the branch of the policy it is there for is the one the oracle's frame takes, the binning form
    is the one it names (plan_bins asked as tests/test_bin_plan.py asks it), and the interval of the optical mass decides nothing
    (input_condition) -- all from the oracle and the plans alone, so a case that cannot tell right from wrong fails here, on a
    machine without a GPU.  (The plans are asked for 256 compute units here; the GPU module takes the context's own.)"""
import ctypes

import numpy as np
import pytest

import bin_reference as B
import work_items_reference as R
from test_bin_plan import FINALIZE_ONLY, FUSED_NARROW, FUSED_WIDE, LARGE_GRID, SEPARATE_FINALIZE, TWO_LEVEL
from test_bin_plan import PLAN as BIN_PLAN
from test_blend_plan import default_capacity, plan_of

U32 = R.U32_MAX
POSES = (3, 47)
S30 = (30000, 0.6, 0.03, 0.25)        # synth_rows(n, 9, sigma, s_lo, s_hi): 24 px of optical mass per list entry at 640 x 480
S60 = (60000, 0.6, 0.03, 0.25)
S80 = (80000, 0.6, 0.03, 0.25)
S40 = (40000, 0.6, 0.01, 0.12)        # small splats: 8.5 px per entry
BLOB = (5000, 0.05, 0.01, 0.03)       # a small blob in the middle of the screen: the bands at its side hold nothing
ENV_TO_KNOB = {"GSR_LONG_ITEMS": "long_items", "GSR_LONG_TAU": "long_tau", "GSR_SATURATE": "saturate", "GSR_SEG_LEN": "seg_len",
               "GSR_SEG_TARGET": "seg_target", "GSR_ITEMS_BY_SIZE": "items_by_size"}
KNOBS = tuple(ENV_TO_KNOB) + ("GSR_BIN_TWO_LEVEL", "GSR_BIN_BIG", "GSR_FUSE_COMBINE", "GSR_BLEND_SUB", "GSR_BLEND_GRID", "GSR_BIN_ROUNDS",
                              "GSR_RECT_CARRY", "GSR_SORT_ORDER", "GSR_FRONT_WAVES")


# ---------------------------------------------------------------------------
# the cases of the GPU module
# ---------------------------------------------------------------------------
def _case(id, scene, expect, size=(640, 480), throughput=False, band=None, env=None, eps=0.0, form=None, records=False):
    if form is None:
        form = FUSED_NARROW if throughput else FUSED_WIDE
    return dict(id=id, scene=scene, expect=expect, size=size, throughput=throughput, band=band, env=env or {}, eps=eps, form=form, records=records)


def _long(c, a):
    return c >= a["long_from"]


# what a case is there for: asserted of cut()'s answer `a` for the oracle's frame (counts c, plan p), first pose `first`
def x_default_30k(a, c, p, first):
    assert not a["dense"] and a["heavy"] and a["by_size"] and a["whole_bins"] > 0 and a["cut_bins"] > 0
    assert a["seg_len"] < a["long_from"] < a["mxbin"]
    if first:
        assert (a["long_from"], a["whole_bins"], a["cut_bins"], a["mxbin"]) == (2526, 16, 6, 13767)


def x_throughput_30k(a, c, p, first):
    assert a["dense"] and a["cut_bins"] == 0 and a["by_size"] and not p["items_by_size"]
    assert (_long(c, a) & (c < a["seg_len"])).any() and (_long(c, a) & (c > 2 * a["seg_len"])).any()      # whole comes before cut
    if first:
        assert (a["long_from"], a["whole_bins"]) == (337, 30)


def x_dense_80k(a, c, p, first):
    assert a["dense"] and a["cut_bins"] == 0 and a["mxbin"] > 16 * a["seg_len"]
    if first:
        assert a["whole_bins"] == 39


def x_neither_40k(a, c, p, first):
    assert not a["dense"] and not a["heavy"] and a["long_from"] == U32 and a["whole_bins"] == 0 and a["cut_bins"] >= 10
    if first:
        assert a["cut_bins"] == 16


def x_mixed_40k(a, c, p, first):
    assert not a["dense"] and p["long_mass_min"] == 0 and a["heavy"] and a["whole_bins"] > 0 and a["cut_bins"] > 0 and a["by_size"]


def x_one_per_bin(a, c, p, first):
    assert a["mxbin"] < min(a["long_from"], a["seg_len"]) and a["cut_bins"] == 0 and a["n_items"] == c.size and a["E"] > 0


def x_policy_0(a, c, p, first):
    assert p["long_policy"] == 0 and a["long_from"] == U32 and a["cut_bins"] > 0


def x_policy_1(a, c, p, first):
    assert p["long_policy"] == 1 and a["long_from"] == 0 and a["n_items"] == c.size and a["by_size"] and a["mxbin"] > a["seg_len"]


def x_tau_20(a, c, p, first):
    assert p["long_tau_bin"] == 20 and a["long_from"] == -(-(20 * 1024 * a["E"]) // a["mass"]) < a["seg_len"] and a["whole_bins"] > 16 and not a["dense"]


def x_seg_256(a, c, p, first):
    assert a["seg_len"] == 256 and a["long_from"] == U32 and 32 < a["nseg"].max() < 64 and a["mxbin"] > 32 * 256


def x_seg_256_capped(a, c, p, first):
    assert a["seg_len"] == 256 and a["mxbin"] > 64 * 256 and a["nseg"].max() == 64 and a["r"].max() > 256      # the last takes the rest


def x_seg_target(a, c, p, first):
    assert p["seg_target_items"] == 50 and a["seg_len"] == a["E"] // 50 // 256 * 256 > p["seg_len"]


def x_by_size_forced(a, c, p, first):
    assert p["items_by_size"] == 0 and a["by_size"] and a["whole_bins"] > 0


def x_by_size_pinned(a, c, p, first):
    assert p["items_by_size"] == 1 and a["by_size"]


def x_raster(a, c, p, first):
    assert not p["items_by_size"] and not a["by_size"] and a["cut_bins"] > 3


def x_sentinel(a, c, p, first):
    assert p["whole_bin"] and a["seg_len"] >= R.WHOLE_BIN_FROM and a["n_items"] == c.size and np.array_equal(a["seg_start"], np.arange(c.size + 1))


def x_empty(a, c, p, first):
    assert a["E"] == 0 and a["n_items"] == c.size and not c.any() and a["long_from"] == U32


def x_any(a, c, p, first):
    assert a["E"] > 2 * c.size


def x_band_dense(a, c, p, first):
    assert c.size == 30 and a["dense"] and a["whole_bins"] >= 10
    if first:
        assert a["whole_bins"] == 14


NO_LONG = {"GSR_LONG_ITEMS": "0"}
CASES = [
    # the branches of the policy
    _case("30k default: heavy, not dense", S30, x_default_30k, records=True),
    _case("30k throughput: dense", S30, x_throughput_30k, throughput=True),
    _case("80k default: dense", S80, x_dense_80k),
    _case("40k default: neither", S40, x_neither_40k),
    _case("40k throughput: mixed", S40, x_mixed_40k, throughput=True),
    _case("C1 default: one item per bin", "C1", x_one_per_bin),
    _case("C1 throughput: one item per bin", "C1", x_one_per_bin, throughput=True),
    # the knobs
    _case("GSR_LONG_ITEMS=0", S30, x_policy_0, env=NO_LONG),
    _case("GSR_LONG_ITEMS=1", S30, x_policy_1, env={"GSR_LONG_ITEMS": "1"}),
    _case("GSR_LONG_TAU=20", S30, x_tau_20, env={"GSR_LONG_TAU": "20"}),
    _case("GSR_SATURATE=0", S30, x_policy_0, env={"GSR_SATURATE": "0"}),
    _case("GSR_SEG_LEN=256 GSR_LONG_ITEMS=0", S30, x_seg_256, env=dict(NO_LONG, GSR_SEG_LEN="256")),
    _case("GSR_SEG_LEN=256 GSR_LONG_ITEMS=0 60k: over the cap", S60, x_seg_256_capped, env=dict(NO_LONG, GSR_SEG_LEN="256")),
    _case("GSR_SEG_TARGET=50", S30, x_seg_target, env={"GSR_SEG_TARGET": "50"}),
    _case("GSR_ITEMS_BY_SIZE=0 default: whole bins force the order", S30, x_by_size_forced, env={"GSR_ITEMS_BY_SIZE": "0"}),
    _case("GSR_ITEMS_BY_SIZE=0 throughput: whole bins force the order", S30, x_by_size_forced, throughput=True, env={"GSR_ITEMS_BY_SIZE": "0"}),
    _case("GSR_ITEMS_BY_SIZE=1 default", S30, x_by_size_pinned, env={"GSR_ITEMS_BY_SIZE": "1"}),
    _case("GSR_ITEMS_BY_SIZE=1 throughput", S30, x_by_size_pinned, throughput=True, env={"GSR_ITEMS_BY_SIZE": "1"}),
    _case("GSR_ITEMS_BY_SIZE=0 GSR_LONG_ITEMS=0 default: raster order", S30, x_raster, env=dict(NO_LONG, GSR_ITEMS_BY_SIZE="0")),
    _case("GSR_LONG_ITEMS=0 throughput: raster order", S30, x_raster, throughput=True, env=NO_LONG),
    _case("early termination: the sentinel", S30, x_sentinel, eps=1e-4),
    # the variants of the finalize step
    _case("stand-alone: empty scene", "empty", x_empty, form=FINALIZE_ONLY),
    _case("narrow 1920x1080 throughput: four bins per thread", S30, x_any, size=(1920, 1080), throughput=True),
    _case("wide 1920x1080 default: two bins per thread", S30, x_any, size=(1920, 1080)),
    _case("k_cell_scatter2: GSR_BIN_TWO_LEVEL=1", S30, x_default_30k, env={"GSR_BIN_TWO_LEVEL": "1"}, form=TWO_LEVEL),
    _case("separate finalize 2080x2048 GSR_BIN_BIG=0", S30, x_any, size=(2080, 2048), env={"GSR_BIN_TWO_LEVEL": "0", "GSR_BIN_BIG": "0"}, form=SEPARATE_FINALIZE),
    _case("large grid 2080x2048 GSR_BIN_BIG=2", S30, x_any, size=(2080, 2048), env={"GSR_BIN_TWO_LEVEL": "0", "GSR_BIN_BIG": "2"}, form=LARGE_GRID),
    # bands
    # (a context's band starts on a bin column, by the ABI: these own the bin columns of (300, 340) and (200, 330), and end inside one)
    _case("band (288, 340) default", S30, x_band_dense, band=(288, 340)),
    _case("band (288, 340) throughput", S30, x_band_dense, band=(288, 340), throughput=True),
    _case("band (192, 330)", S40, x_any, band=(192, 330)),
    _case("band no splat touches", BLOB, x_empty, band=(0, 64)),
]
CASE_IDS = [c["id"] for c in CASES]
BY_ID = {c["id"]: c for c in CASES}
BOUNDS_TOUR = ("30k default: heavy, not dense", "40k throughput: mixed", "band (288, 340) throughput")
OVERFLOW_CASE = "30k default: heavy, not dense"


def fx_of(gh, case):
    W = case["size"][0]
    if case["scene"] == "C1":
        return gh.synth.CONFIGS["C1"]["fx"] * W / gh.synth.CONFIGS["C1"]["width"]
    return 400.0 * W / 640.0


def scene_of(scenes, case):
    """(data u32[8n], positions f32[3n]) of a case"""
    if case["scene"] == "empty":
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32)
    if case["scene"] == "C1":
        return scenes("C1")[1:]
    n, sigma, lo, hi = case["scene"]
    return scenes(n, 9, sigma=sigma, s_lo=lo, s_hi=hi)[1:]


class Frame:
    """the oracle's statement of one (scene, pose, size): boxes, axes, depth order; per band the entries per bin and the figures"""

    def __init__(self, oracle, data, pos, cam, W, H):
        self.W, self.H, self.n = W, H, pos.size // 3
        if self.n:
            v, p, vp = cam.f32()
            _, self.obbox, self.raw = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
            self.odi = oracle.sort(vp, pos)[0]
        else:
            self.obbox, self.raw, self.odi = np.zeros((0, 4), np.int32), np.zeros((0, 12), np.float32), np.zeros(0, np.uint32)
        self.data = data
        self._band = {}

    def of(self, band):
        """(bin starts, entries per bin, figures) for a band"""
        if band not in self._band:
            starts = B.bin_lists_reference(self.obbox, self.odi, self.W, self.H, band)[0]
            self._band[band] = (starts, np.diff(starts.astype(np.int64)), R.frame_figures(self.data, self.obbox, self.raw, self.W, self.H, band))
        return self._band[band]


@pytest.fixture(scope="session")
def work_frames(oracle, scenes):
    """one oracle projection and sort per (scene, pose, size), shared by every case that renders it (never changed)"""
    import gsplat_hip as gh
    cache = {}

    def get(case, pose):
        W, H = case["size"]
        key = (case["scene"], pose, W, H)
        if key not in cache:
            data, pos = scene_of(scenes, case)
            cache[key] = Frame(oracle, data, pos, gh.orbit_camera(pose, 120, W, H, fx_of(gh, case)), W, H)
        return cache[key]

    return get


def cpu_plan(L, case, nbins, npix, n, cus=256):
    knobs = {ENV_TO_KNOB[k]: int(v) for k, v in case["env"].items() if k in ENV_TO_KNOB}
    return plan_of(L, nbins=nbins, npix=npix, capacity=default_capacity(n), cus=cus, throughput=case["throughput"], early_out=case["eps"] > 0, **knobs)


def bin_form(L, case, n, cus=256):
    fn = L.gsr_debug_bin_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_uint,
                   ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_uint, ctypes.c_void_p]
    lo, hi, nby = B.bin_grid(case["size"][0], case["size"][1], case["band"])
    out = np.zeros(1, dtype=BIN_PLAN)
    env = case["env"]
    assert fn(hi - lo, nby, n, default_capacity(n), cus, 8 if case["throughput"] else 16, int(env.get("GSR_BIN_TWO_LEVEL", -1)),
              int(env.get("GSR_BIN_BIG", 2)), 0, 0, out.ctypes.data) == BIN_PLAN.itemsize
    return out[0]


def expected(case, fr, plan, capacity):
    """cut() for a case's frame at both ends of the optical mass interval, the input condition asserted: (at lo, at hi, counts, figures)"""
    _, counts, fig = fr.of(case["band"])
    lo, hi = R.cut_interval(counts, fig, plan, capacity)
    bad = R.input_condition(counts, lo, hi)
    assert bad is None, (case["id"], bad)
    for k in ("dense", "long_from", "seg_len", "by_size", "n_items", "fits"):
        assert lo[k] == hi[k], (case["id"], k)
    return lo, hi, counts, fig


@pytest.mark.parametrize("id", CASE_IDS)
def test_case_takes_the_branch_it_is_there_for(work_frames, id):
    import gsplat_hip
    L = gsplat_hip.load_library()
    case = BY_ID[id]
    W, H = case["size"]
    lo, hi, nby = B.bin_grid(W, H, case["band"])
    nbins = (hi - lo) * nby
    for pose in POSES:
        fr = work_frames(case, pose)
        plan = cpu_plan(L, case, nbins, (hi - lo) * 32 * H, fr.n)
        a, _, counts, fig = expected(case, fr, plan, default_capacity(fr.n))
        assert counts.size == nbins and a["fits"]
        assert fig["omass_hi"] - fig["omass_lo"] <= fig["uncertain"] <= max(fr.n // 1000, 1)
        case["expect"](a, counts, plan, pose == POSES[0])
        right = a["items"][np.argsort(-a["classes"], kind="stable")] if a["by_size"] else R.expected_sequence(a)      # a list that meets the specification
        assert R.check_work_list(right, a["seg_start"], a, nbins, default_capacity(fr.n), plan["max_items"]) is None
    bp = bin_form(L, case, fr.n)
    assert bp["form"] == case["form"] and bp["nbins"] == nbins, (id, bp)
    # the bins per thread of the step the case names: FIN_THREADS is 1024, 512 as the narrow scatter's extra workgroup
    per = -(-nbins // (512 if case["form"] == FUSED_NARROW else 1024))
    if "bins per thread" in id:
        assert per == {"two": 2, "four": 4}[id.split(": ")[1].split()[0]]
    if case["size"] == (640, 480) and case["band"] is None:
        assert nbins == 300 and per == 1


# ---------------------------------------------------------------------------
# cut() against a loop per bin
# ---------------------------------------------------------------------------
def make_plan(**kw):
    p = dict(seg_len=1024, seg_target_items=5000, max_items=1 << 20, items_by_size=1, long_policy=-1, long_tau=340, long_tiles_x2=0, long_tau_bin=0,
             long_mass_min=12, npix=640 * 480)
    p.update(kw)
    return p


def cut_brute(counts, fig, plan, capacity):
    """the specification as one loop over the bins, in Python integers"""
    counts = [int(c) for c in counts]
    E = min(sum(counts), 2 ** 32 - 1)
    mass = fig["omass"] * 256 // 255
    dense = fig["otiles"] * 4096 >= plan["long_tau"] * 255 * plan["npix"] and 2 * fig["D"] >= plan["long_tiles_x2"] * fig["V"]
    heavy = mass >= plan["long_mass_min"] * E
    sentinel = plan["seg_len"] >= 1 << 30
    if sentinel or plan["long_policy"] == 0:
        long_from = 2 ** 32 - 1
    elif plan["long_policy"] > 0:
        long_from = 0
    elif mass > 0 and (dense or heavy or plan["long_tau_bin"]):
        tb = plan["long_tau_bin"] or (8 if dense else 60)
        long_from = min(0xfffffff0, (tb * 1024 * E + mass - 1) // mass)
    else:
        long_from = 2 ** 32 - 1
    seg_len = plan["seg_len"] if sentinel else min(max(E // plan["seg_target_items"] // 256 * 256, plan["seg_len"]), max(8192, plan["seg_len"]))
    full, last, bin_start, seg_start = [], [], [0], [0]
    for b, c in enumerate(counts):
        nf = 0 if c >= long_from else min(c // seg_len, 63)
        r = c - nf * seg_len
        has_last = r > 0 or nf == 0
        nseg = nf + has_last
        w3 = seg_start[b] | nseg << 25
        for k in range(nf):
            end = bin_start[b] + c if k + 1 == nseg else bin_start[b] + (k + 1) * seg_len
            full.append(((b | k << 16, bin_start[b] + k * seg_len, end, w3), int(R.partial_class(seg_len))))
        if has_last:
            last.append(((b | nf << 16, bin_start[b] + nf * seg_len, bin_start[b] + c, w3), int(R.partial_class(r))))
        bin_start.append(bin_start[b] + c)
        seg_start.append(seg_start[b] + nseg)
    fits = bin_start[-1] <= capacity and seg_start[-1] <= plan["max_items"]
    by_size = bool(plan["items_by_size"]) or (max(counts) if counts else 0) >= long_from
    if not fits:
        bin_start, seg_start = [0] * len(bin_start), [0] * len(seg_start)
    return dict(E=E, mass=mass, dense=dense, heavy=heavy, long_from=long_from, seg_len=seg_len, fits=fits, by_size=by_size,
                n_items=len(full) + len(last) if fits else 0, bin_start=bin_start, seg_start=seg_start, sequence=full + last)


def assert_same_cut(counts, fig, plan, capacity):
    a, w = R.cut(counts, fig, plan, capacity), cut_brute(counts, fig, plan, capacity)
    for k in ("E", "mass", "dense", "heavy", "long_from", "seg_len", "fits", "by_size", "n_items"):
        assert a[k] == w[k], (k, a[k], w[k])
    assert a["bin_start"].tolist() == w["bin_start"] and a["seg_start"].tolist() == w["seg_start"]
    seq = R.expected_sequence(a)
    assert seq.tolist() == [list(i) for i, _ in w["sequence"]]
    cls = np.concatenate([a["classes"][~a["is_last"]], a["classes"][a["is_last"]]])
    assert cls.tolist() == [c for _, c in w["sequence"]]
    return a


FIG = dict(V=1000, D=4000, otiles=0, omass=300000)


def test_cut_equals_the_loop_on_random_inputs():
    rng = np.random.default_rng(5)
    for trial in range(300):
        nb = int(rng.integers(1, 70))
        counts = (rng.integers(0, 2, nb) * rng.integers(0, int(rng.choice([5, 600, 3000, 70000])), nb)).astype(np.int64)
        fig = dict(V=int(rng.integers(0, 5000)), D=int(rng.integers(0, 40000)), otiles=int(rng.integers(0, 1 << 24)), omass=int(rng.integers(0, 1 << 22)) * int(rng.integers(0, 2)))
        plan = make_plan(seg_len=int(rng.choice([256, 512, 1024, 1 << 30])), seg_target_items=int(rng.choice([1, 50, 1300, 5000])),
                         max_items=int(rng.choice([3, 200, 1 << 20])), items_by_size=int(rng.integers(0, 2)), long_policy=int(rng.integers(-1, 2)),
                         long_tau=int(rng.choice([120, 340])), long_tiles_x2=int(rng.choice([0, 7])), long_tau_bin=int(rng.choice([0, 0, 20])),
                         long_mass_min=int(rng.choice([0, 12])), npix=int(rng.choice([1024, 640 * 480])))
        assert_same_cut(counts, fig, plan, int(rng.choice([100, 1 << 22])))


def test_cut_at_the_edges_of_a_bin():
    S = 1024
    plan = make_plan(long_policy=0)
    a = assert_same_cut([0, S - 1, S, S + 1, 63 * S, 64 * S - 1, 64 * S, 100 * S], FIG, plan, 1 << 22)
    assert a["seg_len"] == S
    assert a["nseg"].tolist() == [1, 1, 1, 2, 63, 64, 64, 64]
    assert a["r"].tolist() == [0, S - 1, 0, 1, 0, S - 1, S, 37 * S]            # the 64th segment takes whatever is left
    items = a["items"]
    assert items[0].tolist() == [0, 0, 0, 0 | 1 << 25]                        # an empty bin is one item with first == end
    one = items[(items[:, 0] & 0xffff) == 2]
    assert one.shape[0] == 1 and one[0, 2] - one[0, 1] == S and not a["is_last"][a["seg_start"][2]]      # c == seg_len: one full segment, no last
    assert (a["nseg"] <= 64).all()
    last = items[a["seg_start"][8] - 1]
    assert last[0] == (7 | 63 << 16) and last[2] - last[1] == 37 * S and last[2] == a["bin_start"][8]


def test_cut_at_the_edges_of_the_policy():
    counts = np.array([10, 3000, 2525, 2526, 0, 700], dtype=np.int64)
    E = int(counts.sum())
    heavy_fig = dict(FIG, omass=E * 24 * 255 // 256 + 1000)                    # 24 px per entry
    a = assert_same_cut(counts, heavy_fig, make_plan(), 1 << 22)
    assert a["heavy"] and not a["dense"] and a["long_from"] == -(-(60 * 1024 * E) // a["mass"])
    # c = long_from - 1 is cut, c = long_from is one item: with omass = 1020 E the mass is 1024 E, and long_tau_bin = L gives long_from = L
    for L in (1500, 3000):
        edge = [L - 1, L, 7]
        e = assert_same_cut(edge, dict(FIG, omass=1020 * sum(edge)), make_plan(long_tau_bin=L), 1 << 22)
        assert e["long_from"] == L and e["nseg"].tolist() == [-(-(L - 1) // 1024), 1, 1] and e["by_size"]
    d = R.cut([2999, 3000], dict(FIG, omass=0), make_plan(long_tau_bin=3000), 1 << 22)
    assert d["long_from"] == U32                                                # mass == 0: nothing is long, whatever the knob
    assert_same_cut([0, 0, 0], dict(V=0, D=0, otiles=0, omass=0), make_plan(), 1 << 22)                   # E == 0
    for policy in (-1, 0, 1):
        g = assert_same_cut(counts, heavy_fig, make_plan(long_policy=policy), 1 << 22)
        assert g["long_from"] == {-1: a["long_from"], 0: U32, 1: 0}[policy]
    g = assert_same_cut(counts, heavy_fig, make_plan(seg_len=1 << 30, long_policy=1), 1 << 22)             # the sentinel wins
    assert g["long_from"] == U32 and g["seg_len"] == 1 << 30 and g["n_items"] == counts.size
    g = assert_same_cut(counts, heavy_fig, make_plan(long_tau_bin=20), 1 << 22)
    assert g["long_from"] == -(-(20 * 1024 * E) // g["mass"])
    dense = assert_same_cut(counts, dict(heavy_fig, otiles=340 * 255 * 640 * 480 // 4096 + 1), make_plan(), 1 << 22)
    assert dense["dense"] and dense["long_from"] == -(-(8 * 1024 * E) // dense["mass"])
    assert not R.cut(counts, dict(heavy_fig, otiles=340 * 255 * 640 * 480 // 4096 - 1), make_plan(), 1 << 22)["dense"]
    assert not R.cut(counts, dict(heavy_fig, otiles=1 << 30, V=1000, D=3499), make_plan(long_tiles_x2=7), 1 << 22)["dense"]
    assert R.cut(counts, dict(heavy_fig, otiles=1 << 30, V=1000, D=3500), make_plan(long_tiles_x2=7), 1 << 22)["dense"]


def test_cut_that_does_not_fit():
    counts = [100, 2000, 0]
    for capacity, max_items in ((2099, 1 << 20), (1 << 22, 3)):               # entries > capacity; items > max_items (2000 is two segments)
        a = assert_same_cut(counts, FIG, make_plan(long_policy=0, max_items=max_items), capacity)
        assert not a["fits"] and a["n_items"] == 0 and not a["bin_start"].any() and not a["seg_start"].any() and a["items_needed"] == 4
    assert assert_same_cut(counts, FIG, make_plan(long_policy=0, max_items=4), 2100)["fits"]


def test_seg_len_rounding_and_cap():
    for target, E, want in ((50, 50 * 1280 - 1, 1024), (50, 50 * 1280, 1280), (50, 50 * 1536 - 1, 1280), (50, 50 * 8192, 8192), (50, 50 * 9000, 8192),
                            (5000, 5000 * 1023, 1024), (1, 255, 1024)):
        a = assert_same_cut([E], FIG, make_plan(seg_target_items=target, long_policy=0), 1 << 30)
        assert a["seg_len"] == want, (target, E, a["seg_len"])
    assert R.cut([1 << 20], FIG, make_plan(seg_len=16384, seg_target_items=1, long_policy=0), 1 << 30)["seg_len"] == 16384      # a minimum above the cap stays


def test_partial_class():
    def scalar(r):
        if r < 4:
            return r
        e = r.bit_length() - 1
        return min(63, (e - 1) * 4 + ((r >> (e - 2)) & 3))

    assert [int(R.partial_class(r)) for r in range(5)] == [0, 1, 2, 3, 4]
    pts = sorted({max(v, 0) for k in range(18) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1)} | {65535, 65536, 1 << 20, (1 << 32) - 1})
    assert [int(v) for v in R.partial_class(np.array(pts))] == [scalar(r) for r in pts]
    every = R.partial_class(np.arange(1 << 17))
    assert (np.diff(every) >= 0).all() and every[65535] == 59 and every[65536] == 60 and every[7 << 14] == 63 and every[(7 << 14) - 1] == 62 and every.max() == 63
    assert int(R.partial_class(1 << 30)) == 63


# ---------------------------------------------------------------------------
# the checker rejects wrong lists
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def right():
    counts = np.array([0, 5000, 130, 2600, 9000, 17, 3000, 1024, 64, 2100], dtype=np.int64)
    E = int(counts.sum())
    plan = make_plan()
    a = R.cut(counts, dict(FIG, omass=E * 22), plan, 1 << 22)
    assert a["by_size"] and a["heavy"] and 2600 < a["long_from"] <= 3000 and a["cut_bins"] == 2 and a["whole_bins"] == 3
    rng = np.random.default_rng(1)
    order = np.lexsort((rng.permutation(a["n_items"]), -a["classes"]))          # heaviest first, any order inside a class
    items = a["items"][order]
    args = (counts.size, 1 << 22, plan["max_items"])
    assert R.check_work_list(items, a["seg_start"], a, *args) is None
    assert R.check_work_list(a["items"], a["seg_start"], a, *args) is not None   # (raster order is not heaviest first here)
    return a, items, args, counts


def test_checker_rejects_a_dropped_last_segment(right):
    a, items, args, _ = right
    drop = np.flatnonzero(items[:, 0] == (3 | 2 << 16))[0]                        # bin 3: 2600 = 2 x 1024 + 552
    assert R.check_work_list(np.delete(items, drop, axis=0), a["seg_start"], a, *args) is not None


def test_checker_rejects_an_end_one_short(right):
    a, items, args, _ = right
    for row in (0, items.shape[0] // 2, items.shape[0] - 1):
        if items[row, 2] > items[row, 1]:
            bad = items.copy()
            bad[row, 2] -= 1
            assert "item set" in R.check_work_list(bad, a["seg_start"], a, *args)


def test_checker_rejects_a_shared_partial_slot(right):
    a, items, args, _ = right
    bad = items.copy()
    of9, slot3 = (bad[:, 0] & 0xffff) == 9, int(a["seg_start"][3])
    bad[of9, 3] = slot3 | (bad[of9, 3] >> 25 << 25)                               # bin 9 writes its partials where bin 3 does
    assert "share partial slots" in R.check_work_list(bad, a["seg_start"], a, *args)
    assert "share partial slots" in R.item_invariants(bad, *args)
    assert R.item_invariants(items, *args) is None


def test_checker_rejects_the_reversed_order(right):
    a, items, args, _ = right
    assert "heaviest first" in R.check_work_list(items[::-1], a["seg_start"], a, *args)
    # and without by_size the sequence is exact: two last segments exchanged
    b = R.cut(right[3], dict(FIG, omass=0), make_plan(items_by_size=0), 1 << 22)
    seq = R.expected_sequence(b)
    assert not b["by_size"] and R.check_work_list(seq, b["seg_start"], b, *args) is None
    swapped = seq.copy()
    swapped[[-1, -2]] = swapped[[-2, -1]]
    assert "raster order" in R.check_work_list(swapped, b["seg_start"], b, *args)


def test_checker_rejects_a_long_bin_cut_anyway(right):
    a, items, args, counts = right
    assert counts[6] >= a["long_from"]                                            # bin 6, 3000 entries: one item
    cut_all = R.cut(counts, dict(FIG, omass=0), make_plan(), 1 << 22)             # the same bins with nothing long
    assert cut_all["nseg"][6] == 3
    w = R.check_work_list(cut_all["items"], cut_all["seg_start"], a, *args)
    assert w is not None
    # even with the right number of items and the right seg_start: bin 6's one item replaced by a first segment
    bad = items.copy()
    row = np.flatnonzero((bad[:, 0] & 0xffff) == 6)[0]
    bad[row, 2] = bad[row, 1] + 1024
    assert "item set" in R.check_work_list(bad, a["seg_start"], a, *args)


def test_item_invariants_name_what_breaks(right):
    a, items, args, _ = right
    nbins, capacity, max_items = args
    for col, value, word in ((0, nbins, "bin < nbins"), (0, 3 | 5 << 16, "seg < nseg"), (2, capacity + 1, "capacity")):
        bad = items.copy()
        bad[1, col] = value
        assert word in R.item_invariants(bad, *args), word
    assert "max_items" in R.item_invariants(items, nbins, capacity, int(a["seg_start"][-1]) - 1)
    c = R.canonical(items)
    other = a["items"][np.lexsort((np.random.default_rng(2).permutation(a["n_items"]), -a["classes"]))]      # another order inside the classes
    assert not np.array_equal(other, items) and np.array_equal(c, R.canonical(other))
    assert R.check_work_list(c, a["seg_start"], a, *args) is None


# ---------------------------------------------------------------------------
# figures
# ---------------------------------------------------------------------------
def test_figures_of_c1(oracle, scenes):
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C1"]
    _, data, pos = scenes("C1")
    W, H = cfg["width"], cfg["height"]
    cam = gh.orbit_camera(3, 120, W, H, cfg["fx"])
    v, p, vp = cam.f32()
    _, bb, raw = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
    fig = R.frame_figures(data, bb, raw, W, H)
    _, _, V, D = oracle.render_scene(data, pos, v, p, vp, cam.fx, cam.fy, W, H, mode=1)
    assert fig["V"] == V == B.visible_reference(bb, W, H) and fig["D"] == D and V > 1000
    assert 0 < fig["omass_lo"] <= fig["omass_hi"] <= fig["omass_lo"] + fig["uncertain"]
    band = (200, 330)
    fb = R.frame_figures(data, bb, raw, W, H, band)
    assert fb["V"] == B.visible_reference(bb, W, H, band) < V and fb["D"] < D
    # as the kernel defines a band today: tiles clipped to the band, mass not -- the band's splats carry their whole footprint
    keep = (bb[:, 0] <= bb[:, 2]) & (bb[:, 1] <= bb[:, 3]) & ~((bb[:, 2] < 192) | (bb[:, 0] >= 352))
    sub = R.frame_figures(data.reshape(-1, 8)[keep], bb[keep], raw[keep], W, H)
    assert (fb["omass_lo"], fb["omass_hi"]) == (sub["omass_lo"], sub["omass_hi"]) and fb["D"] < sub["D"]

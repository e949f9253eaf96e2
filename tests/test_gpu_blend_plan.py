"""The compositor launched is the compositor planned.

plan_blend (k_blend.hip) picks the compositor's kernel, grid and work-item policy and launch_bin / launch_blend launch from its
answer alone (tests/test_blend_plan.py asks the function itself, on the CPU).  Here every kind of context that takes another
path through the plan renders one frame of a small scene, and then

  (a) the plan the context holds (gsr_debug_last_blend_plan) equals what gsr_debug_blend_plan answers for the context's inputs;
  (b) the fields the case is here for have the values it names;
  (c) work_items() agrees with the plan: the waves per tile, a published segment length that is the sentinel or a multiple of
      256 of at least the plan's minimum, at most max_items items, exactly one per bin for whole bins, more than one per bin where
      GSR_LONG_ITEMS=0 has the long bin cut;
  (d) the image lies within the bound tests/test_gpu_parity.py applies to that kind of frame against the oracle (2e-4; 1e-3
      with early termination at 1e-4);
  (e) pairs agree: the fold fused and separate bit for bit, GSR_BLEND_GRID=3 and the default bit for bit, one and two waves per
      tile within the 2e-6 the project states for another f32 association.

The scene: 1100 splats of gsplat_hip.synth around the origin and a stack of 2900 small ones in one bin of the 256 x 128 frame's
8 x 4, in the right half, so that -- asserted below under tests/bin_reference.py's lists -- the longest bin holds between
2 x 1024 + 1 and 4 x 1024 entries (more than two segments at either kernel's minimum length, one partial), some bin is empty
and some bin holds 1 .. 255 entries (less than a chunk).  One frame of 2080 x 2048, 65 x 64 = 4160 bins, the smallest grid
above the 4096 up to which an unpinned context takes two waves per tile, shows 4000 splats without a stack."""
import ctypes
import os

import numpy as np
import pytest

import bin_reference as B
from test_blend_plan import PLAN, WHOLE_BIN_FROM, default_capacity, plan_of
from test_gpu_parity import TOL_EARLY, TOL_EXACT

pytestmark = pytest.mark.gpu

W, H = 256, 128
BIG_W, BIG_H = 2080, 2048
POSE = 5
RIGHT_HALF = (128, 256)
EARLY_EPS = 1e-4                  # (tests/test_gpu_parity.py, test_image_parity_early_out)
KNOBS = ("GSR_FUSE_COMBINE", "GSR_SATURATE", "GSR_ITEMS_BY_SIZE", "GSR_LONG_ITEMS", "GSR_LONG_TAU", "GSR_BLEND_SUB", "GSR_SEG_TARGET",
         "GSR_BLEND_GRID", "GSR_SEG_LEN")
NO_LONG = {"GSR_LONG_ITEMS": "0"}


def _case(id, env=None, throughput=False, eps=0.0, band=None, big=False, **named):
    return pytest.param(id, id=id), dict(env=env or {}, throughput=throughput, eps=eps, band=band, big=big, named=named)


# (b): per case, the plan's fields it is there for ("cus": times the device's compute units)
_CASES = [
    _case("default", waves_per_tile=2, threads=512, fused=1, separate_fold=0, whole_bin=0, seg_len=1024, grid=(3, "cus"), seg_target_items=5000,
          items_by_size=1, long_policy=-1, long_tau=340, saturate=1),
    _case("default GSR_LONG_ITEMS=0", env=NO_LONG, waves_per_tile=2, long_policy=0),
    _case("throughput", throughput=True, waves_per_tile=1, threads=256, seg_len=512, grid=(7, "cus"), seg_target_items=1300, items_by_size=0,
          long_policy=-1, long_tau=120),
    _case("throughput GSR_LONG_ITEMS=0", env=NO_LONG, throughput=True, waves_per_tile=1, long_policy=0),
    _case("early termination", eps=EARLY_EPS, whole_bin=1, partial_slots=0, separate_fold=0, long_policy=0, waves_per_tile=2),
    _case("GSR_BLEND_SUB=1", env={"GSR_BLEND_SUB": "1"}, waves_per_tile=1, threads=256, seg_len=512, grid=(7, "cus")),
    _case("throughput GSR_BLEND_SUB=2", env={"GSR_BLEND_SUB": "2"}, throughput=True, waves_per_tile=2, threads=512, seg_len=1024, grid=(3, "cus")),
    _case("GSR_FUSE_COMBINE=0 GSR_LONG_ITEMS=0", env=dict(NO_LONG, GSR_FUSE_COMBINE="0"), fused=0, separate_fold=1, long_policy=0),
    _case("GSR_SEG_LEN=256 GSR_LONG_ITEMS=0", env=dict(NO_LONG, GSR_SEG_LEN="256"), seg_len=256, long_policy=0),
    _case("GSR_BLEND_GRID=3", env={"GSR_BLEND_GRID": "3"}, grid=3, queue_start=3),
    _case("band over the right half", band=RIGHT_HALF, npix=128 * H, waves_per_tile=2),
    _case("2080x2048", big=True, waves_per_tile=1, threads=256, seg_len=512, grid=(7, "cus"), npix=BIG_W * BIG_H),
]
CASES = [c[0] for c in _CASES]
SPEC = {c[0].values[0]: c[1] for c in _CASES}


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _rows(gh, big):
    if big:
        return gh.synth.synth_rows(4000, 31, 1.0, 0.004, 0.03)
    stack = gh.synth._edit(gh.synth.synth_rows(2900, 32, 0.02, 0.004, 0.02), offset=(0.3, 0.2, 0.0))
    return np.concatenate([gh.synth.synth_rows(1100, 31, 1.0, 0.004, 0.03), stack])


@pytest.fixture(scope="module")
def material(gh, oracle):
    """per frame size: the scene, the camera, the oracle's image and the reference's entries per bin (computed once, never changed)"""
    out = {}
    for big, (w, h) in ((False, (W, H)), (True, (BIG_W, BIG_H))):
        data, pos = oracle.scene_pack(_rows(gh, big))
        cam = gh.orbit_camera(POSE, 120, w, h, 1132.0 * w / 1920.0)
        v, p, vp = cam.f32()
        obbox = oracle.project(data, v, p, cam.fx, cam.fy, w, h)[1]
        oimg, odi, _, _ = oracle.render_scene(data, pos, v, p, vp, cam.fx, cam.fy, w, h, mode=1)
        counts = {band: np.diff(B.bin_lists_reference(obbox, odi, w, h, band)[0].astype(np.int64)) for band in ((None,) if big else (None, RIGHT_HALF))}
        oimg.setflags(write=False)
        out[big] = dict(data=data, pos=pos, n=pos.size // 3, cam=cam, oimg=oimg, counts=counts, size=(w, h))
    return out


def test_the_scene_has_the_bins_the_cases_need(material):
    """the conditions the scene is built for, on the CPU's reference lists (nothing here touches the device)"""
    for band in (None, RIGHT_HALF):
        c = material[False]["counts"][band]
        assert c.size == (32 if band is None else 16)
        assert 2 * 1024 + 1 <= c.max() <= 4 * 1024, c.max()
        assert (c == 0).any() and ((c >= 1) & (c <= 255)).any()
    c = material[True]["counts"][None]
    assert c.size == 65 * 64 and c.size > 4096 and c.max() <= 300


def _last_plan(r):
    out = np.zeros(1, dtype=PLAN)
    fn = r._L.gsr_debug_last_blend_plan
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]
    assert fn(r._ctx, out.ctypes.data) == 0
    return out[0]


@pytest.fixture(scope="module")
def rendered(gh, material):
    """case id -> what its context planned, published and drew: each context is created under exactly its knobs, renders its one
    frame once, and what it left is kept for the pairs"""
    cache = {}

    def get(id):
        if id in cache:
            return cache[id]
        s = SPEC[id]
        m = material[s["big"]]
        w, h = m["size"]
        saved = {k: os.environ.pop(k, None) for k in KNOBS}      # (all knobs are read once, by gsr_create)
        try:
            os.environ.update(s["env"])
            r = gh.HIPRenderer(w, h, early_out_eps=s["eps"], band=s["band"], throughput=s["throughput"])
        finally:
            for k in KNOBS:
                os.environ.pop(k, None)
                if saved[k] is not None:
                    os.environ[k] = saved[k]
        r.set_raw_scene(m["data"], m["pos"])
        r.render(None, m["cam"])
        cache[id] = dict(plan=_last_plan(r), items=r.work_items(), img=r.readPixelsFloat(), overflow=r.overflow_pending(),
                         overflow_frames=r.stats()["overflow_frames"], L=r._L)
        r.dispose()
        return cache[id]

    yield get
    cache.clear()


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("id", CASES)
def test_the_compositor_launched_is_the_compositor_planned(rendered, material, id):
    s = SPEC[id]
    m = material[s["big"]]
    w, h = m["size"]
    x0, x1 = s["band"] or (0, w)
    nbins = ((x1 - x0 + 31) // 32) * ((h + 31) // 32)
    counts = m["counts"][s["band"]]
    assert counts.size == nbins
    got = rendered(id)
    plan, wi, env = got["plan"], got["items"], s["env"]
    # (a) the plan is the function's answer for the context's inputs: a new scene's list, the item table sized afresh
    want = plan_of(got["L"], nbins=nbins, npix=(x1 - x0) * h, capacity=default_capacity(m["n"]), cus=_cus(), throughput=s["throughput"],
                   early_out=s["eps"] > 0, allocated=0, fuse_combine=env.get("GSR_FUSE_COMBINE", 1), long_items=env.get("GSR_LONG_ITEMS", -1),
                   blend_sub=env.get("GSR_BLEND_SUB", 0), blend_grid=env.get("GSR_BLEND_GRID", 0), seg_len=env.get("GSR_SEG_LEN", 0))
    assert plan == want, (id, plan, want)
    # (b) the fields the case is here for
    for field, value in s["named"].items():
        if isinstance(value, tuple):
            value = value[0] * _cus()
        assert plan[field] == value, (id, field, plan)
    assert plan["queue_start"] == min(plan["max_items"], plan["grid"])
    # (c) what k_bin_finalize published agrees with the plan
    assert wi["waves_per_tile"] == plan["waves_per_tile"] and wi["bins"] == nbins, (id, wi)
    if plan["whole_bin"]:
        assert wi["seg_len"] == plan["seg_len"] >= WHOLE_BIN_FROM and wi["items"] == nbins, (id, wi)      # the sentinel, published as it is
    else:
        assert wi["seg_len"] >= plan["seg_len"] and wi["seg_len"] % 256 == 0 and wi["seg_len"] < WHOLE_BIN_FROM, (id, wi)
    assert nbins <= wi["items"] <= plan["max_items"], (id, wi)
    if env.get("GSR_LONG_ITEMS") == "0":
        assert counts.max() > wi["seg_len"] and wi["items"] > nbins, (id, wi, counts.max())      # the long bin is cut
    # (d) the image against the oracle, within the bound of that kind of frame
    err = np.abs(got["img"][:, x0:x1].astype(np.float64) - m["oimg"][:, x0:x1].astype(np.float64)).max()
    print("%s: max |image - oracle| = %.3g, work items %r" % (id, err, wi))
    assert err <= (TOL_EARLY if s["eps"] > 0 else TOL_EXACT), (id, err)
    assert not got["overflow"] and got["overflow_frames"] == 0


def test_pairs_agree(rendered):
    """(e): the same frame through two plans"""
    img = lambda id: rendered(id)["img"]
    assert np.array_equal(img("GSR_FUSE_COMBINE=0 GSR_LONG_ITEMS=0"), img("default GSR_LONG_ITEMS=0"))      # fused and separate fold
    assert np.array_equal(img("GSR_BLEND_GRID=3"), img("default"))                                           # three workgroups draw every item
    d = np.abs(img("GSR_BLEND_SUB=1") - img("default")).max()                                                # one and two waves per tile
    print("one against two waves per tile: max difference %.3g" % d)
    assert d <= 2e-6, d
    d = np.abs(img("throughput GSR_BLEND_SUB=2") - img("throughput")).max()
    assert d <= 2e-6, d

"""The form launched is the form planned.

plan_sort (k_sort.hip) picks the radix sort's form for every frame and launch_sort launches from its answer alone
(tests/test_sort_plan.py asks the function itself, on the CPU).  Here every kind of context that takes another path
through the plan renders three frames of a small scene, and after each frame

  (a) the plan the frame was launched from (gsr_debug_last_sort_plan) equals what gsr_debug_sort_plan answers for the
      context's inputs and the largest-bucket word the frame before left in the mailbox -- computed from the ORACLE's keys,
      over the splats that frame sorted;
  (b) its form, carry and band are the ones the context is here for;
  (c) depthIndex equals the oracle's, entry for entry;
  (d) the bin lists equal tests/bin_reference.py's, entry for entry (with the rectangles carried through the sort, and
      gathered by the binning).

The scene: 2 x 2048 + 37 splats -- more than one radix workgroup, the last one partial -- of which twenty sit exactly on
another one's position, so that keys tie and the order among them is the index order; 256 x 128 pixels.  The outlier scene
(seven positions times 4000: the key range stretches and all other splats share one high-digit bucket) needs a bucket
above 48 << 10 keys to leave the bucket order, which 4133 splats cannot fill: it has 49 160, the smallest count at which
the n - 7 splats of that bucket exceed the limit.  Every comparison is an equality."""
import ctypes

import numpy as np
import pytest

import bin_reference as B
from test_gpu_bin_lists import _context
from test_sort_plan import BUCKET_NARROW, BUCKET_WIDE, LSD, NARROW, PLAN, WIDE

pytestmark = pytest.mark.gpu

W, H = 256, 128
FX = 1132.0 * W / 1920.0
POSES = (5, 6, 7)
N = 2 * 2048 + 37
N_OUTLIERS = (48 << 10) + 1 + 7
RIGHT_HALF = (128, 256)
NO_REPORT = 0xffffffff
GSR_ERR_ARG = -1   # include/gsplat_hip.h


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _scene(gh, oracle, kind):
    if kind == "outliers":
        data, pos = oracle.scene_pack(gh.synth.synth_rows(N_OUTLIERS, 11))
        p2 = np.array(pos, copy=True).reshape(-1, 3)
        p2[:7] *= 4000.0
        d2 = np.array(data, copy=True).reshape(-1, 8)
        d2[:, 0:3] = p2.view(np.uint32)                # (Scene.data words 0..2 are the position)
        return d2.reshape(-1), p2.reshape(-1)
    rows = np.array(gh.synth.synth_rows(N, 12)).reshape(-1, 32)
    twins = np.arange(20) * 215 + 11                  # twenty splats, spread over both full blocks and the partial one ...
    rows[twins, 0:12] = rows[(twins * 7 + 1000) % N, 0:12]      # ... each on the position of another
    return oracle.scene_pack(rows.reshape(-1))


@pytest.fixture(scope="module")
def frames(gh, oracle):
    """per scene: data, positions and, per pose, the oracle's order, keys, boxes (computed once, shared by the contexts)"""
    cache = {}

    def get(kind):
        if kind not in cache:
            data, pos = _scene(gh, oracle, kind)
            per_pose = []
            for k in POSES:
                cam = gh.orbit_camera(k, 120, W, H, FX)
                v, p, vp = cam.f32()
                odi, keys, _ = oracle.sort(vp, pos)
                per_pose.append(dict(cam=cam, odi=odi, keys=keys, obbox=oracle.project(data, v, p, cam.fx, cam.fy, W, H)[1]))
            cache[kind] = (data, pos, per_pose)
        return cache[kind]

    yield get
    cache.clear()


def _largest_bucket(keys, splats=None):
    """what a frame that sorted `splats` (all of them: None) leaves in the mailbox: the keys in its largest high-digit bucket"""
    k = keys if splats is None else keys[splats]
    return int(np.bincount(k >> 8, minlength=257).max()) if k.size else 0


def _last_plan(r):
    out = np.zeros(1, dtype=PLAN)
    fn = r._L.gsr_debug_last_sort_plan
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]
    rc = fn(r._ctx, out.ctypes.data)
    return rc, out[0]


def _planned(L, n, front, render, cull, largest, env):
    fn = L.gsr_debug_sort_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_uint,
                   ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    carry = int(env.get("GSR_RECT_CARRY", 1))
    out = np.zeros(1, dtype=PLAN)
    assert fn(n, n, front, render, cull, largest, -1, int(env.get("GSR_SORT_KPB", 0)), int(carry != 0), int(carry == 2), out.ctypes.data) == PLAN.itemsize
    return out[0]


def _case(id, scene="ties", env=None, throughput=False, band=None, forms=(LSD, BUCKET_WIDE, BUCKET_WIDE), carry=(1, 0, 0)):
    return pytest.param(scene, env or {}, throughput, band, forms, carry, id=id)


CONTEXTS = [
    _case("default"),
    _case("throughput", throughput=True, forms=(LSD, BUCKET_NARROW, BUCKET_NARROW)),
    _case("throughput GSR_SORT_KPB=4096", env={"GSR_SORT_KPB": "4096"}, throughput=True),           # no narrow kernel for 4096 keys: wide
    _case("default GSR_RECT_CARRY=2", env={"GSR_RECT_CARRY": "2"}, carry=(1, 1, 1)),
    _case("default GSR_RECT_CARRY=0", env={"GSR_RECT_CARRY": "0"}, carry=(0, 0, 0)),
    _case("band over the right half", band=RIGHT_HALF),
    _case("default, outliers fill one bucket", scene="outliers", forms=(LSD, LSD, LSD), carry=(1, 1, 1)),
]


@pytest.mark.parametrize("scene,env,throughput,band,forms,carry", CONTEXTS)
def test_the_form_launched_is_the_form_planned(gh, frames, monkeypatch, scene, env, throughput, band, forms, carry):
    data, pos, per_pose = frames(scene)
    n = pos.size // 3
    assert n == (N_OUTLIERS if scene == "outliers" else N)
    if scene == "outliers":     # the property the scene is here for, from the second frame's point of view and the third's
        assert all(_largest_bucket(f["keys"]) > 48 << 10 for f in per_pose[:2])
        assert _largest_bucket(per_pose[0]["keys"][:-1]) <= 48 << 10         # (one splat fewer would not do)
    else:
        assert all(np.unique(f["keys"]).size <= n - 20 for f in per_pose)    # the twins tie
    r = _context(gh, monkeypatch, W, H, env, throughput, band)
    r.set_raw_scene(data, pos)
    front = NARROW if throughput else WIDE
    assert _last_plan(r)[0] == GSR_ERR_ARG                  # no frame yet
    word = NO_REPORT
    for i, f in enumerate(per_pose):
        what = (scene, env, throughput, band, "frame %d" % (i + 1))
        r.render(None, f["cam"])
        rc, plan = _last_plan(r)
        want = _planned(r._L, n, front, 1, int(band is not None), word, env)
        assert rc == 0 and plan == want, (what, plan, want)                                           # (a)
        assert (plan["form"], plan["carry"], plan["band"]) == (forms[i], carry[i], int(band is not None)), (what, plan)      # (b)
        assert plan["waves"] == (NARROW if forms[i] == BUCKET_NARROW else WIDE) and plan["keys_per_block"] == int(env.get("GSR_SORT_KPB", 2048))
        want_s, want_l = B.bin_lists_reference(f["obbox"], f["odi"], W, H, band)
        starts, lst = r.bin_lists()
        assert want_l.size > 0 and np.array_equal(starts, want_s) and np.array_equal(lst, want_l), (what, B.first_difference(starts, lst, want_s, want_l, f["obbox"]))   # (d)
        word = _largest_bucket(f["keys"], np.unique(want_l) if band else None)      # a band frame sorted the splats that enter its bins
        assert np.array_equal(r.lastDepthIndex(), f["odi"]), what                                      # (c)
        if band:    # the whole permutation of a band context is a sort-only frame behind the render frame: planned like any other
            rc, plan = _last_plan(r)
            want = _planned(r._L, n, front, 0, 1, word, env)
            assert rc == 0 and plan == want and (plan["band"], plan["carry"]) == (0, 0), (what, plan, want)
            word = _largest_bucket(f["keys"])
    assert not r.overflow_pending()
    r.dispose()

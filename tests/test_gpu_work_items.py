"""Every frame's compositor work list against an exact reference.

The finalize step of the binning stage (bin_finalize_body, k_bin.hip) publishes what the compositor draws from: the items (four
words each), seg_start, the segment length and the item count, cut from four figures of the frame (visible splats, tile
overlaps, optical depth, optical mass).  The image cannot see most of what can go wrong there -- another cut changes f32
association by 2e-6 and the speed by a third -- so here the device's list is read back (HIPRenderer.work_list / frame_figures) and
compared with tests/work_items_reference.py, which is fed by the ORACLE's boxes, axes and depth order and by the compositor plan,
never by a device read-back: the figures equal (the optical mass inside its derived interval), every decision equal, seg_start
word for word, the item set equal, the order rule met, and what k_blend relies on of every item.

The cases, the branch of the policy each is there for and the variant of the step it runs are tests/test_work_items_reference.py's
(checked there on the CPU, with the condition that the optical mass interval decides nothing).  Every context renders two poses:
the second frame's figures prove that the step reset the frame slots."""
import ctypes
import os

import numpy as np
import pytest

import bin_reference as B
import work_items_reference as R
from test_blend_plan import PLAN, default_capacity
from test_work_items_reference import (BOUNDS_TOUR, BY_ID, CASE_IDS, KNOBS, OVERFLOW_CASE, POSES, bin_form, expected, fx_of, scene_of,
                                       work_frames)      # noqa: F401 (work_frames is a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
MASS_POSITION = []      # (device omass - omass_lo) / (omass_hi - omass_lo) of every frame whose interval is not a point


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _context(gh, monkeypatch, case, lib_path=None):
    """a context created under exactly the knobs of the case (all knobs are read once, by gsr_create)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    W, H = case["size"]
    r = gh.HIPRenderer(W, H, early_out_eps=case["eps"], band=case["band"], throughput=case["throughput"], lib_path=lib_path)
    for k in case["env"]:
        monkeypatch.delenv(k)
    return r


def _last_plan(r):
    out = np.zeros(1, dtype=PLAN)
    fn = r._L.gsr_debug_last_blend_plan
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]
    assert fn(r._ctx, out.ctypes.data) == 0
    return out[0]


def check_frame(r, case, fr, capacity, what):
    """the context's last frame against the reference; returns cut()'s answer"""
    plan = _last_plan(r)
    a, b, counts, fig = expected(case, fr, plan, capacity)
    nbins = counts.size
    got, wi, st = r.frame_figures(), r.work_items(), r.stats()
    items, seg_start = r.work_list(plan["max_items"])
    print("%s: figures %r, reference %r, seg_len %d, %d items, long_from %d" % (what, got, fig, wi["seg_len"], wi["items"], got["long_from"]))
    # the figures
    assert (got["visible"], got["tiles"], got["otiles"]) == (fig["V"], fig["D"], fig["otiles"]), (what, got, fig)
    assert (st["visible"], st["tile_entries"]) == (fig["V"], fig["D"]), (what, st)
    assert fig["omass_lo"] <= got["omass"] <= fig["omass_hi"], (what, got["omass"], fig)
    if fig["omass_hi"] > fig["omass_lo"]:
        MASS_POSITION.append((got["omass"] - fig["omass_lo"]) / (fig["omass_hi"] - fig["omass_lo"]))
    # what the step decided
    for k, dev in (("E", got["entries"]), ("mxbin", got["mxbin"]), ("dense", got["dense"]), ("heavy", got["heavy"]), ("long_from", got["long_from"]),
                   ("by_size", got["by_size"]), ("fits", got["fits"]), ("seg_len", wi["seg_len"]), ("n_items", wi["items"])):
        assert dev == a[k] == b[k], (what, k, dev, a[k], b[k])
    assert wi["bins"] == nbins
    # the starts and the list
    assert np.array_equal(seg_start, a["seg_start"]), (what, "seg_start")
    starts = r.bin_lists()[0]
    assert np.array_equal(starts, a["bin_start"]), (what, "bin_start")
    bad = R.check_work_list(items, seg_start, a, nbins, capacity, int(plan["max_items"]))
    assert bad is None, (what, bad)
    return a


def run_case(gh, monkeypatch, work_frames, scenes, id, lib_path=None):
    case = BY_ID[id]
    W, H = case["size"]
    data, pos = scene_of(scenes, case)
    r = _context(gh, monkeypatch, case, lib_path)
    try:
        r.set_raw_scene(data, pos)
        n = pos.size // 3
        form = bin_form(r._L, case, n, r.device_info()["compute_units"])["form"]
        assert form == case["form"], (id, form)                                   # the variant of the step this context runs
        for i, pose in enumerate(POSES):
            r.render(None, gh.orbit_camera(pose, 120, W, H, fx_of(gh, case)))
            a = check_frame(r, case, work_frames(case, pose), default_capacity(n), (id, "pose %d" % pose))
            assert a["fits"] and not r.overflow_pending() and r.stats()["overflow_frames"] == 0
            if case["records"] and i == 0:
                r.read_records()                                                  # the projection once more, outside a frame: it must fold nothing
    finally:
        r.dispose()


@pytest.mark.parametrize("id", CASE_IDS)
def test_work_list_is_the_reference(gh, monkeypatch, work_frames, scenes, id):
    run_case(gh, monkeypatch, work_frames, scenes, id)


def test_a_frame_that_does_not_fit_publishes_nothing(gh, monkeypatch, work_frames, scenes):
    """The project's own overflow path (tests/test_gpu_parity.py, test_list_overflow_is_sticky_counted_and_repaired): a list too small
    for the frame, the frame enqueued without repair -- no items, every start zero, the overflow raised -- and after gsr_sync's
    regrowth the full check passes."""
    case = BY_ID[OVERFLOW_CASE]
    W, H = case["size"]
    data, pos = scene_of(scenes, case)
    fr = work_frames(case, POSES[0])
    need = int(fr.of(None)[0][-1])
    small = 65536
    assert need > small
    r = _context(gh, monkeypatch, case)
    try:
        r.set_raw_scene(data, pos)
        r.set_list_capacity(small)
        r.set_camera(gh.orbit_camera(POSES[0], 120, W, H, fx_of(gh, case)))
        r.render_async()
        plan = _last_plan(r)
        a = expected(case, fr, plan, small)[0]
        assert not a["fits"] and a["n_items"] == 0 and a["items_needed"] <= plan["max_items"]      # the entries are the cause
        got = r.frame_figures()
        items, seg_start = r.work_list(plan["max_items"])
        assert not got["fits"] and got["entries"] == need and r.work_items()["items"] == 0 and items.shape[0] == 0
        assert not seg_start.any() and not r.bin_lists()[0].any()
        assert (got["long_from"], got["dense"], got["heavy"]) == (a["long_from"], a["dense"], a["heavy"])
        assert r.overflow_pending()
        r.sync()                                                                  # regrowth, the same frame again
        assert not r.overflow_pending() and r.stats()["overflow_frames"] == 1 and r.stats()["dropped_frames"] == 0
        check_frame(r, case, fr, max(small, need + (need >> 2) + (1 << 20)), "after the repair")
    finally:
        r.dispose()


def test_read_backs_refuse_what_is_not_the_last_frame(gh, monkeypatch, scenes):
    case = BY_ID["C1 default: one item per bin"]
    W, H = case["size"]
    data, pos = scene_of(scenes, case)
    r = _context(gh, monkeypatch, case)
    try:
        r.set_raw_scene(data, pos)
        cam = gh.orbit_camera(3, 120, W, H, fx_of(gh, case))

        def refused():
            for call in (r.frame_figures, lambda: r.work_list(4096)):
                with pytest.raises(gh.GsplatError) as e:
                    call()
                assert e.value.code == -1, e.value                                # GSR_ERR_ARG
        r.set_camera(cam)
        refused()                                                                 # no frame yet
        r.render(None, cam)
        assert r.work_list(4096)[0].shape == (300, 4)
        with pytest.raises(gh.GsplatError):
            r.work_list(299)                                                      # the caller's items are too small
        r.sort(cam)
        refused()                                                                 # the last frame was sort-only
        r.render(None, cam)
        r.set_band(64, 256)
        refused()                                                                 # the band changed
        r.render(None, cam)
        assert r.work_list(4096)[0].shape == (6 * 15, 4)
        r.set_list_capacity(1 << 21)
        refused()                                                                 # the list buffers changed
        r.render(None, cam)
        r.setSize(320, 240)
        refused()                                                                 # the size changed
    finally:
        r.dispose()


def test_bounds_checked_build(gh, monkeypatch, work_frames, scenes):
    """three of the contexts on the build that counts every index derived from device data outside what it indexes
    (tests/test_gpu_bounds.py): the same lists, every counter zero"""
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    for id in BOUNDS_TOUR:
        run_case(gh, monkeypatch, work_frames, scenes, id, lib_path=BOUNDS_LIB)
    L = gh.load_library(BOUNDS_LIB)
    for name in ("bin", "sort", "blend"):
        buf = (ctypes.c_uint32 * 8)()
        assert getattr(L, "gsr_debug_bounds_" + name)(buf) == 0
        assert not any(buf), (name, list(buf))


def test_where_the_device_mass_lies_in_its_interval():
    """(last in the file) a figure, not a bound: the bound is the interval itself, asserted of every frame above"""
    if MASS_POSITION:
        print("optical mass: (device - omass_lo) / (omass_hi - omass_lo) over %d frames: min %.3f, max %.3f" % (len(MASS_POSITION), min(MASS_POSITION), max(MASS_POSITION)))
        assert 0.0 <= min(MASS_POSITION) and max(MASS_POSITION) <= 1.0

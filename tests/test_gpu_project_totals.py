"""The workgroup totals of k_project_key (k_project.hip: wave_total, the ballot count of the visible splats) against numpy.

The projection folds six per-lane values into its workgroup's frame slot: the depth minimum and maximum (the sort's key range),
the visible splats, the 16x16 tiles of their boxes, the optical depth over the boxes and the optical mass.  They are integer
minima, maxima and sums, so the order of the fold cannot be seen in them -- a wrong fold can.  Small frames (64x64, 96x64) and
scenes of N = 1, 63, 64, 65, 255, 257, 1000 splats: a single lane, partial waves, whole waves, a partial workgroup, more than one
workgroup and frame slot.  Of every scene some splats are culled (behind the camera, outside the 1.2 clip), some are hidden
through gsr_hide_selected and some have boxes that cover the whole frame.

What is compared, on a default and on a throughput context:
    stats() visible / tile_entries and frame_figures() visible / tiles / otiles   equal to work_items_reference.frame_figures fed
                                                                                   with the ORACLE's boxes (hidden ones made invisible)
    frame_figures() omass                 inside the reference's interval (it rests on an approximate square root) and equal to a
                                          second context's of the same frame
    lastDepthIndex()                      equal to oracle.sort: the counting sort's keys rest on the folded minimum and maximum
    work_items() and frame_figures()      equal to those of a second context given the same frame"""
import numpy as np
import pytest

import hide_reference as HR
import work_items_reference as R

pytestmark = pytest.mark.gpu

SIZES = ((64, 64), (96, 64))
COUNTS = (1, 63, 64, 65, 255, 257, 1000)
POSE, FX, SEED = 3, 60.0, 11
KINDS = {"default": {}, "throughput": {"throughput": True}}


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _cam(gh, W, H):
    return gh.orbit_camera(POSE, 120, W, H, FX)


def _rows(gh, n, cam):
    """a seeded blob with, by index: i % 7 == 3 behind the camera, i % 5 == 2 far to the side (outside the 1.2 clip), i % 11 == 4 a
    splat near the centre that is larger than the frame; returns (rows, hidden) with hidden = i % 3 == 1"""
    r = np.array(gh.synth.synth_rows(n, SEED, sigma=1.5, s_lo=0.01, s_hi=0.3), dtype=np.uint8).reshape(-1, 32)
    pos = r[:, 0:12].copy().view(np.float32).reshape(-1, 3)
    scale = r[:, 12:24].copy().view(np.float32).reshape(-1, 3)
    i = np.arange(n)
    eye = np.asarray(cam.position, dtype=np.float32)
    big, side, behind = i % 11 == 4, i % 5 == 2, i % 7 == 3
    pos[big] *= np.float32(0.1)
    scale[big] = np.float32(20.0)
    pos[side] += np.asarray((0.0, 40.0, 0.0), dtype=np.float32)
    pos[behind] = pos[behind] * np.float32(0.1) + eye * np.float32(1.5)
    r[:, 0:12] = pos.view(np.uint8).reshape(-1, 12)
    r[:, 12:24] = scale.view(np.uint8).reshape(-1, 12)
    return r.reshape(-1), i % 3 == 1


class Frames:
    """the oracle's statement of every (size, N): rows, hidden set, figures, depth order; computed once, shared, never changed"""

    def __init__(self, oracle, gh):
        self.by = {}
        for W, H in SIZES:
            cam = _cam(gh, W, H)
            v, p, vp = cam.f32()
            for n in COUNTS:
                rows, hid = _rows(gh, n, cam)
                data, pos = oracle.scene_pack(rows)
                _, bbox, raw = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
                bbox = np.asarray(bbox).reshape(-1, 4)
                order = oracle.sort(vp, pos)[0]
                listed = (bbox[:, 0] <= bbox[:, 2]) & (bbox[:, 1] <= bbox[:, 3])
                whole = listed & (bbox[:, 0] == 0) & (bbox[:, 1] == 0) & (bbox[:, 2] == W - 1) & (bbox[:, 3] == H - 1)
                i = np.arange(n)
                assert not listed[(i % 7 == 3) | (i % 5 == 2)].any()                     # both culls cull
                if n >= 63:                                                              # no side of the scene is vacuous
                    assert (~listed).sum() > 0 and (listed & hid).sum() > 0 and (listed & ~hid).sum() > 0 and (whole & ~hid).sum() > 0, (W, H, n)
                fig = R.frame_figures(data, HR.hide_bbox(bbox, hid), raw, W, H)
                assert fig["V"] == int((listed & ~hid).sum())
                for a in (rows, hid, order):
                    a.flags.writeable = False
                self.by[(W, H, n)] = dict(rows=rows, hid=hid, order=order, fig=fig)


@pytest.fixture(scope="module")
def frames(oracle, gh):
    return Frames(oracle, gh)


def _render(gh, r, fr, W, H):
    r.set_scene_rows(fr["rows"])
    r.set_selection(fr["hid"])
    assert r.hide_selected("replace") == int(fr["hid"].sum())
    r.render(None, _cam(gh, W, H))
    assert r.stats()["overflow_frames"] == 0 and not r.overflow_pending()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_totals_are_the_sums_over_the_oracles_boxes(gh, frames, size, kind):
    W, H = size
    r, twin = gh.HIPRenderer(W, H, **KINDS[kind]), gh.HIPRenderer(W, H, **KINDS[kind])
    try:
        for n in COUNTS:
            fr = frames.by[(W, H, n)]
            fig = fr["fig"]
            _render(gh, r, fr, W, H)
            got, st, wi = r.frame_figures(), r.stats(), r.work_items()
            print("%dx%d %s n=%d: device %r, reference %r" % (W, H, kind, n, got, fig))
            assert (st["visible"], st["tile_entries"]) == (fig["V"], fig["D"]), (n, st, fig)
            assert (got["visible"], got["tiles"], got["otiles"]) == (fig["V"], fig["D"], fig["otiles"]), (n, got, fig)
            assert fig["omass_lo"] <= got["omass"] <= fig["omass_hi"], (n, got["omass"], fig)
            assert np.array_equal(r.lastDepthIndex(), fr["order"]), n
            _render(gh, twin, fr, W, H)
            assert twin.work_items() == wi and twin.frame_figures() == got, (n, wi, twin.work_items(), got, twin.frame_figures())
    finally:
        r.dispose()
        twin.dispose()

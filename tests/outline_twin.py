"""What tests/test_gpu_outline.py runs on the shipped build in its own process and on the bounds-checked build in a child: the
outlined overlay of C1, of an odd size and of a band context, for a wide outer and a narrow inner outline, as digests.  The
selections are that test's: every second splat, and for the wide outer outline the sparse one of each set-up (C1 and the band: the
region; the odd size: every 32nd splat).  main() also prints the bounds-checked build's counters (every site must stay 0)."""
import ctypes
import hashlib

import numpy as np

W, H = 640, 480
TINT, MIX = (1.0, 0.5, 0.0), 0.5
REGION = (200, 150, 420, 330)
# (rgb, alpha, threshold, width, side), and whether the case runs on the set-up's sparse selection
OUTLINES = ((((0.125, 7.0, -3.0), 0.4, 0.25, 16, "outer"), True), (((0.125, 7.0, -3.0), 1.0, 0.25, 3, "inner"), False),
            (((1.0, 1.0, 1.0), 1.0, 0.05, 1, "outer"), False), (((0.125, 7.0, -3.0), 0.4, 0.25, 16, "inner"), False))


def _run(gh, r, cam, dense, sparse):
    r.set_overlay(TINT, MIX)
    r.set_camera(cam)
    r.render_async()
    r.sync()
    h = hashlib.sha256()
    for o, on_sparse in OUTLINES:
        (sparse if on_sparse else dense)(r)
        r.set_overlay_outline(*o)
        rgba, cover = r.read_overlay()
        h.update(rgba.tobytes() + cover.tobytes())
    return h.hexdigest()


def cases(gh):
    """(name, renderer, camera, dense selection, sparse selection) one at a time; the caller disposes"""
    cfg = gh.synth.CONFIGS["C1"]
    n = cfg["n"]
    every = lambda count, k: (lambda r: r.set_selection(np.arange(count) % k == 0))
    region = lambda r: r.select_region(REGION)
    r = gh.HIPRenderer(W, H)
    r.set_scene_rows(gh.synth.config_rows("C1"))
    yield "C1", r, gh.orbit_camera(3, width=W, height=H, fx=cfg["fx"]), every(n, 2), region
    r = gh.HIPRenderer(333, 207)
    r.set_scene_rows(gh.synth.synth_rows(1025, 7))
    yield "odd", r, gh.orbit_camera(3, width=333, height=207, fx=cfg["fx"] * 333 / W), every(1025, 2), every(1025, 32)
    r = gh.HIPRenderer(W, H, band=(192, 448))
    r.set_scene_rows(gh.synth.config_rows("C1"))
    yield "band", r, gh.orbit_camera(3, width=W, height=H, fx=cfg["fx"]), every(n, 2), region


def digests(gh, counters=False):
    out = {}
    for name, r, cam, dense, sparse in cases(gh):
        out[name] = _run(gh, r, cam, dense, sparse)
        if counters:
            for fn in ("gsr_debug_bounds_overlay", "gsr_debug_bounds_depth", "gsr_debug_bounds_select"):
                buf = (ctypes.c_uint32 * 8)()
                assert getattr(r._L, fn)(buf) == 0
                print("bounds", name, fn, list(buf))
                assert not any(buf), (name, fn, list(buf))
        r.dispose()
    return out


def main():
    import gsplat_hip as gh
    for name, d in digests(gh, counters=True).items():
        print("digest", name, d)
    print("done")

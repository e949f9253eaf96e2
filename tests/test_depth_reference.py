"""The depth planes' specification (tests/depth_reference.py) on cases whose answer is known without it, and the surface
the feature adds to the three hosts.  No GPU: the reference is fed by the oracle."""
import os
import re

import numpy as np

import depth_reference as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH_SYMBOLS = ("gsr_set_hit_alpha", "gsr_depth_async", "gsr_read_depth", "gsr_depth_device_ptr", "gsr_pick")
W, H = 128, 96


def _rows(splats):
    rows = np.zeros((len(splats), 32), dtype=np.uint8)
    for i, s in enumerate(splats):
        rows[i, 0:12] = np.asarray(s["pos"], dtype=np.float32).view(np.uint8)
        rows[i, 12:24] = np.asarray(s["scale"], dtype=np.float32).view(np.uint8)
        rows[i, 24:28] = s["rgba"]
        rows[i, 28:32] = (255, 128, 128, 128)
    return rows.reshape(-1)


def _planes(oracle, splats, hit_alpha=0.5):
    """planes of a few splats seen from (0, 0, -5) looking down +z: (planes, z per splat, pixel boxes)"""
    import gsplat_hip as gh
    cam = gh.Camera(position=(0.0, 0.0, -5.0), fx=200.0, fy=200.0)
    cam.update(W, H)
    v, p, vp = cam.f32()
    data, pos = oracle.scene_pack(_rows(splats))
    rec, bbox, raw = oracle.project(data, v, p, cam.fx, cam.fy, W, H)
    order = oracle.sort(vp, pos)[0]
    return DR.depth_planes_reference(rec, bbox, raw[:, 10], order, W, H, hit_alpha=hit_alpha), raw[:, 10], bbox


def _centre(bbox, i):
    return (int(bbox[i, 1] + bbox[i, 3]) // 2, int(bbox[i, 0] + bbox[i, 2]) // 2)   # (row, column)


def test_one_opaque_splat(oracle):
    pl, z, bbox = _planes(oracle, [dict(pos=(0, 0, 0), scale=(0.3, 0.3, 0.3), rgba=(255, 0, 0, 255))])
    assert abs(float(z[0]) - 5.0) < 1e-5
    c = _centre(bbox, 0)
    assert pl["index"][c] == 0 and pl["hit"][c] == z[0]
    assert pl["alpha"][c] > 0.9
    assert abs(pl["mean"][c] / pl["alpha"][c] - float(z[0])) < 1e-9          # one fragment: expected depth is its depth
    covered = pl["alpha"] > 0
    assert np.all(np.abs(pl["mean"][covered] / pl["alpha"][covered] - float(z[0])) < 1e-9)
    assert pl["index"][0, 0] == DR.NONE and np.isinf(pl["hit"][0, 0]) and pl["mean"][0, 0] == 0.0   # an empty pixel
    # the hit region is where alpha reaches one half: inside the covered region, not all of it
    assert 0 < int((pl["index"] == 0).sum()) < int(covered.sum())
    assert pl["mask"].mean() < 0.01


def test_two_overlapping_splats_in_both_orders(oracle):
    near = dict(pos=(0, 0, -1), scale=(0.2, 0.2, 0.2), rgba=(0, 255, 0, 255))
    far = dict(pos=(0, 0, 1), scale=(0.4, 0.4, 0.4), rgba=(0, 0, 255, 255))
    for splats, i_near in (([near, far], 0), ([far, near], 1)):
        pl, z, bbox = _planes(oracle, splats)
        i_far = 1 - i_near
        assert z[i_near] < z[i_far]
        c = _centre(bbox, i_near)
        assert pl["index"][c] == i_near and pl["hit"][c] == z[i_near]        # the nearer splat, whatever its index
        assert float(z[i_near]) < pl["mean"][c] / pl["alpha"][c] < float(z[i_far])
        ring = (pl["index"] == i_far)
        assert ring.any()                                                    # the far splat is hit where the near one does not reach
        assert np.all(pl["hit"][ring] == z[i_far])


def test_translucent_stack_never_hits(oracle):
    stack = [dict(pos=(0, 0, k * 0.5), scale=(0.3, 0.3, 0.3), rgba=(200, 200, 200, 20)) for k in range(4)]
    pl, z, bbox = _planes(oracle, stack)
    assert 0.1 < pl["alpha"].max() < 0.5
    assert np.all(pl["index"] == DR.NONE) and np.all(np.isinf(pl["hit"]))
    c = _centre(bbox, 0)
    assert float(z.min()) < pl["mean"][c] / pl["alpha"][c] < float(z.max())
    # a lower threshold is reached
    pl2, _, _ = _planes(oracle, stack, hit_alpha=0.1)
    assert (pl2["index"] != DR.NONE).any()


def test_alpha_of_the_reference_is_the_oracles(oracle, scenes):
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C1"]
    _, data, pos = scenes("C1")
    w, h = cfg["width"], cfg["height"]
    cam = gh.orbit_camera(3, width=w, height=h, fx=cfg["fx"])
    v, p, vp = cam.f32()
    rec, bbox, raw = oracle.project(data, v, p, cam.fx, cam.fy, w, h)
    order = oracle.sort(vp, pos)[0]
    pl = DR.depth_planes_reference(rec, bbox, raw[:, 10], order, w, h)
    img = oracle.render(order, raw, rec, bbox, w, h, mode=1)
    assert np.abs(pl["alpha"] - img[..., 3].astype(np.float64)).max() <= 1e-6
    assert pl["mask"].mean() < 0.01
    hit = pl["index"] != DR.NONE
    assert hit.any() and np.array_equal(pl["hit"][hit], raw[pl["index"][hit], 10])
    assert np.all(pl["alpha"][hit] >= 0.5) and np.all(pl["alpha"][~hit & ~pl["mask"]] < 0.5)


# ---- the surface ----
def test_header_and_exports_name_the_depth_functions():
    import gsplat_hip as gh
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name in DEPTH_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in gh.EXPORTS, name
    assert "gsr_pick_result" in header
    lib = gh.load_library()
    for name in DEPTH_SYMBOLS:
        assert hasattr(lib, name), name
    for method in ("set_hit_alpha", "depth_async", "read_depth", "pick"):
        assert callable(getattr(gh.HIPRenderer, method))


def test_typescript_declares_the_depth_methods():
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for name in ("readDepth", "pick", "setHitAlpha"):
        assert re.search(r"\b%s\s*\(" % name, dts), name


def test_knob_and_kernels_are_in_the_library():
    import subprocess
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    for s in ("k_depth_planes", "k_pick", "GSR_DEPTH_SKIP"):
        assert s in out, s


def test_depth_unit_instantiates_the_walk_and_keeps_its_check_sites():
    from walk_source import CSRC, walk_sites_are_checked
    src = open(os.path.join(CSRC, "k_depth.hip")).read()
    assert "GSR_BOUNDS_DECL(depth)" in src
    walk_sites_are_checked(src, "depth", "DepthBounds", "DepthPass")    # bin, list position, splat index, LDS cell: in the walk the unit instantiates
    for site in (4, 5):                                                 # query pixel, sample of a strided hit plane: the unit's own
        assert re.search(r"GSR_BOUND\(depth, %d," % site, src), site

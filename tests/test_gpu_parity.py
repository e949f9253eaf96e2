"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle.

Bars:
  sort        depthIndex bit-exact (u32 array equality), keys and min/max too
  projection  every record field and bounding box bit-exact, log2(opacity) within 2 ulp-ish (v_log_f32)
  image       max |HIP f32 - oracle f64-accumulated| <= 2e-4 per premultiplied channel with early-out
              disabled, <= 1e-3 with early-out at 1e-4; RGBA8 within +-1 LSB
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_EXACT = 2e-4
TOL_EARLY = 1e-3


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _camera(gh, k, cfg):
    return gh.orbit_camera(k, width=cfg["width"], height=cfg["height"], fx=cfg["fx"])


SMALL = dict(width=640, height=480, fx=1132.0)


@pytest.mark.parametrize("n,seed", [(1, 11), (63, 12), (64, 13), (4096, 1), (70000, 2), (300000, 5)])
def test_sort_bit_exact(gh, oracle, scenes, n, seed):
    rows, data, pos = scenes(n, seed)
    r = gh.HIPRenderer(640, 480)
    r.set_raw_scene(data, pos)
    for k in (0, 17, 63):
        cam = _camera(gh, k, SMALL)
        r.sort(cam)
        di = r.lastDepthIndex()
        keys, mm = r.read_keys()
        odi, okeys, omm = oracle.sort(cam.f32()[2], pos)
        assert mm == omm
        assert np.array_equal(keys, okeys)
        assert np.array_equal(di, odi)
    r.dispose()


def test_sort_ties_and_max_bucket(gh, oracle):
    # G2: >= 3 splats tie at maxDepth (key 65536) and many ties elsewhere: stable order by index
    rng = np.random.default_rng(7)
    n = 5000
    pos = rng.integers(-8, 9, size=(n, 3)).astype(np.float32) * 0.25
    pos[[10, 200, 4000]] = [0.0, 0.0, 50.0]
    data = np.zeros((n, 8), dtype=np.uint32)
    data[:, 0:3] = pos.view(np.uint32)
    vp = np.zeros(16, dtype=np.float32)
    vp[10] = 1.0
    r = gh.HIPRenderer(64, 64)
    r.set_raw_scene(data, pos)
    L = r._L
    ident = np.eye(4, dtype=np.float32).reshape(-1)
    r._check(L.gsr_set_camera(r._ctx, ident.ctypes.data, ident.ctypes.data, vp.ctypes.data, 1.0, 1.0))
    r.sort()
    odi, okeys, _ = oracle.sort(vp, pos)
    assert int((okeys == 65536).sum()) >= 3
    assert np.array_equal(r.read_keys()[0], okeys)
    assert np.array_equal(r.lastDepthIndex(), odi)
    r.dispose()


def test_sort_degenerate_all_equal_depth(gh, oracle):
    n = 1000
    pos = np.zeros((n, 3), dtype=np.float32)
    data = np.zeros((n, 8), dtype=np.uint32)
    r = gh.HIPRenderer(64, 64)
    r.set_raw_scene(data, pos)
    r.sort(gh.orbit_camera(3, width=64, height=64))
    assert np.array_equal(r.lastDepthIndex(), np.arange(n, dtype=np.uint32))
    r.dispose()


def _compare_records(rec, bbox, orec, obbox, oraw):
    assert np.array_equal(bbox, obbox)
    vis = oraw[:, 11] == 1.0
    a, b = rec[vis], orec[vis]
    for col in (0, 1, 2, 3, 4, 5, 7):
        assert np.array_equal(a[:, col].view(np.uint32), b[:, col].view(np.uint32)), "record column %d" % col
    la, lb = a[:, 6], b[:, 6]
    fin = np.isfinite(lb)
    assert np.array_equal(np.isfinite(la), fin)
    assert np.all(np.abs(la[fin] - lb[fin]) <= 4e-6 * np.maximum(1.0, np.abs(lb[fin])))


@pytest.mark.parametrize("name,k", [("C1", 0), ("C1", 40), ("C2", 7)])
def test_projection_bit_exact(gh, oracle, scenes, name, k):
    cfg = gh.synth.CONFIGS[name]
    rows, data, pos = scenes(name)
    cam = _camera(gh, k, cfg)
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_raw_scene(data, pos)
    r.set_camera(cam)
    r.render_async(); r.sync()
    rec, bbox = r.read_records()
    v, p, vp = cam.f32()
    orec, obbox, oraw = oracle.project(data, v, p, cfg["fx"], cfg["fx"], cfg["width"], cfg["height"])
    _compare_records(rec, bbox, orec, obbox, oraw)
    r.dispose()


def _render_pair(gh, oracle, data, pos, cam, W, H, eps=0.0, band=None, throughput=False):
    r = gh.HIPRenderer(W, H, early_out_eps=eps, band=band, throughput=throughput)
    r.set_raw_scene(data, pos)
    r.set_camera(cam)
    r.render_async(); r.sync()
    img = r.readPixelsFloat()
    img8 = r.readPixels()
    di = r.lastDepthIndex()
    st = r.stats()
    r.dispose()
    v, p, vp = cam.f32()
    oimg, odi, V, D = oracle.render_scene(data, pos, v, p, vp, cam.fx, cam.fy, W, H, mode=1)
    return img, img8, di, st, oimg, odi, V, D


@pytest.mark.parametrize("name,k", [("C1", 0), ("C1", 77), ("C2", 13)])
def test_image_parity_exact_mode(gh, oracle, scenes, name, k):
    cfg = gh.synth.CONFIGS[name]
    rows, data, pos = scenes(name)
    cam = _camera(gh, k, cfg)
    img, img8, di, st, oimg, odi, V, D = _render_pair(gh, oracle, data, pos, cam, cfg["width"], cfg["height"])
    assert np.array_equal(di, odi)
    assert st["visible"] == V and st["tile_entries"] == D   # the bench's byte model uses these device counters
    err = np.abs(img.astype(np.float64) - oimg.astype(np.float64)).max()
    assert err <= TOL_EXACT, err
    o8 = np.floor(np.clip(oimg.astype(np.float64), 0, 1) * 255.0 + 0.5).astype(np.int32)
    assert np.abs(img8.astype(np.int32) - o8).max() <= 1


def test_image_parity_throughput_flag(gh, oracle, scenes):
    # GSR_FLAG_THROUGHPUT changes only how a bin's list is cut into work items (2048 instead of 512 entries)
    cfg = gh.synth.CONFIGS["C2"]
    rows, data, pos = scenes("C2")
    cam = _camera(gh, 13, cfg)
    img, img8, di, st, oimg, odi, V, D = _render_pair(gh, oracle, data, pos, cam, cfg["width"], cfg["height"], throughput=True)
    assert np.array_equal(di, odi)
    assert st["visible"] == V and st["tile_entries"] == D
    err = np.abs(img.astype(np.float64) - oimg.astype(np.float64)).max()
    assert err <= TOL_EXACT, err


def test_image_parity_early_out(gh, oracle, scenes):
    cfg = gh.synth.CONFIGS["C2"]
    rows, data, pos = scenes("C2")
    cam = _camera(gh, 30, cfg)
    img, img8, di, st, oimg, odi, V, D = _render_pair(gh, oracle, data, pos, cam, cfg["width"], cfg["height"], eps=1e-4)
    err = np.abs(img.astype(np.float64) - oimg.astype(np.float64)).max()
    assert err <= TOL_EARLY, err


def test_image_odd_size_and_empty_scene(gh, oracle, scenes):
    # W, H not multiples of the 16-px tile / 32-px bin; and N = 0
    rows, data, pos = scenes(20000, 21)
    cam = gh.orbit_camera(9, width=333, height=201, fx=400.0)
    img, img8, di, st, oimg, odi, V, D = _render_pair(gh, oracle, data, pos, cam, 333, 201)
    assert np.abs(img.astype(np.float64) - oimg).max() <= TOL_EXACT
    r = gh.HIPRenderer(100, 50)
    r.set_raw_scene(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32))
    r.set_camera(gh.orbit_camera(0, width=100, height=50))
    r.render_async(); r.sync()
    assert not r.readPixelsFloat().any()
    r.dispose()


def test_large_framebuffer_sliced_binning(gh, oracle, scenes):
    # above 4096 bins the binning runs in two levels (cells of 4 x 4 bins, then every cell list's chunks into the cell's bins):
    # 192 x 101 bins = 48 x 26 cells here, k_cell_scatter1<8>; same image, same permutation.  (The one-level pass that cuts such
    # a grid into sub-grids and count row slices runs only with GSR_BIN_TWO_LEVEL=0: tests/test_gpu_bin_lists.py.)
    W, H = 6144, 3216
    rows, data, pos = scenes(30000, 33)
    cam = gh.orbit_camera(17, width=W, height=H, fx=3600.0)
    img, img8, di, st, oimg, odi, V, D = _render_pair(gh, oracle, data, pos, cam, W, H)
    assert np.array_equal(di, odi)
    assert st["visible"] == V and st["tile_entries"] == D
    err = np.abs(img.astype(np.float64) - oimg.astype(np.float64)).max()
    assert err <= TOL_EXACT, err
    # the largest framebuffer the ABI accepts renders too (256 x 256 bins = 64 x 64 cells, the only grid of k_cell_scatter1<4>):
    # its lists are the reference's, entry for entry
    import bin_reference
    r = gh.HIPRenderer(8192, 8192)
    r.set_raw_scene(data, pos)
    cam = gh.orbit_camera(17, width=8192, height=8192, fx=4800.0)
    r.set_camera(cam)
    r.render_async(); r.sync()
    assert r.stats()["visible"] > 0 and r.bin_totals().shape == (256, 256)
    v, p, vp = cam.f32()
    obbox = oracle.project(data, v, p, cam.fx, cam.fy, 8192, 8192)[1]
    want_starts, want_list = bin_reference.bin_lists_reference(obbox, oracle.sort(vp, pos)[0], 8192, 8192)
    starts, lst = r.bin_lists()
    assert bin_reference.first_difference(starts, lst, want_starts, want_list, obbox) is None
    assert r.stats()["visible"] == bin_reference.visible_reference(obbox, 8192, 8192) and r.stats()["bin_entries"] == want_list.size > 0
    r.dispose()


def test_band_split_equals_full_frame(gh, oracle, scenes):
    # multi-GPU partition: the union of the tile-column bands is the full frame, bit for bit
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    cam = _camera(gh, 5, cfg)
    W, H = cfg["width"], cfg["height"]
    full = _render_pair(gh, oracle, data, pos, cam, W, H)[0]
    parts = np.zeros_like(full)
    edges = [0, 192, 320, 512, W]
    for x0, x1 in zip(edges[:-1], edges[1:]):
        part, _, di, st, _, odi, V, _ = _render_pair(gh, oracle, data, pos, cam, W, H, band=(x0, x1))
        # a band context sorts and bins only the splats whose box touches the band (survivors); the whole
        # permutation is still available on demand and is the reference's
        assert np.array_equal(di, odi)
        assert 0 < st["visible"] < V
        assert not part[:, :x0].any() and not part[:, x1:].any()
        parts[:, x0:x1] = part[:, x0:x1]
    assert np.array_equal(parts, full)


# ---------------------------------------------------------------------------
# BASELINE.json full sizes
# ---------------------------------------------------------------------------
def _full_size_checks(gh, oracle, scenes, name, k, image=True, eps=0.0):
    cfg = gh.synth.CONFIGS[name]
    rows, data, pos = scenes(name)
    cam = _camera(gh, k, cfg)
    r = gh.HIPRenderer(cfg["width"], cfg["height"], early_out_eps=eps)
    r.set_raw_scene(data, pos)
    r.set_camera(cam)
    r.render_async(); r.sync()
    di = r.lastDepthIndex()
    keys, mm = r.read_keys()
    st = r.stats()
    # size-independent properties: a permutation, keys non-decreasing along it, ties in index order
    assert np.array_equal(np.sort(di), np.arange(cfg["n"], dtype=np.uint32))
    ks = keys[di].astype(np.int64)
    assert (np.diff(ks) >= 0).all()
    same = np.diff(ks) == 0
    assert (np.diff(di.astype(np.int64))[same] > 0).all()
    # and the oracle itself
    v, p, vp = cam.f32()
    odi, okeys, omm = oracle.sort(vp, pos)
    assert mm == omm and np.array_equal(keys, okeys) and np.array_equal(di, odi)
    rec, bbox = r.read_records()
    orec, obbox, oraw = oracle.project(data, v, p, cfg["fx"], cfg["fx"], cfg["width"], cfg["height"])
    _compare_records(rec, bbox, orec, obbox, oraw)
    V, D = oracle.tile_stats(obbox)
    assert st["visible"] == V and st["tile_entries"] == D
    if image:
        img = r.readPixelsFloat()
        oimg = oracle.render(odi, oraw, orec, obbox, cfg["width"], cfg["height"], 1)
        err = np.abs(img.astype(np.float64) - oimg.astype(np.float64)).max()
        assert err <= (TOL_EARLY if eps > 0 else TOL_EXACT), err
        a = img[..., 3]
        assert a.min() >= 0.0 and a.max() <= 1.0 + 1e-6
        if eps == 0:
            _check_against_ideal_mode(img, oracle.render(odi, oraw, orec, obbox, cfg["width"], cfg["height"], 0))
    r.dispose()


def _check_against_ideal_mode(img, ideal):
    """The kernel against the oracle's mode 0 (vPosition solved in f64 from the shader's f32 varyings, window
    coordinates: nothing of k_blend's bin-relative f32 expression in it).  The two can differ only where a pixel
    centre lies within f32 rounding of an ellipse edge (|vPosition|^2 = 4), where one side draws a fragment of weight
    <= e^-4 * opacity and the other does not.  Measured on the CPU (mode 1 vs mode 0): 37 such pixels on C2 pose 13,
    69 on C3 pose 21, of 2 073 600; largest difference 0.010."""
    d = np.abs(img.astype(np.float64) - ideal.astype(np.float64)).max(axis=2)
    flips = int((d > TOL_EXACT).sum())
    assert flips <= 2e-4 * d.size, flips
    assert d.max() < np.exp(-4.0) + 1e-3, d.max()


@pytest.mark.parametrize("name,k", [("C1", 40), ("C2", 13)])
def test_image_vs_ideal_mode(gh, oracle, scenes, name, k):
    cfg = gh.synth.CONFIGS[name]
    rows, data, pos = scenes(name)
    cam = _camera(gh, k, cfg)
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_raw_scene(data, pos)
    r.set_camera(cam)
    r.render_async(); r.sync()
    img = r.readPixelsFloat()
    r.dispose()
    v, p, vp = cam.f32()
    ideal = oracle.render_scene(data, pos, v, p, vp, cam.fx, cam.fy, cfg["width"], cfg["height"], mode=0)[0]
    _check_against_ideal_mode(img, ideal)


def test_offaxis_splats_match_independent_closed_form(gh, oracle):
    """The HIP path against tests/independent_math.py (float64 linear algebra from the meaning of the shader's
    expressions: (J'W)(4 Sigma)(J'W)^T + 0.3 I, weight = opacity * exp(-2 d^T C^-1 d)), on off-axis, rotated,
    anisotropic splats: neither oracle.c nor the kernels' operation order is involved in the expected values."""
    import independent_math as im
    from test_oracle_render import _offaxis_case, _usable
    W, H, fx, fy = 160, 120, 260.0, 240.0
    rng = np.random.default_rng(77)
    r = gh.HIPRenderer(W, H)
    checked = 0
    for _ in range(200):
        case = _offaxis_case(oracle, rng, W, H, fx, fy)
        if not _usable(case, W, H) or max(case["C"][0, 0], case["C"][1, 1]) < 6.0:
            continue
        r.set_raw_scene(case["data"], case["pos"])
        r.set_camera_arrays(case["view"], case["proj"], case["vp"], fx, fy)
        r.render_async(); r.sync()
        img = r.readPixelsFloat().astype(np.float64)
        rec, bbox = r.read_records()
        major, minor, lam = im.axes_from_cov(case["C"])
        flip = np.array([1.0, -1.0])
        u, w = 2 * (major * flip) / (major @ major), 2 * (minor * flip) / (minor @ minor)
        assert abs(rec[0, 0] - case["centre"][0]) < 2e-3 and abs(rec[0, 1] - (H - case["centre"][1])) < 2e-3
        assert np.linalg.norm(rec[0, 2:4] - u) <= 1.2e-3 * np.linalg.norm(u)
        assert np.linalg.norm(rec[0, 4:6] - w) <= 1.2e-3 * np.linalg.norm(w)
        rgba = [v / 255.0 for v in case["rgba"]]
        want, edge = im.splat_image(case["centre"], case["C"], rgba[3], rgba[:3], W, H)
        err = np.abs(img - want).max(axis=2)
        err[edge] = 0.0
        assert err.max() < 1e-4, err.max()
        checked += 1
        if checked == 8:
            break
    r.dispose()
    assert checked == 8


def test_overlapping_splats_match_independent_f64_under_composite(gh, oracle):
    """Multi-splat compositing against tests/independent_math.py: 3-5 overlapping off-axis anisotropic splats per image,
    composited in float64 with the reference's "under" blend (WebGLRenderer.ts:139-142,282-285, frag.glsl.ts:13-21) in
    ascending camera depth.  Neither oracle.c nor the kernels' operation order is in the expected image; the same cases
    pin oracle modes 0 and 1 (tests/test_oracle_render.py)."""
    from test_oracle_render import overlap_cases
    cases, (W, H, fx, fy) = overlap_cases(oracle)
    r = gh.HIPRenderer(W, H)
    for case in cases:
        r.set_raw_scene(case["data"], case["pos"])
        r.set_camera_arrays(case["view"], case["proj"], case["vp"], fx, fy)
        r.render_async(); r.sync()
        assert list(r.lastDepthIndex()) == list(np.argsort([f["z"] for f in case["forms"]], kind="stable"))
        err = np.abs(r.readPixelsFloat().astype(np.float64) - case["want"]).max(axis=2)
        err[case["edge"]] = 0.0
        assert err.max() < 1e-4, err.max()
    r.dispose()


def test_full_size_c3_1m_1080p(gh, oracle, scenes):
    _full_size_checks(gh, oracle, scenes, "C3", 21)


def test_full_size_c3_early_out(gh, oracle, scenes):
    _full_size_checks(gh, oracle, scenes, "C3", 84, eps=1e-4)


def test_full_size_c4_5m_4k(gh, oracle, scenes):
    _full_size_checks(gh, oracle, scenes, "C4", 50)


def test_torch_zero_copy_framebuffer(gh, scenes):
    # bench.py's N>1 path wraps the device framebuffer as a torch tensor for the RCCL all-gather
    import torch
    from gsplat_hip import bands
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_raw_scene(data, pos)
    r.set_camera(_camera(gh, 2, cfg))
    r.render_async(); r.sync()
    t = bands.framebuffer_tensor(torch, r, "cuda:0")
    assert t.shape == (cfg["height"], cfg["width"], 4) and t.data_ptr() == r.framebuffer_ptr()
    assert np.array_equal(t.cpu().numpy(), r.readPixelsFloat())
    r.dispose()


def test_api_errors_and_resize(gh, oracle, scenes):
    rows, data, pos = scenes(3000, 31)
    r = gh.HIPRenderer(160, 96)
    # call order: render before a camera is an error with a message, not a crash
    r.set_raw_scene(data, pos)
    with pytest.raises(gh.GsplatError, match="gsr_set_camera"):
        r.render_async()
    # positions must equal data words 0..2 (Scene.ts keeps them in sync)
    with pytest.raises(gh.GsplatError, match="positions differ"):
        r.set_raw_scene(data, pos + 1.0)
    r.set_raw_scene(data, pos)
    with pytest.raises(gh.GsplatError):
        r.set_band(10, 50)          # not on a bin boundary
    with pytest.raises(gh.GsplatError):
        r.setSize(0, 10)
    # resize re-allocates and the next frame matches the oracle at the new size
    for (W, H) in ((160, 96), (321, 203), (64, 64)):
        r.setSize(W, H)
        cam = gh.orbit_camera(4, width=W, height=H, fx=300.0)
        r.set_camera(cam)
        r.render_async(); r.sync()
        v, p, vp = cam.f32()
        oimg = oracle.render_scene(data, pos, v, p, vp, cam.fx, cam.fy, W, H, mode=1)[0]
        assert np.abs(r.readPixelsFloat().astype(np.float64) - oimg).max() <= TOL_EXACT
    # scene replacement with a different size
    rows2, data2, pos2 = scenes(777, 32)
    r.set_raw_scene(data2, pos2)
    r.render_async(); r.sync()
    assert r.lastDepthIndex().size == 777
    r.dispose()
    r.dispose()   # idempotent


def test_giant_and_degenerate_splats(gh, oracle):
    # a splat covering the whole screen (axis clamp 1024 px), a needle, a zero-opacity splat, and a tiny one
    from test_oracle_render import make_scene, front_camera
    W, H, fx = 640, 352, 900.0
    data, pos = make_scene(oracle, [
        dict(pos=(0.02, 0.01, 0), scale=(3.0, 2.5, 2.0), rgba=(200, 100, 50, 90), rot=(200, 160, 90, 130)),
        dict(pos=(0.4, -0.2, 0.5), scale=(1.5, 0.002, 0.002), rgba=(10, 250, 30, 255), rot=(190, 100, 160, 140)),
        dict(pos=(-0.5, 0.3, -0.5), scale=(0.3, 0.3, 0.3), rgba=(255, 255, 255, 0), rot=(255, 128, 128, 128)),
        dict(pos=(0.7, 0.4, 1.0), scale=(0.001, 0.001, 0.001), rgba=(255, 0, 255, 255), rot=(130, 250, 128, 20)),
    ])
    cam = front_camera(W, H, fx, -4.0)
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    r.set_camera(cam)
    r.render_async(); r.sync()
    img = r.readPixelsFloat()
    v, p, vp = cam.f32()
    oimg, odi, V, D = oracle.render_scene(data, pos, v, p, vp, cam.fx, cam.fy, W, H, mode=1)
    assert np.array_equal(r.lastDepthIndex(), odi)
    assert r.stats()["visible"] == V and V >= 3
    assert np.abs(img.astype(np.float64) - oimg).max() <= TOL_EXACT
    r.dispose()


def test_sh_colour_parity(gh, oracle, scenes):
    # SH colour, degree 0..3 by bandsIndices; colours bit-exact, image within tolerance
    n = 40000
    rows, data, pos = scenes(n, 41)
    rng = np.random.default_rng(8)
    b0, b1, b2 = 9999, 19999, 29999          # splats 0..9999: no SH; then degree 1, 2, 3
    shs = (rng.standard_normal((n - (b0 + 1), 48)) * 0.35).astype(np.float32)
    scene = gh.Scene()
    scene.bandsIndices = np.array([b0, b1, b2], dtype=np.int32)
    scene.setData(rows, shs)
    W, H = 640, 480
    cam = gh.orbit_camera(33, width=W, height=H)
    r = gh.HIPRenderer(W, H)
    r.render(scene, cam)
    img = r.readPixelsFloat()
    col = r.read_sh_colors()
    rec, bbox = r.read_records()
    r.dispose()
    v, p, vp = cam.f32()
    sh = oracle.scene_pack_sh(shs)
    orec, obbox, oraw = oracle.project(data, v, p, cam.fx, cam.fy, W, H, sh=sh, band=scene.bandsIndices)
    _compare_records(rec, bbox, orec, obbox, oraw)
    vis = (oraw[:, 11] == 1.0) & (np.arange(n) > b0)
    assert vis.sum() > 1000
    assert np.array_equal(col[vis, :3].view(np.uint32), oraw[vis, 7:10].view(np.uint32))
    assert (rec[vis, 7].view(np.uint32) == 0x01000000).all()
    di = oracle.sort(vp, pos)[0]
    oimg = oracle.render(di, oraw, orec, obbox, W, H, 1)
    assert np.abs(img.astype(np.float64) - oimg).max() <= TOL_EXACT
    # and the colours really are view dependent and differ from the rgba8 fallback
    plain = oracle.project(data, v, p, cam.fx, cam.fy, W, H)[2]
    assert np.abs(plain[vis, 7:10] - oraw[vis, 7:10]).max() > 0.05


@pytest.mark.parametrize("fade", [0.02, 0.11, 0.35, 1.0])
def test_depth_fade_parity(gh, oracle, scenes, fade):
    # FadeInPass uniforms (vertex.glsl.ts:214-229): records bit-exact, image within tolerance, at several fade values
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    cam = _camera(gh, 19, cfg)
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_raw_scene(data, pos)
    r.set_depth_fade(True, fade)
    r.set_camera(cam)
    r.render_async(); r.sync()
    rec, bbox = r.read_records()
    img = r.readPixelsFloat()
    v, p, vp = cam.f32()
    orec, obbox, oraw = oracle.project(data, v, p, cfg["fx"], cfg["fx"], cfg["width"], cfg["height"], fade=fade)
    _compare_records(rec, bbox, orec, obbox, oraw)
    oimg = oracle.render(oracle.sort(vp, pos)[0], oraw, orec, obbox, cfg["width"], cfg["height"], 1)
    assert np.abs(img.astype(np.float64) - oimg).max() <= TOL_EXACT
    # switching the pass off restores the steady state
    r.set_depth_fade(False, fade)
    r.render_async(); r.sync()
    plain = oracle.render_scene(data, pos, v, p, vp, cam.fx, cam.fy, cfg["width"], cfg["height"], mode=1)[0]
    assert np.abs(r.readPixelsFloat().astype(np.float64) - plain).max() <= TOL_EXACT
    if fade < 0.2:
        assert np.abs(oimg - plain).max() > 0.05
    r.dispose()


def test_stream_linked_rgba8_readout(gh, scenes):
    # bench.py's N>1 step: render_async -> convert_rgba8_async -> torch's stream waits on the library's stream -> copy
    import torch
    from gsplat_hip import bands
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_raw_scene(data, pos)
    link = bands.StreamLink(torch, r, "cuda:0")
    fb8 = bands.framebuffer8_tensor(torch, r, "cuda:0")
    outs = []
    for k in (3, 50):
        r.set_camera(_camera(gh, k, cfg))
        link.renderer_waits_for_torch()
        r.render_async()
        r.convert_rgba8_async()
        link.torch_waits_for_renderer()
        outs.append(fb8.clone())            # on torch's stream, ordered after the conversion
        ev = torch.cuda.Event(); ev.record()
        link.renderer_waits_for_event(ev)   # the next frame may overwrite fb8 only after the clone
    torch.cuda.synchronize()
    r.sync()
    assert np.array_equal(outs[1].cpu().numpy(), r.readPixels())
    r.set_camera(_camera(gh, 3, cfg))
    r.render_async(); r.sync()
    assert np.array_equal(outs[0].cpu().numpy(), r.readPixels())
    tot = r.bin_totals()
    assert tot.shape == (-(-cfg["height"] // 32), -(-cfg["width"] // 32)) and tot.sum() == r.stats()["bin_entries"]
    r.dispose()


def test_native_slab_exchange_single_device(gh, scenes):
    # the N>1 RGBA8 exchange of bench.py with the collective replaced by a local stand-in: three "ranks" (contexts with
    # cost-balanced, unequal bands) pack their bands into slabs, a fake all-gather stacks them, one kernel de-slabs;
    # the result must be the whole-frame RGBA8 image bit for bit
    import torch
    from gsplat_hip import bands
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    W, H = cfg["width"], cfg["height"]
    cam = _camera(gh, 21, cfg)
    whole = gh.HIPRenderer(W, H)
    whole.set_raw_scene(data, pos); whole.set_camera(cam); whole.render_async(); whole.sync()
    cost = whole.bin_totals().sum(axis=0) + 8.0 * H
    world = 3
    edges = bands.balanced_edges(W, world, cost)
    assert edges[0][0] == 0 and edges[-1][1] == W and len({b - a for a, b in edges}) > 1
    stacked = {}

    class FakeDist:      # stands in for torch.distributed: "gathers" what the other ranks packed earlier
        def __init__(self, rank): self.rank = rank
        def all_gather_into_tensor(self, flat, slab):
            stacked[self.rank] = slab.clone()
            if len(stacked) == world:
                flat.copy_(torch.cat([stacked[q] for q in range(world)], dim=0))

    rs = []
    for q in range(world):
        r = gh.HIPRenderer(W, H, band=edges[q])
        r.set_raw_scene(data, pos)
        rs.append((r, bands.StreamLink(torch, r, "cuda:0"),
                   bands.FrameExchange(FakeDist(q), torch, W, H, q, world, torch.device("cuda:0"), edges=edges, dtype=torch.uint8)))
    for k in (21, 64):       # the second frame goes through the slab-reuse event path
        c = _camera(gh, k, cfg)
        whole.set_camera(c); whole.render_async(); whole.sync()
        stacked.clear()
        outs = []
        for r, link, x in rs:
            r.set_camera(c)
            r.render_async()
            outs.append(x.exchange_native(r, link))
        torch.cuda.synchronize()
        assert np.array_equal(outs[-1].cpu().numpy(), whole.readPixels())     # the last "rank" saw all three slabs
    # errors: slab narrower than the band, too many ranks
    with pytest.raises(gh.GsplatError):
        rs[0][0].pack_band_rgba8_async(outs[0].data_ptr(), 1)
    with pytest.raises(gh.GsplatError):
        rs[0][0].unpack_slabs_rgba8_async(outs[0].data_ptr(), outs[0].data_ptr(), 64, [(0, 32)] * 17, 0)
    for r, _, _ in rs:
        r.dispose()
    whole.dispose()


def test_graph_replay_equals_individual_launches(gh, scenes, monkeypatch):
    # frames without stage events are replayed from a captured HIP graph; the same frames issued as individual launches
    # (GSR_NO_GRAPH=1 at context creation) must give identical pixels and permutations, across camera changes, a resize
    # (other launch arguments -> recapture) and sampled timing (every 3rd frame takes the individual-launch path)
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    monkeypatch.setenv("GSR_NO_GRAPH", "1")
    plain = gh.HIPRenderer(cfg["width"], cfg["height"])
    monkeypatch.delenv("GSR_NO_GRAPH")
    graph = gh.HIPRenderer(cfg["width"], cfg["height"], timing=True)
    graph.set_timing_interval(3)
    for r in (plain, graph):
        r.set_raw_scene(data, pos)
    for step, (k, size) in enumerate([(0, None), (11, None), (12, None), (40, (512, 384)), (41, None), (90, (cfg["width"], cfg["height"])), (91, None)]):
        for r in (plain, graph):
            if size:
                r.setSize(*size)
            r.set_camera(gh.orbit_camera(k, width=r.width, height=r.height, fx=cfg["fx"]))
            r.render_async(); r.sync()
        assert np.array_equal(plain.readPixelsFloat(), graph.readPixelsFloat()), step
        assert np.array_equal(plain.lastDepthIndex(), graph.lastDepthIndex()), step
    st = graph.stats()
    assert 2 <= st["frames"] <= 4          # 7 renders + the sort-only calls of lastDepthIndex do not all carry events
    with pytest.raises(gh.GsplatError):
        graph.set_timing_interval(0)
    # the calls that reallocate what a captured graph points at or change what its launches are sized by: after each, two
    # frames on both contexts (at most one of two consecutive frames carries events, so one of them is a graph launch)
    n = pos.size // 3
    m = n // 2
    sh = [np.full(8 * n, 0x34003400, dtype=np.uint32) for _ in range(3)]     # (every half-float coefficient 0.25)
    rows2 = gh.synth.synth_rows(4096, 17)
    changes = [lambda r: r.set_list_capacity(1 << 21),
               lambda r: r.set_band(128, 384), lambda r: r.set_band(0, 0),
               lambda r: r.set_sh(sh, [-1, n // 4, n // 2]), lambda r: r.set_sh(sh, [n - 1, n - 1, n - 1]),
               lambda r: r.set_scene_rows(rows2), lambda r: r.scene_limit_box([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0]),
               lambda r: r.set_raw_scene(data[:8 * m], pos[:3 * m])]
    for step, change in enumerate(changes):
        for r in (plain, graph):
            change(r)
        for k in (20 + 2 * step, 21 + 2 * step):
            for r in (plain, graph):
                r.set_camera(gh.orbit_camera(k, width=r.width, height=r.height, fx=cfg["fx"]))
                r.render_async(); r.sync()
            assert np.array_equal(plain.readPixelsFloat(), graph.readPixelsFloat()), (step, k)
            assert np.array_equal(plain.lastDepthIndex(), graph.lastDepthIndex()), (step, k)
    assert plain.stats()["overflow_frames"] == 0 and graph.stats()["overflow_frames"] == 0
    plain.dispose(); graph.dispose()


def test_frames_in_flight_equal_sequential_frames(gh, scenes):
    # bench.py's default mode: three throughput-tuned contexts with a frame in flight each, issued round-robin without
    # waiting; every frame must equal the one a single default context renders on its own (segment lengths differ
    # between the two tunings, so the image is compared within the exact-mode tolerance, the permutation bit for bit)
    cfg = gh.synth.CONFIGS["C2"]
    rows, data, pos = scenes("C2")
    W, H = cfg["width"], cfg["height"]
    rs = [gh.HIPRenderer(W, H, throughput=True, timing=True) for _ in range(3)]
    for r in rs:
        r.set_raw_scene(data, pos)
        r.set_timing_interval(2)
    ref = gh.HIPRenderer(W, H)
    ref.set_raw_scene(data, pos)
    got = {}
    poses = list(range(0, 120, 9))
    for n, k in enumerate(poses):
        r = rs[n % 3]
        if n >= 3:                      # this context's previous frame: read it back before it is overwritten
            r.sync()
            got[poses[n - 3]] = (r.readPixelsFloat(), r.lastDepthIndex())
        r.set_camera(_camera(gh, k, cfg))
        r.render_async()
    for n in range(len(poses) - 3, len(poses)):
        r = rs[n % 3]
        r.sync()
        got[poses[n]] = (r.readPixelsFloat(), r.lastDepthIndex())
    for k in poses:
        ref.set_camera(_camera(gh, k, cfg))
        ref.render_async(); ref.sync()
        assert np.array_equal(got[k][1], ref.lastDepthIndex()), k
        err = np.abs(got[k][0].astype(np.float64) - ref.readPixelsFloat().astype(np.float64)).max()
        assert err <= TOL_EXACT, (k, err)
    for r in rs + [ref]:
        r.dispose()


def test_cpp_caller_matches_python_host(gh, scenes, tmp_path):
    # the stand-alone C++ caller of the C ABI (tools/bench_cabi.cpp: device-side Scene.setData, its own Camera.update in
    # double precision) fed the same .splat bytes must produce the same permutation and the same RGBA8 image as the
    # Python host (host-side Scene.setData + numpy Camera), bit for bit
    import json, os, subprocess
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    f = tmp_path / "c1.splat"
    f.write_bytes(np.asarray(rows, dtype=np.uint8).tobytes())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsplat.js_amd", "lib", "bench_cabi")
    # (--in-flight 1: contexts of the same kind as the Python host's below; throughput contexts composite with the other kernel,
    #  same pixels to f32 association)
    out = subprocess.run([exe, "--config", "C1", "--rows", str(f), "--frames", "30", "--warmup", "5", "--in-flight", "1", "--dump", str(tmp_path / "cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n"] == cfg["n"] and line["frames_per_sec"] > 0
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_raw_scene(data, pos)
    r.set_camera(_camera(gh, 0, cfg))
    r.render_async(); r.sync()
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp.depth_index.bin"), dtype=np.uint32), r.lastDepthIndex())
    got = np.fromfile(str(tmp_path / "cpp.rgba8.bin"), dtype=np.uint8).reshape(cfg["height"], cfg["width"], 4)
    assert np.array_equal(got, r.readPixels())
    r.dispose()


def test_randomised_configurations(gh, oracle, scenes):
    # seeded sweep over the knobs that change code paths: splat count (incl. tiny), ragged framebuffer sizes, splat
    # size range, orbit radius / elevation (camera inside and outside the cloud), bands, early termination, the
    # throughput tuning, stage events; permutation bit-exact, image within the mode's tolerance of the oracle
    rng = np.random.default_rng(20260404)
    for case in range(24):
        n = int(rng.choice([1, 2, 63, 65, 300, 2049, 5000, 20000]))
        W, H = int(rng.integers(17, 900)), int(rng.integers(17, 700))
        s_hi = float(rng.choice([0.02, 0.06, 0.3]))
        rows, data, pos = scenes(n, 1000 + case, sigma=float(rng.choice([0.5, 1.5])), s_lo=0.004, s_hi=s_hi)
        cam = gh.orbit_camera(int(rng.integers(0, 120)), width=W, height=H, fx=float(rng.choice([300.0, 1132.0])),
                              beta=float(rng.uniform(-1.2, 1.2)), radius=float(rng.choice([0.5, 3.0, 8.0, 20.0])))
        eps = float(rng.choice([0.0, 0.0, 1e-3]))
        band = None
        if rng.random() < 0.4 and W > 64:
            b0 = int(rng.integers(0, (W - 1) // 32)) * 32
            band = (b0, min(W, b0 + 32 * int(rng.integers(1, 6))))
        r = gh.HIPRenderer(W, H, early_out_eps=eps, band=band, throughput=bool(rng.random() < 0.5), timing=bool(rng.random() < 0.5))
        r.set_raw_scene(data, pos)
        r.set_camera(cam)
        r.render_async(); r.sync()
        img, di = r.readPixelsFloat(), r.lastDepthIndex()
        r.dispose()
        v, p, vp = cam.f32()
        oimg, odi, V, D = oracle.render_scene(data, pos, v, p, vp, cam.fx, cam.fy, W, H, mode=1)
        assert np.array_equal(di, odi), case
        if band:
            assert not img[:, :band[0]].any() and not img[:, band[1]:].any(), case
            img, oimg = img[:, band[0]:band[1]], oimg[:, band[0]:band[1]]
        err = np.abs(img.astype(np.float64) - oimg.astype(np.float64)).max() if img.size else 0.0
        assert err <= (TOL_EARLY * 2 if eps > 0 else TOL_EXACT), (case, n, W, H, band, eps, err)


def test_on_device_scene_build_and_transforms(gh, oracle):
    # Scene.setData / translate / rotate / scale / limitBox as kernels, bit-exact with the
    # f64 restatement of the JavaScript (which tests/test_js_host.py pins against the JS implementation itself)
    rows = gh.synth.synth_rows(50000, 61)
    r2 = rows.reshape(-1, 32).copy()
    r2[0, 28:32] = [255, 128, 128, 128]                                  # identity rotation
    r2[1, 12:24] = np.array([200.0, 1e-9, 3.0], dtype=np.float32).view(np.uint8)   # halves overflow / underflow
    rows = r2.reshape(-1)
    st = oracle.SceneState(rows)
    W, H = 640, 480
    r = gh.HIPRenderer(W, H)
    r.set_scene_rows(rows)

    def same():
        data, pos, rot, scl = r.read_scene()
        assert np.array_equal(pos, st.positions) and np.array_equal(data, st.data)
        assert np.array_equal(rot, st.rotations) and np.array_equal(scl, st.scales)

    same()
    q = gh.camera.quaternion_from_euler(0.3, -0.2, 0.1)
    for op, arg in (("translate", [0.25, -0.5, 1.0]), ("rotate", q), ("scale", [1.5, 0.75, 1.25]), ("translate", [1e-3, 0, -2]),
                    ("rotate", gh.camera.quaternion_from_euler(-1.0, 2.0, 0.5))):
        getattr(st, op)(arg)
        getattr(r, "scene_" + op)(arg)
        same()
    st.limit_box([-3, 3, -2.5, 4, -4, 1.5])
    assert r.scene_limit_box([-3, 3, -2.5, 4, -4, 1.5]) == st.n and 0 < st.n < 50000
    same()
    with pytest.raises(gh.GsplatError, match="xMin"):
        r.scene_limit_box([1, 1, 0, 1, 0, 1])
    # and the transformed device scene renders like the oracle renders the transformed host scene
    cam = gh.orbit_camera(12, width=W, height=H)
    r.set_camera(cam)
    r.render_async(); r.sync()
    v, p, vp = cam.f32()
    oimg, odi, V, D = oracle.render_scene(st.data, st.positions, v, p, vp, cam.fx, cam.fy, W, H, mode=1)
    assert np.array_equal(r.lastDepthIndex(), odi)
    assert np.abs(r.readPixelsFloat().astype(np.float64) - oimg).max() <= TOL_EXACT
    # a scene uploaded as data/positions has no rotations/scales to transform
    r.set_raw_scene(st.data, st.positions)
    with pytest.raises(gh.GsplatError, match="gsr_set_scene_rows"):
        r.scene_translate([1, 0, 0])
    r.dispose()


def test_list_overflow_is_sticky_counted_and_repaired(gh, oracle, scenes):
    """VERDICT r1 / ADVICE: a frame whose bin lists do not fit publishes no compositor work; with frames enqueued
    asynchronously the host used to see only the LAST frame's overflow word.  Now: a sticky device counter mirrored
    into a host-mapped word, regrowth at the next enqueue or sync, the last frame rendered again, and one
    GSR_ERR_OVERFLOW from gsr_sync that says how many earlier frames were lost."""
    rows, data, pos = scenes(60000, 21)
    W, H = 640, 480
    cams = [gh.orbit_camera(k, width=W, height=H) for k in (3, 9, 15)]
    ref = gh.HIPRenderer(W, H)
    ref.set_raw_scene(data, pos)
    ref.set_camera(cams[2])
    ref.render_async(); ref.sync()
    want = ref.readPixelsFloat()
    assert ref.stats()["overflow_frames"] == 0 and ref.stats()["bin_entries"] > 4096
    ref.dispose()

    # blocking render: overflow -> regrow -> same frame again, invisible to the caller apart from the counter
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    r.set_list_capacity(2048)
    r.set_camera(cams[2])
    r._check(r._L.gsr_render(r._ctx))
    st = r.stats()
    assert st["overflow_frames"] == 1 and st["dropped_frames"] == 0 and not r.overflow_pending()
    assert np.array_equal(r.readPixelsFloat(), want)

    # three asynchronous frames into a list that is far too small
    r.set_list_capacity(2048)
    for cam in cams:
        r.set_camera(cam)
        r.render_async()
    with pytest.raises(gh.GsplatError, match="not composited"):
        r.sync()
    st = r.stats()
    assert st["overflow_frames"] >= 2 and 1 <= st["dropped_frames"] <= 2, st
    assert not r.overflow_pending()
    r.sync()                                   # reported once; the context stays usable
    assert np.array_equal(r.readPixelsFloat(), want), "the last frame was rendered again after the regrowth"
    r.set_camera(cams[0])
    r.render_async(); r.sync()
    assert r.stats()["overflow_frames"] == st["overflow_frames"]
    r.dispose()


def test_sort_host_sees_positions_edited_in_place(gh, oracle, scenes):
    """gsplat_sort_host cached the upload by buffer address + count; a JS Scene.translate edits the same
    Float32Array in place, so the second call sorted the old positions.  It now copies the positions on every call."""
    rows, data, pos = scenes(20000, 31)
    L = gh.load_library()
    vp = gh.orbit_camera(5, width=640, height=480).f32()[2]
    buf = np.array(pos, dtype=np.float32, copy=True)
    out = np.empty(buf.size // 3, dtype=np.uint32)
    keys = np.empty_like(out)
    L.gsplat_sort_host(vp.ctypes.data, out.size, buf.ctypes.data, keys.ctypes.data, out.ctypes.data, None, None)
    odi, okeys, _ = oracle.sort(vp, buf)
    assert np.array_equal(out, odi) and np.array_equal(keys, okeys)
    buf.reshape(-1, 3)[:, 2] *= -1.0            # same address, same count, other scene
    buf.reshape(-1, 3)[:, 0] += 0.25
    L.gsplat_sort_host(vp.ctypes.data, out.size, buf.ctypes.data, None, out.ctypes.data, None, None)
    odi2, _, _ = oracle.sort(vp, buf)
    assert not np.array_equal(odi, odi2)
    assert np.array_equal(out, odi2)
    # other size through the same process-wide context, then back
    m = 777
    out2 = np.empty(m, dtype=np.uint32)
    L.gsplat_sort_host(vp.ctypes.data, m, buf.ctypes.data, None, out2.ctypes.data, None, None)
    assert np.array_equal(out2, oracle.sort(vp, buf[:3 * m])[0])
    # an empty scene between two sorts (a viewer that resets and reloads its scene): it runs no kernel, so it must not move on
    # the sort-only frames' slot sets either -- the sort behind it would fold the depth range of the sort before it into its own
    L.gsplat_sort_host(vp.ctypes.data, out.size, buf.ctypes.data, None, out.ctypes.data, None, None)
    L.gsplat_sort_host(vp.ctypes.data, 0, buf.ctypes.data, None, out2.ctypes.data, None, None)
    near = np.ascontiguousarray(buf[:3 * m] * np.float32(0.25))      # another depth range than the whole scene's
    keys2 = np.empty(m, dtype=np.uint32)
    L.gsplat_sort_host(vp.ctypes.data, m, near.ctypes.data, keys2.ctypes.data, out2.ctypes.data, None, None)
    odi3, okeys3, _ = oracle.sort(vp, near)
    assert np.array_equal(keys2, okeys3) and np.array_equal(out2, odi3)


def test_limit_box_clears_sh_state(gh):
    """limitBox renumbers the splats; SH rows addressed by the old numbering must not survive it."""
    n = 4096
    rows = gh.synth.synth_rows(n, 17)
    r = gh.HIPRenderer(320, 240)
    r.set_scene_rows(rows)
    band = np.array([-1, n // 4, n // 2], dtype=np.int32)
    tex = [np.zeros(8 * n, dtype=np.uint32) for _ in range(3)]
    r.set_sh(tex, band)
    kept = r.scene_limit_box([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0])
    assert 0 < kept < n and r.scene_count() == kept
    r.set_camera(gh.orbit_camera(2, width=320, height=240))
    r.render_async(); r.sync()
    with pytest.raises(gh.GsplatError):
        r.read_sh_colors()                      # no SH state any more: the scene renders with its rgba8 colours
    r.dispose()


def test_rccl_allgather_inside_the_library_single_rank(gh, scenes):
    """The product's multi-GPU exchange (gsr_comm_init / gsr_allgather_frame_async): pack -> ncclAllGather -> de-slab on
    the library's own streams.  A one-GPU box can form a communicator of ONE rank (RCCL refuses two ranks on one
    device); that still runs every call of the path, the stream/event ordering with frames enqueued back to back, and
    the id hand-over.  The gathered RGBA8 frame must equal the plain renderer's RGBA8 image byte for byte."""
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    W, H = cfg["width"], cfg["height"]
    ref = gh.HIPRenderer(W, H)
    ref.set_raw_scene(data, pos)
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    with pytest.raises(gh.GsplatError):
        r.allgather_frame_async()                           # not in a group yet
    with pytest.raises(gh.GsplatError):
        r.join_group(gh.new_group_id(), 0, 1, [(0, W - 32)])   # edges must cover the image
    r.join_group(gh.new_group_id(), 0, 1, [(0, W)])
    cams = [_camera(gh, k, cfg) for k in (5, 41, 77, 113)]
    for cam in cams:                                        # back to back: the next frame must not overtake the exchange
        r.set_camera(cam)
        r.render_async()
        r.allgather_frame_async()
    got = r.read_frame()
    ref.set_camera(cams[-1])
    ref.render_async(); ref.sync()
    assert np.array_equal(got, ref.readPixels())
    r.sync()
    r.leave_group()
    r.set_camera(cams[0])
    r.render_async(); r.sync()                              # usable as a plain renderer again
    ref.set_camera(cams[0])
    ref.render_async(); ref.sync()
    assert np.array_equal(r.readPixels(), ref.readPixels())
    r.dispose(); ref.dispose()


def test_gathered_frame_is_refused_after_a_list_overflow(gh, scenes):
    """A frame whose bin lists do not fit publishes no compositor work: the framebuffer keeps the preceding image.  When
    such a frame was enqueued and gathered without a host sync in between, the gathered frame holds a stale band:
    gsr_read_frame_rgba8 waits for the render stream, sees the overflow, regrows the lists and refuses the frame
    (GSR_ERR_OVERFLOW) instead of returning it; gathering again gives the right frame."""
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    W, H = cfg["width"], cfg["height"]
    ref = gh.HIPRenderer(W, H)
    ref.set_raw_scene(data, pos)
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    r.join_group(gh.new_group_id(), 0, 1, [(0, W)])
    r.set_camera(_camera(gh, 5, cfg))
    r.render_async(); r.allgather_frame_async()
    first = r.read_frame()
    r.set_list_capacity(1024)                  # far too small for the next frame
    cam = _camera(gh, 60, cfg)
    r.set_camera(cam)
    r.render_async()
    r.allgather_frame_async()
    with pytest.raises(gh.GsplatError, match="not composited"):
        r.read_frame()
    r.allgather_frame_async()                  # the lists have been regrown and the frame rendered again: gather it
    got = r.read_frame()
    ref.set_camera(cam)
    ref.render_async(); ref.sync()
    assert np.array_equal(got, ref.readPixels()) and not np.array_equal(got, first)
    assert r.stats()["overflow_frames"] >= 1
    r.dispose(); ref.dispose()


@pytest.mark.parametrize("order", ["lsd", "bucket", "auto"])
def test_sort_orders_give_the_same_permutation(gh, oracle, scenes, monkeypatch, order):
    """Two radix orders produce the reference's permutation: LSD (low 8 bits, then high 9: six launches) and bucket order
    (high 9 bits first, then one workgroup per bucket sorts by the low 8: four launches, used for small scenes).
    'auto' = what ships: LSD for the first frame of a scene, bucket order once a frame has reported that no bucket is
    too large, LSD again when one is.  Scenes: uniform, one with depth outliers that push nearly every splat into a
    few buckets (the fallback case), one with a single multi-chunk bucket (> 8192 keys), tiny ones."""
    if order != "auto":
        monkeypatch.setenv("GSR_SORT_ORDER", order)
    rng = np.random.default_rng(5)
    cases = []
    rows, data, pos = scenes(200000, 41)
    cases.append(("gaussian", np.array(pos, copy=True)))
    p2 = np.array(pos, copy=True).reshape(-1, 3)
    p2[:7] *= 4000.0                               # outliers stretch the key range: the rest collapses into a few buckets
    cases.append(("outliers", p2.reshape(-1)))
    p3 = rng.normal(size=(60000, 3)).astype(np.float32) * 1e-3
    p3[::7] += rng.normal(size=(p3[::7].shape)).astype(np.float32)
    cases.append(("dense slab", p3.reshape(-1)))
    cases.append(("tiny", np.array(pos[:3 * 77], copy=True)))
    for name, pp in cases:
        n = pp.size // 3
        d = np.zeros((n, 8), dtype=np.uint32)
        d[:, 0:3] = pp.reshape(-1, 3).view(np.uint32)
        r = gh.HIPRenderer(640, 480)
        r.set_raw_scene(d, pp)
        for k in (0, 17, 63, 91):
            cam = _camera(gh, k, SMALL)
            r.sort(cam)
            odi, okeys, omm = oracle.sort(cam.f32()[2], pp)
            keys, mm = r.read_keys()
            assert mm == omm and np.array_equal(keys, okeys), (name, k)
            assert np.array_equal(r.lastDepthIndex(), odi), (name, k, order)
        r.dispose()


@pytest.mark.gpu
def test_fold_inside_the_compositor_matches_the_separate_kernel(gh, monkeypatch):
    """Bins cut into several segments are folded by the workgroup that delivers the bin's last segment (inside k_blend;
    the partials cross XCDs with agent-scope stores and loads).  The fold order is fixed, so the image must equal the
    separate k_combine launch (GSR_FUSE_COMBINE=0) bit for bit -- on every pose, with several frames queued back to
    back (a stale partial from the previous frame would show), and for a second context on the same device."""
    cfg = gh.synth.CONFIGS["C3"]
    W, H = cfg["width"], cfg["height"]
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows("C3"))
    monkeypatch.setenv("GSR_LONG_ITEMS", "0")   # 512-entry segments: up to ~50 partials per bin (long items with a front
    monkeypatch.setenv("GSR_FUSE_COMBINE", "0")  # window exist only with the fold inside k_blend: no k_combine counterpart)
    ref = gh.HIPRenderer(W, H)
    monkeypatch.delenv("GSR_FUSE_COMBINE")
    a, b = gh.HIPRenderer(W, H), gh.HIPRenderer(W, H)
    poses = list(range(0, 120, 5))
    ref.render(scene, gh.orbit_camera(0, 120, W, H, cfg["fx"]))
    a.render(scene, gh.orbit_camera(0, 120, W, H, cfg["fx"]))
    b.render(scene, gh.orbit_camera(0, 120, W, H, cfg["fx"]))
    multi = 0
    for k in poses:
        cam = gh.orbit_camera(k, 120, W, H, cfg["fx"])
        ref.render(scene, cam)
        want = ref.readPixelsFloat()
        for r in (a, b):      # three frames queued without a sync in between, the last one is read
            r.set_camera(gh.orbit_camera((k + 60) % 120, 120, W, H, cfg["fx"]))
            r.render_async()
            r.set_camera(gh.orbit_camera((k + 30) % 120, 120, W, H, cfg["fx"]))
            r.render_async()
            r.set_camera(cam)
            r.render_async()
        for r in (a, b):
            r.sync()
            assert np.array_equal(r.readPixelsFloat(), want), k
        multi += 1
    assert multi == len(poses)
    for r in (ref, a, b):
        r.dispose()


@pytest.mark.gpu
def test_read_pixels_into_a_caller_buffer(gh):
    """readPixels(out) / readPixelsFloat(out) fill and return the caller's array (no allocation per frame) and refuse
    arrays of the wrong type or size."""
    cfg = gh.synth.CONFIGS["C1"]
    W, H = cfg["width"], cfg["height"]
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows("C1"))
    r = gh.HIPRenderer(W, H)
    r.render(scene, gh.orbit_camera(5, 120, W, H, cfg["fx"]))
    a8 = np.zeros((H, W, 4), dtype=np.uint8)
    af = np.zeros(H * W * 4, dtype=np.float32)
    assert r.readPixels(a8) is a8 and np.array_equal(a8, r.readPixels())
    assert r.readPixelsFloat(af) is af and np.array_equal(af.reshape(H, W, 4), r.readPixelsFloat())
    with pytest.raises(ValueError):
        r.readPixels(np.zeros((H, W, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        r.readPixelsFloat(a8)
    r.dispose()


@pytest.mark.gpu
def test_band_contexts_with_multi_segment_bins_equal_the_full_frame(gh, monkeypatch):
    """The multi-GPU partition at the size where bins are cut into segments (C3: up to ~50 segments per bin with short
    work items), so that band contexts run the fold of the partials too: four band contexts, each compositing its columns
    of the same frame, reproduce the full-frame context's image bit for bit, on several poses, when the work-item length
    is pinned.  Left to itself every context picks the length from the optical depth of its OWN pixels (dense centre
    bands: long items, sparse edge bands: short segments), and the bands then agree with the full frame to f32
    association order (2e-6; RGBA8 within one step)."""
    cfg = gh.synth.CONFIGS["C3"]
    W, H = cfg["width"], cfg["height"]
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows("C3"))
    edges = [0, 448, 960, 1472, W]
    for pinned in ("0", None):
        if pinned is None:
            monkeypatch.delenv("GSR_LONG_ITEMS", raising=False)
        else:
            monkeypatch.setenv("GSR_LONG_ITEMS", pinned)
        full = gh.HIPRenderer(W, H)
        parts = [gh.HIPRenderer(W, H, band=(x0, x1)) for x0, x1 in zip(edges[:-1], edges[1:])]
        for k in (7, 52, 99):
            cam = gh.orbit_camera(k, 120, W, H, cfg["fx"])
            full.render(scene, cam)
            want = full.readPixelsFloat()
            got = np.zeros_like(want)
            for r, x0, x1 in zip(parts, edges[:-1], edges[1:]):
                r.render(scene, cam)
                img = r.readPixelsFloat()
                assert not img[:, :x0].any() and not img[:, x1:].any()
                got[:, x0:x1] = img[:, x0:x1]
            if pinned is None:
                assert np.abs(got - want).max() <= 2e-6, k
            else:
                assert np.array_equal(got, want), k
        for r in [full] + parts:
            r.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["bucket", "lsd", "lsd gather"])
def test_band_lists_are_the_full_frames_lists_of_the_band(gh, monkeypatch, order):
    """A band context sorts and bins only its survivors: k_project_key packs them per workgroup, k_kept_scan / k_band_gather
    leave them dense in index order, and every kernel behind runs on that many keys (workgroups and table rows past them do
    nothing).  Their sorted order must be the restriction of the frame's order: the band's bin lists equal, entry for entry,
    the lists the full-frame context builds for the same bin columns -- in both sort orders, with the rectangles carried
    through the sort or gathered, for bands that keep most splats, few, and none at all."""
    monkeypatch.setenv("GSR_SORT_ORDER", order.split()[0])
    if "gather" in order:
        monkeypatch.setenv("GSR_RECT_CARRY", "0")
    W, H, n = 1280, 736, 150_001            # (a last projection workgroup of 241 splats)
    scene = gh.Scene()
    scene.setData(gh.synth.synth_rows(n, 77, 2.0, 0.004, 0.05))
    full = gh.HIPRenderer(W, H)
    bands = [(0, 32), (32, 608), (608, 672), (672, 1248), (1248, W)]
    parts = [gh.HIPRenderer(W, H, band=b) for b in bands]
    nbx, nby = (W + 31) // 32, (H + 31) // 32
    for k in (3, 41):
        cam = gh.orbit_camera(k, 120, W, H, 900.0)
        full.render(scene, cam)
        fs, fl = full.bin_lists()
        want_img = full.readPixelsFloat()
        survivors = []
        for r, (x0, x1) in zip(parts, bands):
            r.render(scene, cam)
            st, lst = r.bin_lists()
            bx0, bx1 = x0 // 32, (x1 + 31) // 32
            w = bx1 - bx0
            assert st.size == w * nby + 1
            for by in range(nby):
                for bx in range(w):
                    a = fl[fs[by * nbx + bx0 + bx]:fs[by * nbx + bx0 + bx + 1]]
                    b = lst[st[by * w + bx]:st[by * w + bx + 1]]
                    assert np.array_equal(a, b), (order, k, x0, bx, by)
            assert np.array_equal(r.readPixelsFloat()[:, x0:x1], want_img[:, x0:x1])
            survivors.append(r.stats()["visible"])
            assert np.array_equal(r.lastDepthIndex(), full.lastDepthIndex())   # (the whole permutation, on demand)
        assert 0 < min(survivors) < max(survivors) < full.stats()["visible"]
    # a band no splat touches: a small blob in the middle of the screen, the band at the left edge
    off = gh.Scene()
    off.setData(gh.synth.synth_rows(20_000, 78, 0.1, 0.004, 0.02))
    cam = gh.orbit_camera(0, 120, W, H, 900.0)
    parts[0].render(off, cam)
    assert parts[0].stats()["visible"] == 0 and not parts[0].readPixelsFloat().any()
    full.render(off, cam)
    assert full.stats()["visible"] > 0
    for r in [full] + parts:
        r.dispose()


def _lists_of(gh, size, scene, cams, env, monkeypatch, band=None):
    for k in ("GSR_BIN_TWO_LEVEL", "GSR_RECT_CARRY", "GSR_SORT_ORDER"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = gh.HIPRenderer(size[0], size[1], band=band) if band else gh.HIPRenderer(size[0], size[1])
    for k in env:
        monkeypatch.delenv(k)
    out = []
    for cam in cams:
        r.render(scene, cam)
        starts, lst = r.bin_lists()
        out.append((starts, lst, r.lastDepthIndex(), r.readPixelsFloat(), r.stats()["overflow_frames"]))
    r.dispose()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["640x480", "1000x712 lsd", "4k", "4k band", "4k band lsd", "4k lsd gather"])
def test_two_level_binning_builds_the_one_level_lists(gh, monkeypatch, case):
    """Large bin grids are binned in two levels (k_bin.hip: cells of 4 x 4 bins with the lane-set pass, then every cell
    list's chunks into the cell's 16 bins with ballots), and in the LSD sort order the packed rectangles travel with the
    keys instead of being gathered through depthIndex.  Both must leave exactly the lists of the one-level pass --
    every bin's start and every entry, i.e. the depth order inside every bin (what the front-to-back blend of
    WebGLRenderer.ts:139-142,282-285 needs) -- and with them the same image bit for bit.  Forced on at small sizes
    (partial cells at the right and bottom edges: 640x480 = 20 x 15 bins, 1000x712 = 32 x 23), natural at 4K, in a band
    context (columns relative to the band), with the rectangles gathered and carried (640x480: carried through the bucket
    order's two kernels as well, GSR_RECT_CARRY=2)."""
    W, H = {"640x480": (640, 480), "1000x712 lsd": (1000, 712)}.get(case, (3840, 2160))
    n = 60000 if W < 3840 else 400000
    scene = gh.Scene()
    scene.setData(gh.synth.synth_rows(n, 77, sigma=1.2, s_lo=0.004, s_hi=0.09))
    cams = [gh.orbit_camera(k, 120, W, H, 1132.0 * W / 1920.0) for k in (4, 41, 97)]
    band = (1184, 2848) if "band" in case else None   # (a band context sorts its survivors only: the first pass drops the rest)
    lsd = {"GSR_SORT_ORDER": "lsd"} if "lsd" in case else {}
    want = _lists_of(gh, (W, H), scene, cams, dict(lsd, GSR_BIN_TWO_LEVEL="0", GSR_RECT_CARRY="0"), monkeypatch, band)
    got = _lists_of(gh, (W, H), scene, cams, dict(lsd, GSR_BIN_TWO_LEVEL="1", GSR_RECT_CARRY="0" if "gather" in case else "2" if case == "640x480" else "1"), monkeypatch, band)
    for (ws, wl, wd, wi, _), (gs, gl, gd, gi, _) in zip(want, got):
        assert np.array_equal(wd, gd)
        assert np.array_equal(ws, gs), "bin starts"
        assert ws[-1] > 4 * ws.size and np.array_equal(wl, gl), "list entries"
        assert np.array_equal(wi, gi)
        # a bin's entries are a subsequence of depthIndex: ranks ascending inside every bin
        rank = np.empty(wd.size, dtype=np.int64)
        rank[wd] = np.arange(wd.size)
        rk = rank[gl]
        first_of_bin = np.zeros(rk.size + 1, dtype=bool)
        first_of_bin[gs] = True
        assert np.all((np.diff(rk) > 0) | first_of_bin[1:rk.size])


@pytest.mark.gpu
def test_two_level_binning_overflow_is_repaired_in_one_regrowth(gh, monkeypatch):
    """A frame whose lists do not fit must report how many entries it needs in ONE pass (the host regrows once and
    renders the frame again; a second overflow is an error): the two-level pass knows the need before it has built a
    single list -- the count pass over the cells also sums the rectangles' areas in bins -- and, when the cell lists
    themselves would not fit, gives the frame no chunks at all."""
    W, H = 3840, 2160
    scene = gh.Scene()
    scene.setData(gh.synth.synth_rows(300000, 78, sigma=1.2, s_lo=0.004, s_hi=0.09))
    cam = gh.orbit_camera(11, 120, W, H, 2264.0)
    ref = gh.HIPRenderer(W, H)
    ref.render(scene, cam)
    want = ref.readPixelsFloat()
    entries = ref.stats()["bin_entries"]
    ws, wl = ref.bin_lists()
    ref.dispose()
    for cap in (entries - 1, entries // 2, 4096):     # just too small; smaller than the lists; smaller than the cell lists
        r = gh.HIPRenderer(W, H)
        r.render(scene, gh.orbit_camera(60, 120, W, H, 2264.0))
        r.set_list_capacity(int(cap))
        r.render(scene, cam)                            # overflow -> regrow -> the same frame again
        st = r.stats()
        assert st["overflow_frames"] == 1 and st["dropped_frames"] == 0, (cap, st)
        gs, gl = r.bin_lists()
        assert np.array_equal(gs, ws) and np.array_equal(gl, wl)
        assert np.array_equal(r.readPixelsFloat(), want)
        r.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("throughput", [False, True], ids=["k_blend2", "k_blend"])
@pytest.mark.parametrize("long_items", ["0", "1"])
def test_saturated_quadrants_are_skipped_without_changing_a_bit(gh, monkeypatch, long_items, throughput):
    """The compositor drops a quadrant once every one of its pixels has a transmittance below 2^-27 of its smallest colour
    channel: no later splat can change a bit of such a pixel (w <= T, c <= 1: w*c is under half an ulp of the channel; alpha
    is 1 - T = 1.0f), and what the segment's own T would still become only multiplies later segments in the fold, whose
    terms are then under half an ulp as well.  So the image must equal, BIT FOR BIT, the one composited without the skip
    (GSR_SATURATE=0) -- with short segments (512 entries: the fold of partials is in play) and with long work items
    (whole bins, where most of the skipping happens: 53 % of C3's list entries).  Both kernels, each asserted to be the one
    that ran: a default context at 1080p runs k_blend2 (two waves per tile), which tests at the chunk boundaries; a
    throughput context runs k_blend (one wave per tile), which tests after every 64-entry step."""
    cfg = gh.synth.CONFIGS["C3"]
    W, H = cfg["width"], cfg["height"]
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows("C3"))
    monkeypatch.setenv("GSR_LONG_ITEMS", long_items)
    monkeypatch.setenv("GSR_SATURATE", "0")
    full = gh.HIPRenderer(W, H, throughput=throughput)
    monkeypatch.delenv("GSR_SATURATE")
    skip = gh.HIPRenderer(W, H, throughput=throughput)
    for k in (2, 31, 64, 97):
        cam = gh.orbit_camera(k, 120, W, H, cfg["fx"])
        full.render(scene, cam)
        skip.render(scene, cam)
        for r in (full, skip):
            assert r.work_items()["waves_per_tile"] == (1 if throughput else 2)
        assert np.array_equal(skip.readPixelsFloat(), full.readPixelsFloat()), k
        assert np.array_equal(skip.readPixels(), full.readPixels()), k
    full.dispose(); skip.dispose()


@pytest.mark.gpu
def test_long_and_short_work_items_agree(gh, monkeypatch):
    """Which bins are handed to the compositor as ONE work item is chosen per bin by k_bin_finalize, from figures of the frame
    alone: the frame-wide prior (optical depth over the splats' boxes, tiles per splat) and the bin's own optical depth (its
    entries x the frame's optical mass per entry).  A dense blob (C3) comes out as whole bins throughout, bit for bit the
    pinned long cut; a frame of small splats (C2) as segments throughout, bit for bit the pinned short cut; a tight cluster
    inside a sparse halo -- not dense as a frame -- as a MIX: the cluster's bins whole, the halo's cut.  The cuts differ in f32
    association order only (2e-6; RGBA8 one step), gsr_read_work_items tells what was picked, and the choice is a function of
    the frame alone (the same frame again, another frame in between: the same bits)."""
    W, H, fx = 1920, 1080, 1132.0
    for name, rows in (("C3", gh.synth.config_rows("C3")), ("C2", gh.synth.config_rows("C2")), ("cluster+halo", gh.synth.cluster_in_halo())):
        scene = gh.Scene()
        scene.setData(rows)
        cam = gh.orbit_camera(17, 120, W, H, fx)
        imgs, items = {}, {}
        for mode in ("0", "1", "auto", "auto again"):
            if mode.startswith("auto"):
                monkeypatch.delenv("GSR_LONG_ITEMS", raising=False)
            else:
                monkeypatch.setenv("GSR_LONG_ITEMS", mode)
            r = gh.HIPRenderer(W, H)
            if mode == "auto again":
                r.render(scene, gh.orbit_camera(63, 120, W, H, fx))      # another frame in between changes nothing
            r.render(scene, cam)
            imgs[mode] = (r.readPixelsFloat(), r.readPixels())
            wi = r.work_items()
            items[mode] = wi["items"]
            nbins = wi["bins"]
            assert wi["waves_per_tile"] == 2 and not wi["speculative"]
            r.dispose()
        assert np.abs(imgs["0"][0] - imgs["1"][0]).max() <= 2e-6
        assert np.abs(imgs["0"][1].astype(np.int32) - imgs["1"][1].astype(np.int32)).max() <= 1
        assert np.array_equal(imgs["auto"][0], imgs["auto again"][0]) and items["auto"] == items["auto again"], name
        assert items["1"] == nbins < items["0"], (name, items)
        if name == "C3":
            assert items["auto"] == nbins and np.array_equal(imgs["auto"][0], imgs["1"][0]), (name, items)
        elif name == "C2":
            assert items["auto"] == items["0"] and np.array_equal(imgs["auto"][0], imgs["0"][0]), (name, items)
        else:                # the mix: more items than bins (the halo's long bins are cut), fewer than the all-segments cut
            assert nbins < items["auto"] < items["0"], (name, items)
            assert np.abs(imgs["auto"][0] - imgs["1"][0]).max() <= 2e-6 and np.abs(imgs["auto"][0] - imgs["0"][0]).max() <= 2e-6


@pytest.mark.gpu
def test_two_waves_per_tile_agree_with_one(gh, oracle, scenes, monkeypatch):
    """k_blend2 gives every 16x16 tile two waves: the first walks the first half of each 256-entry chunk's hits under the
    running transmittance, the second the other half from (colour 0, transmittance 1), folded at the chunk boundary
    (associativity of "under": frag.glsl.ts:13-21 with the blend state of WebGLRenderer.ts:139-142).  Same depth order,
    another f32 association than k_blend: images within 2e-6 of each other on C3 (whole-bin items, saturation skip on and
    off bit-identical within the kernel) and C2 (short segments), and within 2e-4 of the oracle on C1 and C2 with either
    kernel.  Contexts that render one frame at a time use it up to 4096 bins; throughput contexts and 4K keep k_blend."""
    for name, poses in (("C3", (11, 73)), ("C2", (40,))):
        cfg = gh.synth.CONFIGS[name]
        W, H = cfg["width"], cfg["height"]
        scene = gh.Scene()
        scene.setData(gh.synth.config_rows(name))
        monkeypatch.setenv("GSR_BLEND_SUB", "1")
        one = gh.HIPRenderer(W, H)
        monkeypatch.setenv("GSR_BLEND_SUB", "2")
        two = gh.HIPRenderer(W, H)
        monkeypatch.setenv("GSR_SATURATE", "0")
        monkeypatch.setenv("GSR_LONG_ITEMS", "1")
        two_all = gh.HIPRenderer(W, H)
        monkeypatch.delenv("GSR_SATURATE")
        two_pinned = gh.HIPRenderer(W, H)
        monkeypatch.delenv("GSR_LONG_ITEMS")
        monkeypatch.delenv("GSR_BLEND_SUB")
        auto = gh.HIPRenderer(W, H)
        thr = gh.HIPRenderer(W, H, throughput=True)
        for k in poses:
            cam = gh.orbit_camera(k, 120, W, H, cfg["fx"])
            imgs = {}
            for key, r in (("one", one), ("two", two), ("two_all", two_all), ("two_pinned", two_pinned), ("auto", auto), ("thr", thr)):
                r.render(scene, cam)
                imgs[key] = r.readPixelsFloat()
            assert one.work_items()["waves_per_tile"] == 1 and two.work_items()["waves_per_tile"] == 2
            assert auto.work_items()["waves_per_tile"] == 2 and thr.work_items()["waves_per_tile"] == 1
            assert np.abs(imgs["one"] - imgs["two"]).max() <= 2e-6, (name, k)
            assert np.abs(imgs["one"] - imgs["thr"]).max() <= 2e-6, (name, k)      # k_blend as well, with the throughput cut of the lists
            assert np.array_equal(imgs["two"], imgs["auto"]), (name, k)
            assert np.array_equal(imgs["two_all"], imgs["two_pinned"]), (name, k)   # the saturation skip changes no bit here either
        for r in (one, two, two_all, two_pinned, auto, thr):
            r.dispose()
    for sub in ("1", "2"):
        monkeypatch.setenv("GSR_BLEND_SUB", sub)
        for name, pose in (("C1", 40), ("C2", 13)):
            c = gh.synth.CONFIGS[name]
            rows, data, pos = scenes(name)
            cam = _camera(gh, pose, c)
            img, img8, di, st, oimg, odi, V, D = _render_pair(gh, oracle, data, pos, cam, c["width"], c["height"])
            assert np.array_equal(di, odi)
            assert np.abs(img.astype(np.float64) - oimg.astype(np.float64)).max() <= TOL_EXACT, (sub, name)
    monkeypatch.delenv("GSR_BLEND_SUB")
    w4 = gh.HIPRenderer(3840, 2160)      # 8160 bins: one wave per tile
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows("C1"))
    w4.render(scene, gh.orbit_camera(3, 120, 3840, 2160, 2264.0))
    assert w4.work_items()["waves_per_tile"] == 1
    w4.dispose()


@pytest.mark.gpu
def test_c5_workload_as_eight_bands_on_one_gpu(gh, oracle, scenes, monkeypatch):
    """BASELINE C5's workload on the one GPU a test box has: the C4 scene (5 M splats, 3840x2160, fx 2264) rendered as EIGHT
    cost-balanced band contexts -- what the eight ranks of a C5 run each do (bench.py split_config: edges from two
    calibration poses) -- and as one full-frame context.  At this size a band context takes the paths only 5 M splats select:
    the LSD radix order with the bin rectangles carried through it, survivor sort, and (bands of up to 4096 bins) the
    one-level binning beside the full frame's two-level binning.  Checked on two poses:
      * the union of the bands is the full frame: bit for bit when every context cuts its lists alike (work-item length
        pinned), within f32 association order (2e-6) when each band decides from the optical depth of its own pixels;
      * a band's per-bin list lengths are the full frame's for its columns, its counters (visible splats, 16x16 tile
        overlaps, list entries) are what the full frame's records give for the band, and the bands' entries sum to the frame's;
      * gsr_read_depth_index on a band context (survivor sort in the frame, full sort on demand) is the oracle's permutation."""
    from gsplat_hip import bands
    cfg = gh.synth.CONFIGS["C4"]
    W, H, N = cfg["width"], cfg["height"], cfg["n"]
    rows, data, pos = scenes("C4")
    world = 8
    cal = gh.HIPRenderer(W, H)
    cal.set_raw_scene(data, pos)
    cost = np.zeros(-(-W // 32))
    for k in (0, 60):
        cal.set_camera(_camera(gh, k, cfg))
        cal.render_async(); cal.sync()
        cost += cal.bin_totals().sum(axis=0) + 0.25 * 32 * H
    cal.dispose()
    edges = bands.balanced_edges(W, world, cost)
    assert len(edges) == world and edges[0][0] == 0 and edges[-1][1] == W and all(b > a for a, b in edges)
    assert max(b - a for a, b in edges) > min(b - a for a, b in edges)      # centre-heavy scene: unequal bands
    for pinned in ("1", None):
        # pinned: every context cuts its lists alike AND composites with the same kernel (left alone, the full 4K frame --
        # 8160 bins -- takes one wave per tile and a band of up to 4096 bins two: the same pixels to f32 association)
        if pinned is None:
            monkeypatch.delenv("GSR_LONG_ITEMS", raising=False)
            monkeypatch.delenv("GSR_BLEND_SUB", raising=False)
        else:
            monkeypatch.setenv("GSR_LONG_ITEMS", pinned)
            monkeypatch.setenv("GSR_BLEND_SUB", "1")
        full = gh.HIPRenderer(W, H)
        parts = [gh.HIPRenderer(W, H, band=e) for e in edges]
        for r in [full] + parts:
            r.set_raw_scene(data, pos)
        for k in (50, 110):
            cam = _camera(gh, k, cfg)
            full.set_camera(cam)
            full.render_async(); full.sync()
            want = full.readPixelsFloat()
            totals = full.bin_totals()
            fst = full.stats()
            assert fst["overflow_frames"] == 0 and fst["bin_entries"] == int(totals.sum())
            _, bbox = full.read_records()
            bx0, by0, bx1, by1 = (bbox[:, j].astype(np.int64) for j in range(4))
            drawn = bx0 <= bx1
            got = np.zeros_like(want)
            entries = 0
            for r, (x0, x1) in zip(parts, edges):
                r.set_camera(cam)
                r.render_async(); r.sync()
                img = r.readPixelsFloat()
                assert not img[:, :x0].any() and not img[:, x1:].any()
                got[:, x0:x1] = img[:, x0:x1]
                lo, hi = x0 // 32, -(-x1 // 32)
                assert np.array_equal(r.bin_totals(), totals[:, lo:hi]), (k, x0)
                st = r.stats()
                touch = drawn & (bx1 >= 32 * lo) & (bx0 < 32 * hi)
                tx0, tx1 = np.maximum(bx0 // 16, 2 * lo), np.minimum(bx1 // 16, 2 * hi - 1)
                tiles = ((tx1 - tx0 + 1) * (by1 // 16 - by0 // 16 + 1))[touch].sum()
                assert st["overflow_frames"] == 0
                assert (st["visible"], st["tile_entries"], st["bin_entries"]) == (int(touch.sum()), int(tiles), int(totals[:, lo:hi].sum())), (k, x0)
                entries += st["bin_entries"]
            assert entries == fst["bin_entries"]
            if pinned is None:
                assert np.abs(got - want).max() <= 2e-6, k
            else:
                assert np.array_equal(got, want), k
            del want, got, img
        if pinned is None:
            v, p, vp = cam.f32()
            odi = oracle.sort(vp, pos)[0]
            for r in (parts[0], parts[4]):
                assert np.array_equal(r.lastDepthIndex(), odi)
            assert np.array_equal(full.lastDepthIndex(), odi)
        for r in [full] + parts:
            r.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("sub", ["1", "2"])
def test_bins_with_more_than_64_segments(gh, monkeypatch, sub):
    """A bin's arrival mask has one bit per segment, so a bin is cut into at most 64 segments and the last one takes
    whatever is left (k_bin_finalize's cut, k_blend's `seg + 1 == nseg ? bin_end`).  C3 seen at a third of its resolution
    (the whole scene on 240 bins) has bins of several ten thousand entries: with 256-entry segments well over 64 segments'
    worth.  The fold inside the compositor (both kernels) must equal the separate k_combine launch bit for bit there, and
    the whole-bin cut to f32 association."""
    cfg = dict(gh.synth.CONFIGS["C3"])
    W, H = 640, 360
    cfg["fx"] /= 3
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows("C3"))
    monkeypatch.setenv("GSR_LONG_ITEMS", "0")
    monkeypatch.setenv("GSR_SEG_LEN", "256")
    monkeypatch.setenv("GSR_SEG_TARGET", "100000")    # (so that the frame's segment length is not raised above the 256 asked for)
    monkeypatch.setenv("GSR_BLEND_SUB", sub)
    cam0 = gh.orbit_camera(5, 120, W, H, cfg["fx"])
    fused = gh.HIPRenderer(W, H)
    fused.render(scene, cam0)
    monkeypatch.setenv("GSR_FUSE_COMBINE", "0")
    separate = gh.HIPRenderer(W, H)
    separate.render(scene, cam0)
    monkeypatch.delenv("GSR_FUSE_COMBINE")
    monkeypatch.delenv("GSR_SEG_LEN")
    monkeypatch.delenv("GSR_SEG_TARGET")
    monkeypatch.setenv("GSR_LONG_ITEMS", "1")
    whole = gh.HIPRenderer(W, H)
    whole.render(scene, cam0)
    for k in (17, 71):
        cam = gh.orbit_camera(k, 120, W, H, cfg["fx"])
        for r in (fused, separate, whole):
            r.render(scene, cam)
        wi = fused.work_items()
        assert wi["seg_len"] == 256 and int(fused.bin_totals().max()) > 64 * 256 and wi["items"] > 4 * wi["bins"]
        a, b, c = fused.readPixelsFloat(), separate.readPixelsFloat(), whole.readPixelsFloat()
        assert np.array_equal(a, b), k
        assert np.abs(a - c).max() <= 2e-6, k
        assert fused.stats()["overflow_frames"] == 0
    for r in (fused, separate, whole):
        r.dispose()


# Every environment knob the library still reads (DESIGN.md section 6 lists them), at a non-default value: each selects code that
# otherwise only an A/B run would execute.  C1 rendered twice (the first frame of a scene sorts in LSD order) under the knob,
# depthIndex bit-exact and image within 2e-4 of the oracle; knobs of the large-grid binning at 3840x2160 (8160 bins).
_KNOBS = [("GSR_NO_GRAPH", "1", None), ("GSR_SORT_ORDER", "lsd", None), ("GSR_SORT_ORDER", "bucket", None), ("GSR_FUSE_COMBINE", "0", None),
          ("GSR_SATURATE", "0", None), ("GSR_LONG_ITEMS", "0", None), ("GSR_LONG_ITEMS", "1", None), ("GSR_LONG_TAU", "20", None),
          ("GSR_BLEND_SUB", "1", None), ("GSR_BLEND_SUB", "2", None), ("GSR_ITEMS_BY_SIZE", "0", None), ("GSR_SEG_TARGET", "200", None),
          ("GSR_SEG_LEN", "256", None), ("GSR_BLEND_GRID", "64", None), ("GSR_SORT_KPB", "4096", None),
          ("GSR_RECT_CARRY", "0", None), ("GSR_RECT_CARRY", "2", None), ("GSR_TIMING_EVERY", "3", None),
          ("GSR_BIN_TWO_LEVEL", "1", None), ("GSR_BIN_TWO_LEVEL", "0", "4k"), ("GSR_CELL_GRID", "64", "4k"), ("GSR_BIN_BIG", "0", "4k one level"),
          ("GSR_BIN_BIG", "1", "4k one level"), ("GSR_BIN_ROUNDS", "2", "4k one level")]
_KNOB_ORACLE = {}


@pytest.mark.gpu
@pytest.mark.parametrize("knob", _KNOBS, ids=["%s=%s%s" % (k, v, " " + w if w else "") for k, v, w in _KNOBS])
def test_every_knob_at_a_non_default_value_matches_the_oracle(gh, oracle, scenes, monkeypatch, knob):
    env, val, where = knob
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    W, H = (3840, 2160) if where else (cfg["width"], cfg["height"])
    if where and "one level" in where and env != "GSR_BIN_TWO_LEVEL":
        monkeypatch.setenv("GSR_BIN_TWO_LEVEL", "0")
    monkeypatch.setenv(env, val)
    r = gh.HIPRenderer(W, H, timing=env == "GSR_TIMING_EVERY")
    r.set_raw_scene(data, pos)
    for k in (11, 58):
        cam = gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"])
        r.set_camera(cam)
        r.render_async(); r.sync()
        if (W, k) not in _KNOB_ORACLE:
            v, p, vp = cam.f32()
            _KNOB_ORACLE[(W, k)] = oracle.render_scene(data, pos, v, p, vp, cam.fx, cam.fy, W, H, mode=1)[:2]
        oimg, odi = _KNOB_ORACLE[(W, k)]
        assert np.array_equal(r.lastDepthIndex(), odi), (env, val, k)
        err = np.abs(r.readPixelsFloat().astype(np.float64) - oimg.astype(np.float64)).max()
        assert err <= TOL_EXACT, (env, val, k, err)
    assert r.stats()["overflow_frames"] == 0
    r.dispose()


@pytest.mark.gpu
def test_assembly_walk_equals_the_cpp_loop(gh, monkeypatch):
    """The compositor's innermost loop -- the walk over a tile's entries of a 64-entry step -- ships as a block of assembly
    (k_blend.hip, GSR_ASM_WALK_STEP: s_ff1 / s_bitset0 / s_bitcmp1 for the walk, v_cmpx for the coverage); the same loop in C++
    is the `cppwalk` twin of the library (-DGSR_CPP_WALK, built by __graft_entry__.build()).  Same arithmetic instruction for
    instruction, so every image must be equal bit for bit: both compositor kernels, both cuts of the lists, the separate
    fold, early termination, throughput contexts (the benchmarked form, C3 and C4) -- and the depthIndex, which the compositor
    does not touch."""
    import os
    lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsplat.js_amd", "lib_exp", "cppwalk", "libgsplat_hip.so")
    assert os.path.exists(lib), "the C++-walk build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    cases = [("C1", {}, {}), ("C2", {}, {}), ("C3", {}, {}), ("C3", {"GSR_BLEND_SUB": "1"}, {}), ("C3", {"GSR_LONG_ITEMS": "0"}, {}),
             ("C2", {"GSR_FUSE_COMBINE": "0"}, {}), ("C2", {}, {"early_out_eps": 1e-4}), ("C2", {}, {"throughput": True}), ("C3", {}, {"throughput": True}),
             ("C4", {}, {"throughput": True})]
    for name, env, kw in cases:
        cfg = gh.synth.CONFIGS[name]
        W, H = cfg["width"], cfg["height"]
        scene = gh.Scene()
        scene.setData(gh.synth.config_rows(name))
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        a = gh.HIPRenderer(W, H, **kw)
        b = gh.HIPRenderer(W, H, lib_path=lib, **kw)
        for k in ((9,) if name == "C4" else (9, 77)):
            cam = gh.orbit_camera(k, 120, W, H, cfg["fx"])
            a.render(scene, cam); b.render(scene, cam)
            assert np.array_equal(a.readPixelsFloat(), b.readPixelsFloat()), (name, env, kw, k)
            assert np.array_equal(a.lastDepthIndex(), b.lastDepthIndex())
        a.dispose(); b.dispose()
        for k in env:
            monkeypatch.delenv(k)

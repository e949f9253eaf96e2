"""Front-end workgroup width (GSR_FRONT_WAVES; SortPlan::waves and BinPlan::form in FrameArgs): throughput contexts run the four heavy front-end
kernels of the one-level 1080p chain -- the bucket order's partition pass and k_local_sort, k_bin_count, k_bin_scatter --
as 8-wave workgroups, default contexts as 16-wave ones.  A workgroup owns the same keys / ranks and the same table row at
either width, so everything a frame leaves behind must be the same bits: depthIndex, every bin's start and entries, the
cut into work items, the image."""
import ctypes

import numpy as np
import pytest

WIDTHS = ("16", "8")
GSR_ERR_ARG = -1   # include/gsplat_hip.h


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _renderer(gh, monkeypatch, W, H, waves, throughput, order=None):
    """a context pinned to `waves` (None: what its kind chooses) and, optionally, to one sort order"""
    for k, v in (("GSR_FRONT_WAVES", waves), ("GSR_SORT_ORDER", order)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    r = gh.HIPRenderer(W, H, throughput=throughput)
    monkeypatch.delenv("GSR_FRONT_WAVES", raising=False)
    monkeypatch.delenv("GSR_SORT_ORDER", raising=False)
    return r


def _frame(r):
    starts, lst = r.bin_lists()
    return dict(di=r.lastDepthIndex(), starts=starts, list=lst, items=r.work_items(), img=r.readPixelsFloat())


def _assert_same_frame(a, b, what):
    assert np.array_equal(a["di"], b["di"]), (what, "depthIndex")
    assert np.array_equal(a["starts"], b["starts"]), (what, "bin starts")
    assert a["starts"][-1] > a["starts"].size and np.array_equal(a["list"], b["list"]), (what, "list entries")
    assert a["items"] == b["items"], (what, a["items"], b["items"])
    assert np.array_equal(a["img"], b["img"]), (what, float(np.abs(a["img"] - b["img"]).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["bucket", "lsd"])
@pytest.mark.parametrize("kind", ["throughput", "default"])
@pytest.mark.parametrize("name,poses", [("C2", (13, 40)), ("C3", (21, 84))])
def test_both_widths_build_the_same_frame(gh, monkeypatch, name, poses, kind, order):
    cfg = gh.synth.CONFIGS[name]
    W, H = cfg["width"], cfg["height"]
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows(name))
    rs = [_renderer(gh, monkeypatch, W, H, w, kind == "throughput", order) for w in WIDTHS]
    for k in poses:
        cam = gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"])
        frames = []
        for r in rs:
            r.render(scene, cam)
            frames.append(_frame(r))
        assert frames[0]["items"]["bins"] <= 4096          # the one-level chain the narrow kernels belong to
        _assert_same_frame(frames[0], frames[1], (name, k, kind, order))
    for r in rs:
        r.dispose()


@pytest.mark.gpu
def test_a_large_bucket_falls_back_to_the_lsd_order_at_either_width(gh, scenes, monkeypatch):
    """Depth outliers stretch the key range, nearly every splat lands in a few high-digit buckets (> 48 K keys), and the
    frames after the first report fall back to the LSD order -- whose kernels have one width.  The frames in front of the
    fall-back and behind it are the same at both widths, and the sort is the oracle's."""
    from oracle import oracle as O
    cfg = gh.synth.CONFIGS["C2"]
    W, H = cfg["width"], cfg["height"]
    rows, data, pos = scenes("C2")
    p2 = np.array(pos, copy=True).reshape(-1, 3)
    p2[:7] *= 4000.0
    d2 = np.array(data, copy=True).reshape(-1, 8)
    d2[:, 0:3] = p2.view(np.uint32)                # (Scene.data words 0..2 are the position)
    p2 = p2.reshape(-1)
    rs = [_renderer(gh, monkeypatch, W, H, w, True) for w in WIDTHS]
    for r in rs:
        r.set_raw_scene(d2, p2)
    for k in (5, 6, 7, 58):
        cam = gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"])
        frames = []
        for r in rs:
            r.set_camera(cam)
            r.render_async(); r.sync()
            frames.append(_frame(r))
        _assert_same_frame(frames[0], frames[1], ("outliers", k))
        odi, _, _ = O.sort(cam.f32()[2], p2)
        assert np.array_equal(frames[1]["di"], odi), k
    for r in rs:
        r.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("C2", 13), ("C3", 21)])
def test_narrow_throughput_context_meets_the_oracle(gh, oracle, scenes, monkeypatch, name, k):
    """What ships: a throughput context with no knob set runs the narrow kernels.  depthIndex bit for bit, image within 2e-4."""
    cfg = gh.synth.CONFIGS[name]
    W, H = cfg["width"], cfg["height"]
    rows, data, pos = scenes(name)
    cam = gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"])
    r = _renderer(gh, monkeypatch, W, H, None, True)
    r.set_raw_scene(data, pos)
    r.set_camera(cam)
    for _ in range(2):      # (the second frame sorts in the bucket order: the first one of a scene has no bucket report yet)
        r.render_async(); r.sync()
    img, di = r.readPixelsFloat(), r.lastDepthIndex()
    r.dispose()
    v, p, vp = cam.f32()
    odi, _, _ = oracle.sort(vp, pos)
    assert np.array_equal(di, odi)
    oimg, odi2, V, D = oracle.render_scene(data, pos, v, p, vp, cam.fx, cam.fy, W, H, mode=1)
    assert np.array_equal(di, odi2)
    err = float(np.abs(img.astype(np.float64) - oimg.astype(np.float64)).max())
    assert err <= 2e-4, err


@pytest.mark.gpu
def test_graphs_of_contexts_at_different_widths_stay_apart(gh, monkeypatch):
    """The width is part of FrameArgs, a context's graph key: two contexts that differ in nothing else capture a graph
    each and replay their own.  Frames alternate between them (untimed contexts replay the captured graph from the second
    frame of a pose on) and stay equal, frame by frame, to a third context that launches kernel by kernel."""
    cfg = gh.synth.CONFIGS["C2"]
    W, H = cfg["width"], cfg["height"]
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows("C2"))
    rs = [_renderer(gh, monkeypatch, W, H, w, True) for w in WIDTHS]
    monkeypatch.setenv("GSR_NO_GRAPH", "1")
    plain = _renderer(gh, monkeypatch, W, H, "8", True)
    monkeypatch.delenv("GSR_NO_GRAPH")
    for r in rs + [plain]:
        r.render(scene, gh.orbit_camera(0, width=W, height=H, fx=cfg["fx"]))
    for k in (3, 4, 5, 6, 7, 8):
        cam = gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"])
        for r in rs + [plain]:
            r.set_camera(cam)
            r.render_async()
        for r in rs + [plain]:
            r.sync()
        want = _frame(plain)
        for r, w in zip(rs, WIDTHS):
            _assert_same_frame(want, _frame(r), ("graph", k, w))
    for r in rs + [plain]:
        r.dispose()


@pytest.mark.parametrize("value", ["4", "12", "0", "-8", "8x", "wide", ""])
def test_the_knob_refuses_widths_no_kernel_is_built_for(monkeypatch, value):
    """GSR_FRONT_WAVES is read with the other knobs when a context is created, before any device is looked for: a value
    other than 8 or 16 fails gsr_create with GSR_ERR_ARG and says why (with or without a GPU)."""
    import gsplat_hip as gh
    lib = gh.load_library()
    monkeypatch.setenv("GSR_FRONT_WAVES", value)
    ctx = ctypes.c_void_p()
    rc = lib.gsr_create(ctypes.byref(ctx), None)
    assert rc == GSR_ERR_ARG and not ctx.value
    lib.gsr_last_error.restype = ctypes.c_char_p
    msg = lib.gsr_last_error(None).decode()
    assert "GSR_FRONT_WAVES" in msg and "8 or 16" in msg


@pytest.mark.parametrize("value", ["8", "16"])
def test_the_knob_accepts_both_widths(monkeypatch, value):
    """... and 8 or 16 get past the knobs: a context where there is a GPU, the no-device error where there is none."""
    import gsplat_hip as gh
    lib = gh.load_library()
    monkeypatch.setenv("GSR_FRONT_WAVES", value)
    ctx = ctypes.c_void_p()
    rc = lib.gsr_create(ctypes.byref(ctx), None)
    lib.gsr_last_error.restype = ctypes.c_char_p
    if rc == 0:
        assert ctx.value
        lib.gsr_destroy(ctx)
    else:
        assert rc != GSR_ERR_ARG and "GSR_FRONT_WAVES" not in lib.gsr_last_error(None).decode()

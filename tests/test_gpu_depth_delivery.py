"""Frame delivery with depth (gsr_delivery_open_depth; k_depth_planes<.., 2> and k_deliver_depth).  The bar everywhere: the plane
a depth ring delivers with frame k is, bit for bit, the definition in plain numpy (tests/depth_delivery_reference.py) applied to
what gsr_read_depth returns for the same pose; the colour beside it is the colour of the same ring without depth; and
everything the ring promises holds with the plane aboard."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_delivery_reference as DD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
GSR_ERR_ARG = -1
# (scene, size, pose): C1 and C2 at their own size, an odd size, and a size below one 32-pixel bin
CASES = [("C1", None, 3), ("C2", None, 13), ("C1", (1001, 701), 40), ("C1", (23, 9), 7)]


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _camera(gh, k, cfg, W=None, H=None):
    W, H = W or cfg["width"], H or cfg["height"]
    return gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"] * W / cfg["width"])


def _renderer(gh, scenes, name, size=None, **kw):
    cfg = gh.synth.CONFIGS[name]
    W, H = size or (cfg["width"], cfg["height"])
    r = gh.HIPRenderer(W, H, **kw)
    r.set_raw_scene(*scenes(name)[1:])
    return r, cfg, W, H


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _colour(px):
    return px.ravel().copy() if isinstance(px, np.ndarray) else np.concatenate([p.ravel() for p in px])


def _deliver_one(r):
    """render_async + deliver + acquire + release of the current camera's frame: (serial, colour bytes, depth plane), copies"""
    r.render_async()
    k = r.deliver()
    s, px, depth = r.acquire(k)
    assert s == k and not depth.flags.writeable
    out = (s, _colour(px), depth.copy())
    r.release(s)
    return out


def _want(hit, fmt, step, near):
    w = DD.subsample(hit, step)
    return DD.quantise_u16(w, near) if fmt == "u16" else w


# ---- 1.-3. the plane ----
@pytest.mark.parametrize("name,size,pose", CASES)
def test_delivered_plane_is_the_definition_of_read_depth(gh, scenes, name, size, pose):
    r, cfg, W, H = _renderer(gh, scenes, name, size)
    r.set_camera(_camera(gh, pose, cfg, W, H))
    r.render_async()
    hit = r.read_depth()[1]
    if min(W, H) >= 32:
        assert np.isfinite(hit).any() and np.isinf(hit).any()
    for fmt, step, near in (("f32", 1, 0.1), ("f32", 2, 0.1), ("u16", 1, 0.1), ("u16", 2, 0.1), ("u16", 2, 2.5), ("u16", 1, 6.0)):
        r.open_delivery_depth(2, depth=fmt, depth_step=step, depth_near=near)
        Wd, Hd = DD.plane_size(W, H, step)
        lay = r.depth_layout()
        colour = r.delivery_layout()["bytes"]
        assert lay == {"format": fmt, "step": step, "width": Wd, "height": Hd, "stride": Wd * (4 if fmt == "f32" else 2),
                       "offset": (colour + 15) // 16 * 16, "bytes": Wd * Hd * (4 if fmt == "f32" else 2), "near": float(np.float32(near)) if fmt == "u16" else 0.0}
        s, px, depth = _deliver_one(r)
        want = _want(hit, fmt, step, near)
        assert depth.dtype == want.dtype and depth.shape == (Hd, Wd)
        assert np.array_equal(_bits(depth), _bits(want)), (fmt, step, near, int((_bits(depth) != _bits(want)).sum()))
        assert np.array_equal(px, r.readPixels().ravel())
        r.close_delivery()
    if name == "C2":          # the quantiser meets hits on both sides of near
        u = DD.quantise_u16(hit, 6.0)
        assert (u == 65535).any() and (u == 0).any() and ((u > 0) & (u < 65535)).any()
    r.dispose()


_SKIP_CHILD = r"""
import sys, hashlib, json
sys.path[:0] = [%r, %r]
import numpy as np
import gsplat_hip as gh
cfg = gh.synth.CONFIGS["C2"]
r = gh.HIPRenderer(cfg["width"], cfg["height"])
r.set_scene_rows(gh.synth.config_rows("C2"))
out = {}
for step in (1, 2):
    r.open_delivery_depth(2, depth="f32", depth_step=step)
    r.set_camera(gh.orbit_camera(13, width=cfg["width"], height=cfg["height"], fx=cfg["fx"]))
    r.render_async()
    s, px, depth = r.acquire(r.deliver())
    out[str(step)] = hashlib.sha256(depth.tobytes()).hexdigest()
    r.release(s)
    r.close_delivery()
r.dispose()
print(json.dumps(out))
"""


def test_without_the_tile_skip_the_same_bytes(gh):
    """GSR_DEPTH_SKIP=0 is read when a context is created: a child process per setting"""
    got = {}
    for skip in ("1", "0"):
        env = dict(os.environ, GSR_DEPTH_SKIP=skip)
        out = subprocess.run([sys.executable, "-c", _SKIP_CHILD % (ROOT, os.path.join(ROOT, "gsplat.js_amd", "py"))], capture_output=True, text=True,
                             env=env, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        got[skip] = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["0"] == got["1"] and got["1"]["1"] != got["1"]["2"]


# ---- 4. the colour beside it ----
@pytest.mark.parametrize("fmt", ["rgba8", "nv12", "i420"])
@pytest.mark.parametrize("size", [None, (1001, 701), (23, 9)])
def test_colour_payload_and_layout_are_those_of_the_ring_without_depth(gh, scenes, fmt, size):
    r, cfg, W, H = _renderer(gh, scenes, "C1", size)
    r.set_camera(_camera(gh, 21, cfg, W, H))
    kw = dict(format=fmt, full_range=True, background=(255, 128, 7)) if fmt != "rgba8" else dict(format=fmt)
    r.open_delivery(2, **kw)
    plain_layout = r.delivery_layout()
    r.render_async()
    s, px = r.acquire(r.deliver())
    plain = _colour(px)
    r.release(s)
    nbytes = ctypes.c_uint64()
    r._L.gsr_delivery_slot_ptr(r._ctx, 0, ctypes.byref(nbytes))
    with pytest.raises(gh.GsplatError):
        r.depth_layout()                                 # a ring without depth has none
    r.close_delivery()
    for dfmt, step in (("u16", 2), ("f32", 1)):
        r.open_delivery_depth(2, depth=dfmt, depth_step=step, **kw)
        assert r.delivery_layout() == plain_layout
        got_bytes = ctypes.c_uint64()
        r._L.gsr_delivery_slot_ptr(r._ctx, 0, ctypes.byref(got_bytes))
        assert got_bytes.value == nbytes.value == plain_layout["bytes"]
        s, colour, depth = _deliver_one(r)
        assert np.array_equal(colour, plain), (fmt, dfmt, step)
        r.close_delivery()
    r.dispose()


# ---- 5. frames in flight ----
@pytest.mark.parametrize("throughput", [False, True])
def test_every_serial_carries_its_own_poses_depth(gh, scenes, throughput):
    r, cfg, W, H = _renderer(gh, scenes, "C2", throughput=throughput)
    ref, _, _, _ = _renderer(gh, scenes, "C2")
    poses = [5, 25, 45, 65, 85, 105, 115, 10]
    r.open_delivery_depth(3, format="nv12", depth="u16", depth_step=2, depth_near=0.5)
    got, pending = {}, []

    def pick_up():
        s, px, depth = r.acquire(pending.pop(0))
        got[s] = (_colour(px), depth.copy())
        r.release(s)

    for j, k in enumerate(poses):
        if len(pending) == 3:                             # acquiring late: only when the ring is full ...
            pick_up()
            if j % 2:                                     # ... and out of step with rendering
                pick_up()
        r.set_camera(_camera(gh, k, cfg))
        r.render_async()
        pending.append(r.deliver())
    while pending:
        pick_up()
    assert sorted(got) == list(range(1, len(poses) + 1))
    planes = []
    for s, k in enumerate(poses, 1):
        ref.set_camera(_camera(gh, k, cfg))
        ref.render_async()
        want = _want(ref.read_depth()[1], "u16", 2, 0.5)
        assert np.array_equal(got[s][1], want), (s, k)
        planes.append(want)
    assert not np.array_equal(planes[0], planes[1])
    r.dispose(); ref.dispose()


# ---- 6. hit_alpha, and the planes cache is left alone ----
def test_hit_alpha_of_the_call_and_read_depth_undisturbed(gh, scenes):
    r, cfg, W, H = _renderer(gh, scenes, "C1")
    r.set_camera(_camera(gh, 3, cfg))
    r.render_async()
    before = r.read_depth()
    points = [(320, 240), (100, 77), (0, 0), (639, 479)]
    picked = r.pick(points)
    ptrs = [r._L.gsr_depth_device_ptr(r._ctx, p) for p in range(3)]
    r.open_delivery_depth(2, depth="f32", depth_step=2)
    s, _, half = _deliver_one(r)
    assert np.array_equal(_bits(half), _bits(before[1][::2, ::2]))
    assert [r._L.gsr_depth_device_ptr(r._ctx, p) for p in range(3)] == ptrs
    r.set_hit_alpha(0.05)
    s, _, early = _deliver_one(r)                        # the same pose, rendered again
    r.set_hit_alpha(0.5)
    s, _, again = _deliver_one(r)
    assert np.array_equal(_bits(again), _bits(half)) and not np.array_equal(_bits(early), _bits(half))
    assert np.isfinite(early).sum() > np.isfinite(half).sum()    # a lower threshold is reached wherever the higher one is, and in more pixels
    after = r.read_depth()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, after))
    assert np.array_equal(r.pick(points), picked)
    r.set_hit_alpha(0.05)
    assert np.array_equal(_bits(r.read_depth()[1][::2, ::2]), _bits(early))
    r.dispose()


# ---- 7. a band context ----
def test_band_context_delivers_its_columns_and_nothing_outside(gh, scenes):
    full, cfg, W, H = _renderer(gh, scenes, "C2")
    x0, x1 = 864, 1056
    band, _, _, _ = _renderer(gh, scenes, "C2", band=(x0, x1))
    cam = _camera(gh, 13, cfg)
    full.set_camera(cam); band.set_camera(cam)
    full.render_async()
    hit = full.read_depth()[1]
    for fmt, step, empty in (("f32", 1, np.float32(np.inf)), ("f32", 2, np.float32(np.inf)), ("u16", 2, np.uint16(0)), ("u16", 1, np.uint16(0))):
        band.open_delivery_depth(2, depth=fmt, depth_step=step, depth_near=0.5)
        for _ in range(2):                                # (the second frame finds the other columns filled already)
            s, _, depth = _deliver_one(band)
            want = _want(hit, fmt, step, 0.5)
            inside = np.zeros(W, bool)
            inside[x0:x1] = True
            inside = inside[::step]
            assert np.array_equal(_bits(depth[:, inside]), _bits(want[:, inside])), (fmt, step)
            assert (depth[:, ~inside] == empty).all() and np.isfinite(hit[:, x0:x1]).any()
        band.close_delivery()
    full.dispose(); band.dispose()


def test_band_moves_under_an_open_ring(gh, scenes):
    """The band moves while the ring -- and the context's own planes -- stay as they are: the columns the band left hold "nothing" again,
    in the delivered plane (+inf, or 0 as u16) and in read_depth() (0, +inf, none: what test_gpu_depth.py::test_band_context asserts)."""
    W, H = 192, 96
    rows, data, pos = scenes(4000, 21)
    cam = gh.orbit_camera(3, width=W, height=H)
    full = gh.HIPRenderer(W, H)
    full.set_raw_scene(data, pos)
    full.set_camera(cam)
    full.render_async()
    planes = full.read_depth()
    hit = planes[1]
    bands = [(32, 96), (96, 160), (0, 0)]
    assert all(np.isfinite(hit[:, x0:x1]).any() and np.isinf(hit[:, x0:x1]).any() for x0, x1 in bands[:2])
    none = (np.float32(0).view(np.uint32), np.float32(np.inf).view(np.uint32), np.uint32(0xFFFFFFFF))
    for fmt, step, empty in (("f32", 1, np.float32(np.inf)), ("u16", 2, np.uint16(0))):
        band = gh.HIPRenderer(W, H, band=bands[0])
        band.set_raw_scene(data, pos)
        band.set_camera(cam)
        band.open_delivery_depth(2, depth=fmt, depth_step=step, depth_near=0.5)      # one ring, open throughout
        want = _want(hit, fmt, step, 0.5)
        for j, (x0, x1) in enumerate(bands):
            if j:
                band.set_band(x0, x1)
            s, _, depth = _deliver_one(band)
            inside = np.zeros(W, bool)
            inside[x0:x1 or W] = True
            assert s == j + 1 and depth.shape == want.shape
            assert np.array_equal(_bits(depth[:, inside[::step]]), _bits(want[:, inside[::step]])), (fmt, step, x0, x1)
            assert (depth[:, ~inside[::step]] == empty).all(), (fmt, step, x0, x1)
            for got, ref, rest in zip(band.read_depth(), planes, none):
                assert np.array_equal(got.view(np.uint32)[:, inside], ref.view(np.uint32)[:, inside]), (fmt, step, x0, x1)
                assert (got.view(np.uint32)[:, ~inside] == rest).all(), (fmt, step, x0, x1)
        band.close_delivery()
        band.dispose()
    full.dispose()


# ---- 8. the ring's promises ----
def test_busy_release_resize_close_reopen(gh, scenes):
    r, cfg, W, H = _renderer(gh, scenes, "C1")
    r.open_delivery_depth(2, format="i420", depth="u16", depth_step=2, depth_near=0.25)
    held = []
    for k in (0, 30):
        r.set_camera(_camera(gh, k, cfg))
        r.render_async()
        held.append(r.acquire(r.deliver()))
    r.set_camera(_camera(gh, 60, cfg))
    r.render_async()
    with pytest.raises(gh.GsplatError) as ei:
        r.deliver()                                      # every slot is held
    assert ei.value.code == gh.GSR_ERR_BUSY
    snap = held[0][2].copy()
    for refused in (lambda: r.setSize(320, 240), r.close_delivery):
        with pytest.raises(gh.GsplatError) as ei:
            refused()
        assert ei.value.code == GSR_ERR_ARG
    r.release(2)
    assert r.deliver() == 3                              # the refused call handed out no serial and enqueued nothing
    assert r.frame_ready(1) is True
    s, px, depth = r.acquire(3)
    assert np.array_equal(depth, _want(r.read_depth()[1], "u16", 2, 0.25))     # pose 60
    assert np.array_equal(held[0][2], snap)
    r.release(3); r.release(1)
    del held, px, depth
    r.setSize(323, 241)                                  # an idle ring follows the framebuffer, and so does the plane
    lay = r.depth_layout()
    colour = 323 * 241 + 2 * 162 * 121
    assert (lay["width"], lay["height"], lay["stride"], lay["bytes"], lay["offset"]) == (162, 121, 324, 324 * 121, (colour + 15) // 16 * 16)
    assert r.delivery_layout()["bytes"] == colour
    r.set_camera(_camera(gh, 5, cfg, 323, 241))
    s, _, depth = _deliver_one(r)
    assert s == 4 and np.array_equal(depth, _want(r.read_depth()[1], "u16", 2, 0.25))
    r.render_async(); r.deliver()                        # a frame nobody picks up: close waits for its copy and drops it
    r.close_delivery()
    with pytest.raises(gh.GsplatError):
        r.depth_layout()
    r.open_delivery(2)                                   # and a ring without depth again: two-tuples, no plane
    r.render_async()
    got = r.acquire(r.deliver())
    assert len(got) == 2 and got[0] == 6 and np.array_equal(got[1], r.readPixels())
    with pytest.raises(gh.GsplatError):
        r.depth_layout()
    r.release(6)
    r.render_async(); r.deliver()
    r.sync()                                             # waits for the copies as well
    r.close_delivery()
    r.open_delivery_depth(2, depth="f32")
    r.render_async(); r.deliver()
    r.dispose()                                          # a copy in flight


# ---- 9. overflow ----
def test_a_frame_that_did_not_fit_is_refused_and_the_pose_delivers_again(gh, scenes):
    rows, data, pos = scenes(60000, 21)
    W, H = 640, 480
    cams = [gh.orbit_camera(k, width=W, height=H) for k in (3, 9)]
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    r.open_delivery_depth(2, depth="f32", depth_step=2)
    r.set_camera(cams[0])
    s, _, first = _deliver_one(r)
    r.set_list_capacity(2048)                            # far too small for the next frame
    r.set_camera(cams[1])
    r.render_async()
    k = r.deliver()
    with pytest.raises(gh.GsplatError, match="frame %d was not composited" % k) as ei:
        r.acquire(k)
    assert ei.value.code == gh.GSR_ERR_OVERFLOW
    with pytest.raises(gh.GsplatError):
        r.release(k)                                     # the refused frame holds no slot
    got = {}
    for _ in range(2):                                   # the same pose again: the lists are regrown; both slots are free
        s, _, got[s] = _deliver_one(r)
    want = r.read_depth()[1][::2, ::2]
    assert sorted(got) == [k + 1, k + 2]
    assert all(np.array_equal(_bits(g), _bits(want)) for g in got.values()) and not np.array_equal(_bits(want), _bits(first))
    with pytest.raises(gh.GsplatError, match="not composited"):
        r.sync()                                         # the lost frame is reported once, as before
    r.sync()
    r.dispose()


# ---- 10. refusals ----
def test_refusals(gh, scenes):
    r, cfg, W, H = _renderer(gh, scenes, "C1")
    L = r._L
    opt = gh.GsrDeliveryOptions(2, gh.GSR_FORMAT_RGBA8, 0, (ctypes.c_uint8 * 4)())

    def open_raw(fmt, step, near, reserved=0):
        d = gh.GsrDepthDeliveryOptions(fmt, step, near, reserved)
        return L.gsr_delivery_open_depth(r._ctx, ctypes.byref(opt), ctypes.byref(d))

    for args in ((1, 3, 0.1), (1, 4, 0.1), (2, 0, 0.1), (3, 1, 0.1), (-1, 1, 0.1), (2, 1, 0.0), (2, 2, -1.0), (2, 1, float("nan")), (2, 1, float("inf")),
                 (1, 1, 0.1, 7)):
        assert open_raw(*args) == GSR_ERR_ARG, args
        lay = gh.GsrDepthLayout()
        assert L.gsr_delivery_depth_layout(r._ctx, ctypes.byref(lay)) == GSR_ERR_ARG     # nothing was opened
    assert L.gsr_delivery_open_depth(r._ctx, None, None) == GSR_ERR_ARG
    with pytest.raises(ValueError):
        r.open_delivery_depth(2, depth="u8")
    assert open_raw(1, 1, float("nan")) == 0              # near is ignored for F32 ...
    r.close_delivery()
    assert L.gsr_delivery_open_depth(r._ctx, ctypes.byref(opt), None) == 0                # ... and no depth options: gsr_delivery_open_ex
    assert L.gsr_delivery_depth_layout(r._ctx, ctypes.byref(gh.GsrDepthLayout())) == GSR_ERR_ARG
    r.close_delivery()
    assert open_raw(0, 9, -1.0) == 0                      # GSR_DEPTH_NONE likewise, whatever else the struct holds
    r.close_delivery()

    r.open_delivery_depth(2, depth="u16", depth_step=2)
    with pytest.raises(gh.GsplatError) as ei:
        r.open_delivery_depth(2, depth="f32")            # a ring is open
    assert ei.value.code == GSR_ERR_ARG and r.depth_layout()["format"] == "u16"

    def refused(match):
        with pytest.raises(gh.GsplatError, match=match) as ei:
            r.deliver()
        assert ei.value.code == GSR_ERR_ARG

    refused("no frame|nothing rendered")                 # nothing rendered yet
    r.set_camera(_camera(gh, 3, cfg))
    r.render_async()
    assert r.deliver() == 1                              # (and the refusals above took neither a serial nor a slot)
    r.sort()
    refused("sort-only")
    r.render_async()
    r.set_raw_scene(*scenes("C1")[1:])                   # the scene changed since the frame
    refused("no frame|nothing rendered")
    r.render_async()
    assert r.deliver() == 2
    s, _, depth = r.acquire(2)
    assert np.array_equal(depth, _want(r.read_depth()[1], "u16", 2, 0.1))
    r.release(2)
    s, _, _ = r.acquire(1)
    r.release(1)
    # a context in a group: depth is not exchanged between ranks
    world = 2

    def allgather(send, recv, nbytes, stream):           # never called: no frame is gathered here
        raise AssertionError

    from gsplat_hip import bands
    edges = bands.band_edges(W, world)
    r.join_group_custom(0, world, edges, allgather)      # joined AFTER the depth ring was opened: the delivery is refused
    r.render_async()
    refused("depth is not exchanged between ranks")
    r.close_delivery()
    with pytest.raises(gh.GsplatError, match="depth is not exchanged between ranks") as ei:
        r.open_delivery_depth(2, depth="u16")
    assert ei.value.code == GSR_ERR_ARG
    r.open_delivery(2)                                   # a ring without depth is what a group delivers
    r.close_delivery()
    r.leave_group()
    r.open_delivery_depth(2, depth="u16")
    r.set_camera(_camera(gh, 3, cfg))
    r.render_async()
    assert r.deliver() == 3
    r.dispose()


# ---- 11. the bounds twin ----
def test_bounds_twin_counts_nothing(gh, scenes):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    r = gh.HIPRenderer(cfg["width"], cfg["height"], lib_path=BOUNDS_LIB)
    r.set_raw_scene(data, pos)
    frames = 0
    for W, H in [(640, 480), (1001, 701), (23, 9), (7, 1), (1, 1)]:
        r.setSize(W, H)
        r.set_camera(_camera(gh, 17, cfg, W, H))
        for fmt, step, colour in (("u16", 2, "nv12"), ("f32", 2, "rgba8"), ("u16", 1, "i420"), ("f32", 1, "rgba8")):
            r.open_delivery_depth(2, format=colour, depth=fmt, depth_step=step)
            s, _, depth = _deliver_one(r)
            assert np.array_equal(_bits(depth), _bits(_want(r.read_depth()[1], fmt, step, 0.1))), (W, H, fmt, step)
            r.close_delivery()
            frames += 1
    counters = {}
    for name in ("depth", "deliver"):
        buf = (ctypes.c_uint32 * 8)()
        assert getattr(r._L, "gsr_debug_bounds_" + name)(buf) == 0
        counters[name] = list(buf)
    r.dispose()
    assert counters == {"depth": [0] * 8, "deliver": [0] * 8} and frames == 20, counters


# ---- the C++ host and the measurement ----
def _fnv1a(b):
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_cpp_caller_delivers_the_plane_the_python_host_delivers(gh, scenes, tmp_path):
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    f = tmp_path / "c1.splat"
    f.write_bytes(np.asarray(rows, dtype=np.uint8).tobytes())
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    out = subprocess.run([exe, "--config", "C1", "--rows", str(f), "--frames", "30", "--warmup", "5", "--in-flight", "1", "--deliver",
                          "--deliver-depth", "u16", "--depth-step", "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["frames_per_sec_delivered"] > 0 and line["delivery_depth"] == "u16" and line["depth_step"] == 2
    assert (line["depth_width"], line["depth_height"], line["depth_bytes"]) == (320, 240, 320 * 240 * 2)
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_raw_scene(data, pos)
    r.open_delivery_depth(3, depth="u16", depth_step=2)
    r.set_camera(_camera(gh, 0, cfg))
    s, colour, depth = _deliver_one(r)
    assert np.array_equal(depth, _want(r.read_depth()[1], "u16", 2, 0.1))
    assert _fnv1a(depth.tobytes()) == line["delivered_depth_fnv1a"] and _fnv1a(colour.tobytes()) == line["delivered_rgba8_fnv1a"]
    r.dispose()


def test_bench_delivery_prints_one_line_with_checked_planes(gh):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_delivery.py"), "--config", "C1", "--frames", "24", "--warmup", "6",
                          "--other", "", "--format", "nv12", "--depth", "u16", "--depth-step", "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["depth"] == "u16" and line["depth_step"] == 2 and line["depth_bytes_per_frame"] == 320 * 240 * 2 and line["format"] == "nv12"
    assert line["delivered"]["delivered_depth_equals_reference"] is True and line["delivered_in_flight"]["delivered_depth_equals_reference"] is True
    assert line["value"] > 0

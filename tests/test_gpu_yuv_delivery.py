"""Frame delivery in 4:2:0 Y'CbCr (gsr_delivery_open_ex: NV12 / I420).  The bar everywhere: a delivered payload is, byte for byte,
the definition in plain numpy (tests/yuv_reference.py) applied to what gsr_read_pixels_rgba8 (in a group: gsr_read_frame_rgba8)
returns for the same frame; and everything the ring promises for RGBA8 holds for every format."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import yuv_reference as yr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
SIZES = [(1920, 1080), (640, 480), (1001, 713), (33, 17), (1, 1)]      # (1 x 1: the smallest size gsr_resize accepts)
BACKGROUND = (255, 128, 7)


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _camera(gh, k, cfg, W=None, H=None):
    W, H = W or cfg["width"], H or cfg["height"]
    return gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"] * W / cfg["width"])


def _bytes(planes):
    return np.concatenate([p.ravel() for p in planes])


def _check_planes(planes, fmt, W, H):
    Wc, Hc = (W + 1) // 2, (H + 1) // 2
    want = [(H, W), (Hc, Wc, 2)] if fmt == "nv12" else [(H, W), (Hc, Wc), (Hc, Wc)]
    assert [p.shape for p in planes] == want and all(p.dtype == np.uint8 and not p.flags.writeable for p in planes)
    base = planes[0].ctypes.data
    assert [p.ctypes.data - base for p in planes] == [off for off, _, _ in yr.layout(W, H, fmt)["planes"]]


def _deliver_one(r, fmt):
    """render_async + deliver + acquire of the current camera's frame: (serial, a copy of the payload)"""
    r.render_async()
    k = r.deliver()
    s, planes = r.acquire(k)
    assert s == k
    _check_planes(planes, fmt, r.width, r.height)
    got = _bytes(planes)
    r.release(s)
    return s, got


# ---- 1. bytes ----
@pytest.mark.parametrize("config,throughput", [("C1", False), ("C1", True), ("C2", False), ("C2", True)])
def test_payload_equals_the_reference_of_read_pixels(gh, scenes, config, throughput):
    cfg = gh.synth.CONFIGS[config]
    rows, data, pos = scenes(config)
    r = gh.HIPRenderer(cfg["width"], cfg["height"], throughput=throughput)
    r.set_raw_scene(data, pos)
    frames = 0
    for W, H in SIZES:
        r.setSize(W, H)
        r.set_camera(_camera(gh, 17, cfg, W, H))
        for fmt in ("nv12", "i420"):
            for full_range in (False, True):
                for bg in ((0, 0, 0), BACKGROUND):
                    r.open_delivery(2, format=fmt, full_range=full_range, background=bg)
                    lay = r.delivery_layout()
                    ref = yr.layout(W, H, fmt)
                    assert (lay["format"], lay["width"], lay["height"], lay["bytes"]) == (fmt, W, H, ref["bytes"])
                    assert [(p["offset"], p["stride"], p["rows"]) for p in lay["planes"]] == ref["planes"]
                    nbytes = ctypes.c_uint64(0)
                    assert r._L.gsr_delivery_slot_ptr(r._ctx, 0, ctypes.byref(nbytes)) and nbytes.value == ref["bytes"]
                    s, got = _deliver_one(r, fmt)
                    rgba = r.readPixels()          # nothing was enqueued behind the frame: the framebuffer still holds it
                    want = yr.payload(rgba, fmt, full_range, bg)
                    assert got.size == want.size and np.array_equal(got, want), (W, H, fmt, full_range, bg, np.flatnonzero(got != want)[:8])
                    r.close_delivery()
                    frames += 1
        if W >= 640:
            assert rgba[..., 3].min() < 255 and rgba.any()    # (translucent pixels: the background shows through)
    assert frames == len(SIZES) * 8
    r.dispose()


def test_rgba8_ring_through_open_ex_equals_the_plain_one(gh, scenes):
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    W, H = cfg["width"], cfg["height"]
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    r.set_camera(_camera(gh, 40, cfg))
    got = []
    for ex in (False, True):
        if ex:
            opt = gh.GsrDeliveryOptions(3, gh.GSR_FORMAT_RGBA8, 1, (ctypes.c_uint8 * 4)(9, 9, 9, 9))    # (range and background: Y'CbCr only)
            assert r._L.gsr_delivery_open_ex(r._ctx, ctypes.byref(opt)) == 0
        else:
            r.open_delivery(3)
        lay = r.delivery_layout()
        assert lay == {"format": "rgba8", "width": W, "height": H, "bytes": W * H * 4, "planes": [{"offset": 0, "stride": W * 4, "rows": H}]}
        r.render_async()
        s, px = r.acquire(r.deliver())
        assert px.shape == (H, W, 4)
        got.append(px.copy())
        r.release(s)
        r.close_delivery()
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], r.readPixels()) and got[0].any()
    r.dispose()


# ---- 2. pipelining ----
def _pipelined(r, cams, slots):
    pending, got = [], {}
    for cam in cams:
        if len(pending) == slots:
            s, planes = r.acquire(pending[0])
            assert s == pending.pop(0)
            got[s] = _bytes(planes)
            r.release(s)
        r.set_camera(cam)
        r.render_async()
        pending.append(r.deliver())
    while pending:
        s, planes = r.acquire()            # serial 0: the oldest frame not acquired yet
        assert s == pending.pop(0) and r.frame_ready(s)
        got[s] = _bytes(planes)
        r.release(s)
    return got


@pytest.mark.parametrize("slots,fmt", [(2, "nv12"), (3, "i420")])
def test_pipelined_frames_equal_blocking_renders(gh, scenes, slots, fmt):
    cfg = gh.synth.CONFIGS["C2"]
    rows, data, pos = scenes("C2")
    cams = [_camera(gh, k, cfg) for k in range(0, 120, 10)]
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_raw_scene(data, pos)
    r.open_delivery(slots, format=fmt)
    got = _pipelined(r, cams, slots)
    assert sorted(got) == list(range(1, 13))
    for k, cam in enumerate(cams):
        r.set_camera(cam)
        r.render_async(); r.sync()
        assert np.array_equal(got[k + 1], yr.payload(r.readPixels(), fmt)), k
    r.dispose()


def test_three_contexts_in_flight_each_with_its_own_ring(gh, scenes):
    cfg = gh.synth.CONFIGS["C2"]
    rows, data, pos = scenes("C2")
    cams = [_camera(gh, k, cfg) for k in range(0, 120, 10)]
    rs = [gh.HIPRenderer(cfg["width"], cfg["height"], throughput=True) for _ in range(3)]
    for r in rs:
        r.set_raw_scene(data, pos)
        r.open_delivery(2, format="nv12")
    pending, got = [[] for _ in rs], {}
    for n, cam in enumerate(cams):
        q = n % 3
        r = rs[q]
        if len(pending[q]) == 2:
            m, k = pending[q].pop(0)
            s, planes = r.acquire(k)
            got[m] = _bytes(planes)
            r.release(s)
        r.set_camera(cam)
        r.render_async()
        pending[q].append((n, r.deliver()))
    for q, r in enumerate(rs):
        for m, k in pending[q]:
            s, planes = r.acquire(k)
            got[m] = _bytes(planes)
            r.release(s)
    ref = rs[0]
    for n, cam in enumerate(cams):
        ref.set_camera(cam)
        ref.render_async(); ref.sync()
        assert np.array_equal(got[n], yr.payload(ref.readPixels(), "nv12")), n
    for r in rs:
        r.dispose()


# ---- 3. hold ----
def test_held_frame_is_stable_and_a_full_ring_is_busy(gh, scenes):
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_raw_scene(data, pos)
    r.open_delivery(3, format="i420")
    held = []
    for k in (0, 30, 60):
        r.set_camera(_camera(gh, k, cfg))
        r.render_async()
        held.append(r.acquire(r.deliver()))
    assert [s for s, _ in held] == [1, 2, 3]
    r.set_camera(_camera(gh, 90, cfg))
    r.render_async()
    with pytest.raises(gh.GsplatError) as ei:
        r.deliver()                                     # every slot is held
    assert ei.value.code == gh.GSR_ERR_BUSY
    s1, planes1 = held[0]
    snap, addr = _bytes(planes1), planes1[0].ctypes.data
    r.release(2)
    assert r.deliver() == 4                             # the refused call handed out no serial
    s, planes = r.acquire(4)
    assert np.array_equal(_bytes(planes), yr.payload(r.readPixels(), "i420"))
    r.release(4)
    r.release(3)
    for k in (15, 45, 75, 105):                         # four more frames around the held one
        r.set_camera(_camera(gh, k, cfg))
        s, got = _deliver_one(r, "i420")
        assert np.array_equal(got, yr.payload(r.readPixels(), "i420"))
    assert s == 8
    assert planes1[0].ctypes.data == addr and np.array_equal(_bytes(planes1), snap)
    r.set_camera(_camera(gh, 0, cfg))
    r.render_async(); r.sync()
    assert np.array_equal(snap, yr.payload(r.readPixels(), "i420"))
    r.release(1)
    r.dispose()


# ---- 4. overflow ----
def test_a_frame_that_was_not_composited_is_refused_and_its_slot_freed(gh, scenes):
    rows, data, pos = scenes(60000, 21)
    W, H = 640, 480
    cams = [gh.orbit_camera(k, width=W, height=H) for k in (3, 9)]
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    r.open_delivery(2, format="nv12")
    r.set_camera(cams[0])
    s, first = _deliver_one(r, "nv12")
    r.set_list_capacity(2048)                           # far too small for the next frame
    r.set_camera(cams[1])
    r.render_async()
    k = r.deliver()
    with pytest.raises(gh.GsplatError, match="frame %d was not composited" % k) as ei:
        r.acquire(k)
    assert ei.value.code == gh.GSR_ERR_OVERFLOW
    with pytest.raises(gh.GsplatError):
        r.release(k)                                    # the refused frame holds no slot
    got = {}
    for _ in range(2):                                  # the same pose again: the lists are regrown; both slots are free
        s, got[s] = _deliver_one(r, "nv12")
    want = yr.payload(r.readPixels(), "nv12")
    assert sorted(got) == [k + 1, k + 2]
    assert np.array_equal(got[k + 1], want) and np.array_equal(got[k + 2], want) and not np.array_equal(want, first)
    with pytest.raises(gh.GsplatError, match="not composited"):
        r.sync()                                        # the lost frame is reported once, as before
    r.sync()
    r.dispose()


# ---- 5. lifetime ----
def test_open_is_checked_and_resize_gives_the_new_layout(gh, scenes):
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    W, H = cfg["width"], cfg["height"]
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    lay = gh.GsrFrameLayout()
    assert r._L.gsr_delivery_layout(r._ctx, ctypes.byref(lay)) == -1          # no ring
    assert r._L.gsr_delivery_open_ex(r._ctx, None) == -1
    for slots, fmt in ((1, 1), (9, 2), (3, 3), (3, -1)):
        opt = gh.GsrDeliveryOptions(slots, fmt, 0, (ctypes.c_uint8 * 4)())
        assert r._L.gsr_delivery_open_ex(r._ctx, ctypes.byref(opt)) == -1, (slots, fmt)
    with pytest.raises(ValueError):
        r.open_delivery(3, format="yuv9")
    r.open_delivery(2, format="nv12")
    with pytest.raises(gh.GsplatError) as ei:
        r.open_delivery(2, format="i420")               # a ring is open
    assert ei.value.code == -1 and r.delivery_layout()["format"] == "nv12"
    r.set_camera(_camera(gh, 5, cfg))
    r.render_async()
    s, planes = r.acquire(r.deliver())
    snap = _bytes(planes)
    for refused in (lambda: r.setSize(320, 240), r.close_delivery):
        with pytest.raises(gh.GsplatError) as ei:
            refused()
        assert ei.value.code == -1
    assert np.array_equal(_bytes(planes), snap)
    r.release(s)
    del planes
    r.setSize(323, 241)                                 # an idle ring follows the framebuffer, in its format
    lay = r.delivery_layout()
    assert (lay["format"], lay["width"], lay["height"], lay["bytes"]) == ("nv12", 323, 241, 323 * 241 + 2 * 162 * 121)
    assert [(p["offset"], p["stride"], p["rows"]) for p in lay["planes"]] == [(0, 323, 241), (323 * 241, 324, 121)]
    r.set_camera(_camera(gh, 5, cfg, 323, 241))
    s2, got = _deliver_one(r, "nv12")
    assert s2 == s + 1 and np.array_equal(got, yr.payload(r.readPixels(), "nv12")) and got[:323 * 241].max() > 16
    r.render_async(); r.deliver()                       # a frame nobody picks up: close waits for its copy and drops it
    r.close_delivery()
    r.open_delivery(2, format="i420", full_range=True)
    assert _deliver_one(r, "i420")[0] == s2 + 2         # serials never restart
    r.render_async(); r.deliver()
    r.render_async(); r.deliver()
    r.dispose()                                         # copies in flight


# ---- 6. group ----
def test_delivery_of_the_gathered_frame_single_rank_rccl(gh, scenes):
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    W, H = cfg["width"], cfg["height"]
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    r.open_delivery(3, format="nv12", background=BACKGROUND)
    r.join_group(gh.new_group_id(), 0, 1, [(0, W)])
    with pytest.raises(gh.GsplatError):
        r.deliver()                                     # nothing gathered yet
    cams = [_camera(gh, k, cfg) for k in (5, 41, 77)]
    serials, frames = [], []
    for cam in cams:                                    # back to back: the next de-slab must not overtake a conversion
        r.set_camera(cam)
        r.render_async()
        r.allgather_frame_async()
        serials.append(r.deliver())
    last = r.read_frame()
    ref = gh.HIPRenderer(W, H)
    ref.set_raw_scene(data, pos)
    for k, cam in zip(serials, cams):
        s, planes = r.acquire(k)
        _check_planes(planes, "nv12", W, H)
        ref.set_camera(cam)
        ref.render_async(); ref.sync()
        assert np.array_equal(_bytes(planes), yr.payload(ref.readPixels(), "nv12", background=BACKGROUND)), k
        if k == serials[-1]:
            assert np.array_equal(_bytes(planes), yr.payload(last, "nv12", background=BACKGROUND))
        r.release(s)
    # a gathered frame with a stale band is refused where gsr_read_frame_rgba8 refuses it
    r.sync()
    r.set_list_capacity(1024)
    r.set_camera(_camera(gh, 60, cfg))
    r.render_async()
    r.allgather_frame_async()
    k = r.deliver()
    with pytest.raises(gh.GsplatError, match="not composited") as ei:
        r.acquire(k)
    assert ei.value.code == gh.GSR_ERR_OVERFLOW
    with pytest.raises(gh.GsplatError, match="not composited"):
        r.read_frame()
    r.render_async()                                    # the lists have been regrown
    r.allgather_frame_async()
    s, planes = r.acquire(r.deliver())
    assert np.array_equal(_bytes(planes), yr.payload(r.read_frame(), "nv12", background=BACKGROUND))
    r.release(s)
    r.leave_group()                                     # a plain context again: the ring delivers its own framebuffer
    r.set_camera(cams[0])
    s, got = _deliver_one(r, "nv12")
    assert np.array_equal(got, yr.payload(r.readPixels(), "nv12", background=BACKGROUND))
    r.dispose(); ref.dispose()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _group_worker(rank, world, port, out):
    """world > 1 on one GPU the way tests/test_gpu_delivery.py does it: the collective injected through gsr_comm_init_custom as a
    host-staged gloo all-gather, everything around it the product path."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "gsplat.js_amd", "py"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    import gsplat_hip as gh
    import yuv_reference as yr
    from gsplat_hip import bands
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = gh.synth.CONFIGS["C1"]
        W, H = cfg["width"], cfg["height"]
        scene = gh.Scene()
        scene.setData(gh.synth.config_rows("C1"))
        cams = [gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"]) for k in (3, 38, 71)]
        cal = gh.HIPRenderer(W, H, device=0)
        edges = bands.band_edges(W, world)
        dev = torch.device("cuda:0")

        def allgather(send, recv, nbytes, stream):
            s = torch.cuda.ExternalStream(stream, device=dev)
            s.synchronize()
            mine = torch.as_tensor(bands.DevicePointer(send, (nbytes,), "|u1"), device=dev).cpu()
            every = torch.empty(world * nbytes, dtype=torch.uint8)
            dist.all_gather_into_tensor(every, mine)
            with torch.cuda.stream(s):
                torch.as_tensor(bands.DevicePointer(recv, (world * nbytes,), "|u1"), device=dev).copy_(every)
            s.synchronize()

        a = gh.HIPRenderer(W, H, device=0)
        a.join_group_custom(rank, world, edges, allgather)
        a.open_delivery(2, format="i420", full_range=True)
        a.render(scene, cams[0])
        ok = True
        serials = []
        for cam in cams[:2]:                                 # two frames back to back through a ring of two
            a.set_camera(cam)
            a.render_async()
            a.allgather_frame_async()
            serials.append(a.deliver())
        last = a.read_frame()
        for k, cam in zip(serials, cams):
            s, planes = a.acquire(k)
            got = np.concatenate([p.ravel() for p in planes])
            cal.render(scene, cam)
            ok = ok and np.array_equal(got, yr.payload(cal.readPixels(), "i420", True))
            if k == serials[-1]:
                ok = ok and np.array_equal(got, yr.payload(last, "i420", True))
            a.release(s)
        # one rank's lists overflow: every rank's delivered frame carries the stale band and every rank refuses it
        a.sync()
        if rank == world - 1:
            a.set_list_capacity(1024)
        a.set_camera(cams[2])
        a.render_async()
        a.allgather_frame_async()
        k = a.deliver()
        try:
            a.acquire(k)
            ok = False
        except gh.GsplatError as e:
            ok = ok and e.code == gh.GSR_ERR_OVERFLOW
        a.render_async()
        a.allgather_frame_async()
        s, planes = a.acquire(a.deliver())
        cal.render(scene, cams[2])
        ok = ok and np.array_equal(np.concatenate([p.ravel() for p in planes]), yr.payload(cal.readPixels(), "i420", True))
        a.release(s)
        try:
            a.sync()
        except gh.GsplatError:
            pass                                             # (the overflowing rank reports its lost frame once)
        a.dispose(); cal.dispose()
        res = torch.tensor([1 if ok else 0])
        dist.all_reduce(res, op=dist.ReduceOp.MIN)
        if rank == 0:
            open(out, "w").write("ok" if int(res.item()) == 1 else "mismatch")
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_delivery_of_the_gathered_frame_in_a_larger_world(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "result.txt")
    mp.spawn(_group_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert open(out).read() == "ok"


# ---- 7. the bounds twin ----
def test_bounds_twin_counts_nothing(gh, scenes):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    r = gh.HIPRenderer(cfg["width"], cfg["height"], lib_path=BOUNDS_LIB)
    r.set_raw_scene(data, pos)
    frames = 0
    for W, H in [(640, 480), (648, 481), (1001, 713), (33, 17), (8, 2), (7, 1), (1, 1)]:
        r.setSize(W, H)
        r.set_camera(_camera(gh, 17, cfg, W, H))
        for fmt in ("nv12", "i420"):
            r.open_delivery(2, format=fmt, background=BACKGROUND)
            s, got = _deliver_one(r, fmt)
            assert np.array_equal(got, yr.payload(r.readPixels(), fmt, background=BACKGROUND)), (W, H, fmt)
            r.close_delivery()
            frames += 1
    r.setSize(cfg["width"], cfg["height"])
    r.open_delivery(2, format="nv12")
    r.join_group(gh.new_group_id(), 0, 1, [(0, cfg["width"])])     # the RGBA8 source
    r.set_camera(_camera(gh, 17, cfg))
    r.render_async()
    r.allgather_frame_async()
    s, planes = r.acquire(r.deliver())
    assert np.array_equal(_bytes(planes), yr.payload(r.read_frame(), "nv12"))
    r.release(s)
    buf = (ctypes.c_uint32 * 8)()
    assert r._L.gsr_debug_bounds_deliver(buf) == 0
    r.dispose()
    assert list(buf) == [0] * 8 and frames == 14, list(buf)


# ---- 8. the C++ host and the measurement ----
def _fnv1a(b):
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_cpp_caller_delivers_what_the_python_host_delivers(gh, scenes, tmp_path, fmt):
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    f = tmp_path / "c1.splat"
    f.write_bytes(np.asarray(rows, dtype=np.uint8).tobytes())
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    for in_flight in ("3", "1"):           # (one frame in flight: a default context, the kind the Python host below composites with)
        out = subprocess.run([exe, "--config", "C1", "--rows", str(f), "--frames", "30", "--warmup", "5", "--in-flight", in_flight, "--deliver",
                              "--deliver-format", fmt], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line["frames_per_sec_delivered"] > 0 and line["delivery_format"] == fmt and "delivered_rgba8_fnv1a" not in line
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_raw_scene(data, pos)
    r.open_delivery(3, format=fmt)
    r.set_camera(_camera(gh, 0, cfg))
    s, got = _deliver_one(r, fmt)
    assert np.array_equal(got, yr.payload(r.readPixels(), fmt))
    assert _fnv1a(got) == line["delivered_payload_fnv1a"]
    r.dispose()


def test_bench_delivery_prints_one_line_with_checked_frames(gh):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_delivery.py"), "--config", "C1", "--frames", "24", "--warmup", "6",
                          "--other", "C2", "--format", "nv12"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["value"] == line["delivered"]["frames_per_sec"] > 0 and line["bytes_per_frame"] == 640 * 480 * 3 // 2 and line["format"] == "nv12"
    for leg in (line["delivered"], line["delivered_in_flight"], line["other_configs"]["C2"]["delivered"]):
        assert leg["frames_per_sec"] > 0 and leg["delivered_equals_reference"] is True
    assert line["delivered_in_flight"]["contexts"] == 3
    for key in ("render_only", "with_rgba8_readback", "frame_latency_ms", "delivered_frame_latency_ms"):
        assert key in line

"""Frame delivery (gsr_delivery_* / gsr_deliver_frame_async / gsr_acquire_frame): finished RGBA8 frames reach the host through
the library's ring of pinned blocks while the next frames render.  The bar everywhere: a delivered frame is, byte for byte,
what gsr_read_pixels_rgba8 (in a group: gsr_read_frame_rgba8) returns for the same frame."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _camera(gh, k, cfg):
    return gh.orbit_camera(k, width=cfg["width"], height=cfg["height"], fx=cfg["fx"])


def _deliver_one(r):
    """render_async + deliver + acquire of the current camera's frame: (serial, a copy of the pixels)"""
    r.render_async()
    k = r.deliver()
    s, px = r.acquire(k)
    assert s == k and px.shape == (r.height, r.width, 4) and px.dtype == np.uint8
    got = px.copy()
    r.release(s)
    return s, got


# ---- 1. bytes ----
@pytest.mark.parametrize("case", ["C1", "C2", "C3", "odd size", "empty scene", "sh colour", "throughput", "band"])
def test_delivered_frame_equals_read_pixels(gh, scenes, case):
    kw = {}
    scene = None
    if case in ("C1", "C2", "C3"):
        cfg = gh.synth.CONFIGS[case]
        rows, data, pos = scenes(case)
        W, H, cam = cfg["width"], cfg["height"], _camera(gh, 17, cfg)
    elif case == "odd size":          # 333 x 227 = 75591 pixels = 4 * 18897 + 3: the last lane converts three pixels one by one
        rows, data, pos = scenes(20000, 21)
        W, H = 333, 227
        cam = gh.orbit_camera(9, width=W, height=H, fx=400.0)
    elif case == "empty scene":
        data, pos = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32)
        W, H = 100, 50
        cam = gh.orbit_camera(0, width=W, height=H)
    elif case == "sh colour":
        n = 40000
        rows, data, pos = scenes(n, 41)
        shs = (np.random.default_rng(8).standard_normal((n - 10000, 48)) * 0.35).astype(np.float32)
        scene = gh.Scene()
        scene.bandsIndices = np.array([9999, 19999, 29999], dtype=np.int32)
        scene.setData(rows, shs)
        W, H = 640, 480
        cam = gh.orbit_camera(33, width=W, height=H)
    else:
        cfg = gh.synth.CONFIGS["C1"]
        rows, data, pos = scenes("C1")
        W, H, cam = cfg["width"], cfg["height"], _camera(gh, 40, cfg)
        kw = dict(throughput=True) if case == "throughput" else dict(band=(128, 416))
    assert case != "odd size" or (W * H) % 4 == 3
    r = gh.HIPRenderer(W, H, **kw)
    if scene is not None:
        r.render(scene, cam)
    else:
        r.set_raw_scene(data, pos)
        r.set_camera(cam)
    r.open_delivery(3)
    for lap in range(2):               # (the second frame goes through a slot of its own)
        s, got = _deliver_one(r)
        assert s == lap + 1
        want = r.readPixels()          # nothing was enqueued behind the frame: the framebuffer still holds it
        assert np.array_equal(got, want), case
    assert case == "empty scene" or got.any()
    r.dispose()


# ---- 2. pipelining ----
def _pipelined(gh, r, cams, slots):
    """every pose enqueued back to back through a ring of `slots`; the oldest frame is picked up (while the later ones are
    still enqueued) only when the ring is full: {serial: pixels}"""
    pending, got = [], {}
    for cam in cams:
        if len(pending) == slots:
            s, px = r.acquire(pending[0])
            assert s == pending.pop(0)
            got[s] = px.copy()
            r.release(s)
        r.set_camera(cam)
        r.render_async()
        pending.append(r.deliver())
    while pending:
        s, px = r.acquire()            # serial 0: the oldest frame not acquired yet
        assert s == pending.pop(0) and r.frame_ready(s)
        got[s] = px.copy()
        r.release(s)
    return got


@pytest.mark.parametrize("slots", [2, 3])
def test_pipelined_frames_equal_blocking_renders(gh, scenes, slots):
    cfg = gh.synth.CONFIGS["C2"]
    rows, data, pos = scenes("C2")
    W, H = cfg["width"], cfg["height"]
    cams = [_camera(gh, k, cfg) for k in range(0, 120, 10)]
    assert len(cams) == 12
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    r.open_delivery(slots)
    got = _pipelined(gh, r, cams, slots)
    assert sorted(got) == list(range(1, 13))
    for k, cam in enumerate(cams):
        r.set_camera(cam)
        r.render_async(); r.sync()
        assert np.array_equal(got[k + 1], r.readPixels()), k
    r.dispose()


def test_three_contexts_in_flight_each_with_its_own_ring(gh, scenes):
    cfg = gh.synth.CONFIGS["C2"]
    rows, data, pos = scenes("C2")
    W, H = cfg["width"], cfg["height"]
    cams = [_camera(gh, k, cfg) for k in range(0, 120, 10)]
    rs = [gh.HIPRenderer(W, H, throughput=True) for _ in range(3)]
    for r in rs:
        r.set_raw_scene(data, pos)
        r.open_delivery(2)
    pending, got = [[] for _ in rs], {}
    for n, cam in enumerate(cams):
        q = n % 3
        r = rs[q]
        if len(pending[q]) == 2:
            m, k = pending[q].pop(0)
            s, px = r.acquire(k)
            got[m] = px.copy()
            r.release(s)
        r.set_camera(cam)
        r.render_async()
        pending[q].append((n, r.deliver()))
    for q, r in enumerate(rs):
        for m, k in pending[q]:
            s, px = r.acquire(k)
            got[m] = px.copy()
            r.release(s)
    ref = rs[0]
    for n, cam in enumerate(cams):
        ref.set_camera(cam)
        ref.render_async(); ref.sync()
        assert np.array_equal(got[n], ref.readPixels()), n
    for r in rs:
        r.dispose()


# ---- 3. hold ----
def test_held_frame_is_stable_and_a_full_ring_is_busy(gh, scenes):
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    W, H = cfg["width"], cfg["height"]
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    r.open_delivery(3)
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
    s1, px1 = held[0]
    snap, addr = px1.copy(), px1.ctypes.data
    r.release(2)
    assert r.deliver() == 4                             # the refused call handed out no serial (and enqueued nothing)
    s, px = r.acquire(4)
    assert np.array_equal(px, r.readPixels())           # pose 90, through the slot frame 2 gave back
    r.release(4)
    r.release(3)
    for k in (15, 45, 75, 105):                         # four more frames around the held one
        r.set_camera(_camera(gh, k, cfg))
        s, got = _deliver_one(r)
        assert np.array_equal(got, r.readPixels())
    assert s == 8
    assert px1.ctypes.data == addr and np.array_equal(px1, snap)
    r.set_camera(_camera(gh, 0, cfg))
    r.render_async(); r.sync()
    assert np.array_equal(snap, r.readPixels())
    with pytest.raises(gh.GsplatError):
        r.release(7)                                    # not held any more
    r.release(1)
    r.dispose()


# ---- 4. overflow ----
def test_a_frame_that_was_not_composited_is_refused_and_its_slot_freed(gh, scenes):
    rows, data, pos = scenes(60000, 21)
    W, H = 640, 480
    cams = [gh.orbit_camera(k, width=W, height=H) for k in (3, 9)]
    ref = gh.HIPRenderer(W, H)
    ref.set_raw_scene(data, pos)
    ref.set_camera(cams[1])
    ref.render_async(); ref.sync()
    want = ref.readPixels()
    ref.dispose()
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    r.open_delivery(2)
    r.set_camera(cams[0])
    s, first = _deliver_one(r)
    r.set_list_capacity(2048)                           # far too small for the next frame
    r.set_camera(cams[1])
    r.render_async()
    k = r.deliver()
    with pytest.raises(gh.GsplatError, match="frame %d was not composited" % k) as ei:
        r.acquire(k)
    assert ei.value.code == gh.GSR_ERR_OVERFLOW
    with pytest.raises(gh.GsplatError):
        r.release(k)                                    # the refused frame holds no slot
    # the same pose again: gsr_render_async regrows the lists before it enqueues; both slots are free
    got = {}
    for _ in range(2):
        s, got[s] = _deliver_one(r)
    assert sorted(got) == [k + 1, k + 2]
    assert np.array_equal(got[k + 1], want) and np.array_equal(got[k + 2], want) and not np.array_equal(want, first)
    assert r.stats()["overflow_frames"] >= 1
    with pytest.raises(gh.GsplatError, match="not composited"):
        r.sync()                                        # the lost frame is reported once, as before
    r.sync()
    r.dispose()


# ---- 5. lifetime ----
def test_resize_and_close_wait_for_the_host_to_let_go(gh, scenes):
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    W, H = cfg["width"], cfg["height"]
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    f, nbytes = gh.GsrFrame(), ctypes.c_uint64(1)
    for rc in (r._L.gsr_deliver_frame_async(r._ctx, None), r._L.gsr_frame_ready(r._ctx, 0), r._L.gsr_acquire_frame(r._ctx, 0, ctypes.byref(f)),
               r._L.gsr_release_frame(r._ctx, 1), r._L.gsr_delivery_close(r._ctx)):
        assert rc == -1                                 # no ring
    assert r._L.gsr_delivery_slot_ptr(r._ctx, 0, ctypes.byref(nbytes)) is None and nbytes.value == 0
    with pytest.raises(gh.GsplatError):
        r.open_delivery(1)
    with pytest.raises(gh.GsplatError):
        r.open_delivery(9)
    r.open_delivery(2)
    with pytest.raises(gh.GsplatError):
        r.deliver()                                     # nothing rendered yet
    r.set_camera(_camera(gh, 5, cfg))
    r.render_async()
    s, px = r.acquire(r.deliver())
    snap = px.copy()
    for refused in (lambda: r.setSize(320, 240), r.close_delivery, lambda: r.open_delivery(3)):
        with pytest.raises(gh.GsplatError) as ei:
            refused()
        assert ei.value.code == -1
    assert (r.width, r.height) == (W, H) and np.array_equal(px, snap)
    r.setSize(W, H)                                     # the same size keeps the ring, and the held frame
    assert np.array_equal(px, snap)
    r.release(s)
    del px
    r.setSize(322, 241)                                 # an idle ring follows the framebuffer
    r.set_camera(gh.orbit_camera(5, width=322, height=241, fx=cfg["fx"] / 2))
    s2, got = _deliver_one(r)
    assert s2 == s + 1 and got.shape == (241, 322, 4) and np.array_equal(got, r.readPixels()) and got.any()
    r.render_async(); r.deliver()                       # a frame nobody picks up: close waits for its copy and drops it
    r.close_delivery()
    with pytest.raises(gh.GsplatError):
        r.acquire()
    r.open_delivery(2)
    assert _deliver_one(r)[0] == s2 + 2                 # serials never restart
    r.render_async(); r.deliver()
    r.render_async(); r.deliver()
    r.dispose()                                         # copies in flight


def test_contexts_with_rings_come_and_go_without_leaking(gh):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "leak_check.py")], capture_output=True, text=True)
    assert out.returncode == 0 and "ok: no growth" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- 6. group ----
def test_delivery_of_the_gathered_frame_single_rank_rccl(gh, scenes):
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    W, H = cfg["width"], cfg["height"]
    ref = gh.HIPRenderer(W, H)
    ref.set_raw_scene(data, pos)
    r = gh.HIPRenderer(W, H)
    r.set_raw_scene(data, pos)
    r.open_delivery(3)
    r.join_group(gh.new_group_id(), 0, 1, [(0, W)])
    with pytest.raises(gh.GsplatError):
        r.deliver()                                     # nothing gathered yet
    cams = [_camera(gh, k, cfg) for k in (5, 41, 77)]
    serials = []
    for cam in cams:                                    # back to back: the next de-slab must not overtake a copy
        r.set_camera(cam)
        r.render_async()
        r.allgather_frame_async()
        serials.append(r.deliver())
    last = r.read_frame()
    for k, cam in zip(serials, cams):
        s, px = r.acquire(k)
        ref.set_camera(cam)
        ref.render_async(); ref.sync()
        assert np.array_equal(px, ref.readPixels()), k
        if k == serials[-1]:
            assert np.array_equal(px, last)
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
    s, px = r.acquire(r.deliver())
    ref.set_camera(_camera(gh, 60, cfg))
    ref.render_async(); ref.sync()
    assert np.array_equal(px, ref.readPixels()) and np.array_equal(px, r.read_frame())
    r.release(s)
    r.leave_group()                                     # a plain context again: the ring delivers its own framebuffer
    r.set_camera(cams[0])
    s, got = _deliver_one(r)
    assert np.array_equal(got, r.readPixels())
    r.dispose(); ref.dispose()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _group_worker(rank, world, port, out):
    """world > 1 on one GPU the way tests/test_gpu_bands_gloo.py does it: the collective injected through
    gsr_comm_init_custom as a host-staged gloo all-gather, everything around it the product path."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "gsplat.js_amd", "py"))
    import torch
    import torch.distributed as dist
    import gsplat_hip as gh
    from gsplat_hip import bands
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = gh.synth.CONFIGS["C1"]
        W, H = cfg["width"], cfg["height"]
        scene = gh.Scene()
        scene.setData(gh.synth.config_rows("C1"))
        cams = [gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"]) for k in (3, 38, 71, 104)]
        cal = gh.HIPRenderer(W, H, device=0)
        cal.render(scene, cams[0])
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
        a.open_delivery(2)
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
            s, px = a.acquire(k)
            cal.render(scene, cam)
            ok = ok and np.array_equal(px, cal.readPixels())
            if k == serials[-1]:
                ok = ok and np.array_equal(px, last)
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
        s, px = a.acquire(a.deliver())
        cal.render(scene, cams[2])
        ok = ok and np.array_equal(px, cal.readPixels())
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


@pytest.mark.parametrize("world", [2, 3])
def test_delivery_of_the_gathered_frame_in_a_larger_world(tmp_path, world):
    import torch.multiprocessing as mp
    out = str(tmp_path / "result.txt")
    mp.spawn(_group_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    assert open(out).read() == "ok"


# ---- 7. the C++ host ----
def _fnv1a(b):
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_cpp_caller_delivers_what_the_python_host_delivers(gh, scenes, tmp_path):
    cfg = gh.synth.CONFIGS["C1"]
    rows, data, pos = scenes("C1")
    f = tmp_path / "c1.splat"
    f.write_bytes(np.asarray(rows, dtype=np.uint8).tobytes())
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    for in_flight in ("1", "3"):
        out = subprocess.run([exe, "--config", "C1", "--rows", str(f), "--frames", "30", "--warmup", "5", "--in-flight", in_flight, "--deliver"],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line["frames_per_sec_delivered"] > 0 and line["delivered_equals_read_pixels"] is True
        assert line["delivered_rgba8_fnv1a"] == line["rgba8_fnv1a"]
        if in_flight == "1":
            cpp = line["delivered_rgba8_fnv1a"]
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_raw_scene(data, pos)
    r.open_delivery(3)
    r.set_camera(_camera(gh, 0, cfg))
    s, got = _deliver_one(r)
    assert _fnv1a(got) == cpp
    r.dispose()


# ---- 8. the measurement beside bench.py ----
def test_bench_delivery_prints_one_line_with_checked_frames(gh):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_delivery.py"), "--config", "C1", "--frames", "24", "--warmup", "6",
                          "--other", "C2"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["value"] == line["delivered"]["frames_per_sec"] > 0 and line["bytes_per_frame"] == 640 * 480 * 4
    for leg in (line["delivered"], line["delivered_in_flight"], line["other_configs"]["C2"]["delivered"]):
        assert leg["frames_per_sec"] > 0 and leg["delivered_equals_read_pixels"] is True
    assert line["delivered_in_flight"]["contexts"] == 3
    for key in ("render_only", "with_rgba8_readback", "frame_latency_ms", "delivered_frame_latency_ms"):
        assert key in line
    assert line["delivered_frame_latency_ms"]["p50"] > 0

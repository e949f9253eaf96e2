"""Depth in a group (gsr_comm_set_depth): the ranks exchange depth slabs beside the colour slabs.  The bar everywhere is exact: the
gathered plane is, bit for bit, tests/depth_delivery_reference.py applied to the hit plane of a context that renders the whole
image, and a slab's depth section is tests/depth_exchange_reference.py's.  Worlds 2 and 3 run on one GPU the way
tests/test_gpu_delivery.py does it: spawned processes, a host-staged gloo all-gather through join_group_custom, a whole-image
calibration context per rank (at most 3 processes with the GPU open per case)."""
import ctypes
import os
import socket
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
GSR_ERR_ARG = -1
ODD = (617, 333)                       # a width that is no multiple of 32 (and odd), an odd height
COMBOS = (("u16", 2), ("f32", 1), ("u16", 1), ("f32", 2))
JOIN_TIMEOUT = 240                     # seconds a spawned world may take: a rank that fails must not leave the others in the collective


def _paths():
    for p in (ROOT, os.path.join(ROOT, "gsplat.js_amd", "py"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _want(hit, fmt, step, near):
    import depth_delivery_reference as D
    s = D.subsample(hit, step)
    return s if fmt == "f32" else D.quantise_u16(s, near)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _cams(gh, W, H, fx):
    """two orbit poses that fill the image, and a distant one looking past the scene: the splats lie in one side of the image only"""
    from gsplat_hip.camera import Camera, orbit_pose
    near_cams = [gh.orbit_camera(k, width=W, height=H, fx=fx) for k in (3, 38)]
    pos, rot = orbit_pose(0.4, 0.3, 60.0, target=(10.0, 0.0, 0.0))
    return near_cams + [Camera(pos, rot, fx, fx).update(W, H)]


NEARS = (8.0, 8.0, 64.0)               # per camera of _cams: inside the scene's depth range, so that some hits lie in front of it


def _calibrate(cal, scene, cam):
    """(colour, hit plane) of the whole image on a context of its own"""
    cal.render(scene, cam)
    return cal.readPixels().copy(), cal.read_depth()[1].copy()


class _World:
    """a rank's view of a spawned world: gloo, the host-staged collective, and what it was last handed"""

    def __init__(self, rank, world, port):
        _paths()
        import torch
        import torch.distributed as dist
        import gsplat_hip as gh
        from gsplat_hip import bands
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        self.torch, self.dist, self.gh, self.bands, self.rank, self.world = torch, dist, gh, bands, rank, world
        self.dev = torch.device("cuda:0")
        self.nbytes, self.slab = None, None
        self.bad = []

    def allgather(self, send, recv, nbytes, stream):
        torch, bands, world = self.torch, self.bands, self.world
        s = torch.cuda.ExternalStream(stream, device=self.dev)
        s.synchronize()
        mine = torch.as_tensor(bands.DevicePointer(send, (nbytes,), "|u1"), device=self.dev).cpu()
        self.nbytes, self.slab = nbytes, mine.numpy().copy()
        every = torch.empty(world * nbytes, dtype=torch.uint8)
        self.dist.all_gather_into_tensor(every, mine)
        with torch.cuda.stream(s):
            torch.as_tensor(bands.DevicePointer(recv, (world * nbytes,), "|u1"), device=self.dev).copy_(every)
        s.synchronize()

    def check(self, ok, what):
        if not ok:
            self.bad.append(str(what))

    def raises(self, fn, code, match, what):
        try:
            fn()
            self.bad.append("%s: not refused" % what)
        except self.gh.GsplatError as e:
            self.check(e.code == code and match in str(e), "%s: code %s, %s" % (what, e.code, e))

    def finish(self, out):
        res = self.torch.tensor([0 if self.bad else 1])
        self.dist.all_reduce(res, op=self.dist.ReduceOp.MIN)
        open("%s.%d" % (out, self.rank), "w").write("ok" if not self.bad else "\n".join(self.bad))
        self.dist.barrier()


def _scene(gh, name="C1", rows=None):
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows(name) if rows is None else rows)
    return scene


def _gather(a):
    a.render_async()
    a.allgather_frame_async()


# ---- the scenarios a spawned world runs ----
def _planes_and_slabs(w, lib=None):
    """2a / 2b: every rank's gathered plane against the calibration context; the bytes handed to the collective against the reference"""
    import depth_exchange_reference as X
    gh = w.gh
    fx = gh.synth.CONFIGS["C1"]["fx"]
    scene = _scene(gh)
    for (W, H) in ((640, 480), ODD) if lib is None else (ODD,):
        cams = _cams(gh, W, H, fx)
        edges = w.bands.band_edges(W, w.world)
        cal = gh.HIPRenderer(W, H, device=0)
        truth = [_calibrate(cal, scene, cam) for cam in cams]
        cal.dispose()
        # the premises of the cases: a band without any hit, and hits in front of near
        far_hit = truth[2][1]
        w.check(np.isfinite(far_hit).any() and any(not np.isfinite(far_hit[:, a:b]).any() for a, b in edges), "no band without a hit at %dx%d" % (W, H))
        for (colour, hit), near in zip(truth, NEARS):
            w.check((hit < near).any() and (hit[np.isfinite(hit)] > near).any(), "near %g does not cut the hits" % near)
        a = gh.HIPRenderer(W, H, device=0, lib_path=lib)
        a.join_group_custom(w.rank, w.world, edges, w.allgather)
        a.render(scene, cams[0])
        for fmt, step in COMBOS if lib is None else COMBOS[:2]:
            for cam, (colour, hit), near in zip(cams, truth, NEARS):
                a.set_group_depth(fmt, step, near)
                a.set_camera(cam)
                _gather(a)
                got = a.read_frame_depth()
                want = _want(hit, fmt, step, near)
                tag = (W, H, fmt, step, near)
                w.check(_same(got, want), ("plane", tag, int((np.asarray(got) != want).sum()) if got.shape == want.shape else got.shape))
                w.check(_same(a.read_frame(), colour), ("colour", tag))
                lay = X.layout(W, H, edges, step, fmt)
                fl = a.frame_depth_layout()
                w.check((fl["width"], fl["height"], fl["offset"], fl["bytes"], fl["stride"]) ==
                        (lay["Wd"], lay["Hd"], 0, want.nbytes, lay["Wd"] * lay["sample_bytes"]), ("layout", tag, fl))
                w.check(w.nbytes == lay["slab_bytes"], ("bytes_per_rank", tag, w.nbytes, lay["slab_bytes"]))
                sec = X.section(want, edges, w.rank, step, fmt)
                w.check(w.slab[lay["offset"]:].tobytes() == sec.tobytes(), ("section", tag))
        if lib is not None:
            for name in ("deliver", "depth", "blend"):
                buf = (ctypes.c_uint32 * 8)()
                w.check(getattr(a._L, "gsr_debug_bounds_" + name)(buf) == 0 and not any(buf), ("bounds", name, list(buf)))
        a.dispose()


def _ring(w):
    """4: two frames back to back through a ring of two; serial k carries colour k and depth k"""
    import yuv_reference as Y
    gh = w.gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H = cfg["width"], cfg["height"]
    scene = _scene(gh)
    cams = _cams(gh, W, H, cfg["fx"])[:2]
    cal = gh.HIPRenderer(W, H, device=0)
    truth = [_calibrate(cal, scene, cam) for cam in cams]
    cal.dispose()
    w.check(not _same(truth[0][1], truth[1][1]), "the two poses have one depth")
    edges = w.bands.band_edges(W, w.world)
    a = gh.HIPRenderer(W, H, device=0)
    a.join_group_custom(w.rank, w.world, edges, w.allgather)
    a.render(scene, cams[0])
    for colour_fmt, (fmt, step) in (("rgba8", ("u16", 2)), ("nv12", ("f32", 1)), ("rgba8", ("f32", 2))):
        a.set_group_depth(fmt, step, 8.0)
        a.open_delivery_depth(2, format=colour_fmt, depth=fmt, depth_step=step, depth_near=8.0)
        lay_before = (a.delivery_layout(), a.depth_layout())
        serials = []
        for cam in cams:
            a.set_camera(cam)
            _gather(a)
            serials.append(a.deliver())
        for k, (colour, hit) in zip(serials, truth):
            s, px, depth = a.acquire(k)
            w.check(s == k, ("serial", s, k))
            if colour_fmt == "rgba8":
                w.check(_same(px, colour), ("ring colour", colour_fmt, k))
            else:
                w.check(np.concatenate([p.ravel() for p in px]).tobytes() == Y.payload(colour, "nv12").tobytes(), ("ring colour", colour_fmt, k))
            w.check(_same(depth, _want(hit, fmt, step, 8.0)), ("ring depth", colour_fmt, fmt, step, k))
            a.release(s)
        w.check(lay_before == (a.delivery_layout(), a.depth_layout()), "the layouts moved")
        a.close_delivery()
    a.dispose()


def _share(w):
    """5: two contexts of one rank, frames in flight, each with the option"""
    gh = w.gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H = cfg["width"], cfg["height"]
    scene = _scene(gh)
    cams = _cams(gh, W, H, cfg["fx"])
    cal = gh.HIPRenderer(W, H, device=0)
    truth = [_calibrate(cal, scene, cam) for cam in cams]
    cal.dispose()
    edges = w.bands.band_edges(W, w.world)
    a = gh.HIPRenderer(W, H, device=0)
    a.join_group_custom(w.rank, w.world, edges, w.allgather)
    b = gh.HIPRenderer(W, H, device=0)
    a.render(scene, cams[0])
    b.render(scene, cams[0])
    b.share_group(a)
    for r in (a, b):
        r.set_group_depth("u16", 2, 8.0)
        r.open_delivery_depth(2, depth="u16", depth_step=2, depth_near=8.0)
    order = [(a, 0), (b, 1), (a, 2), (b, 0)]             # the same order of collectives on every rank
    serials = []
    for r, i in order:
        r.set_camera(cams[i])
        _gather(r)
        serials.append(r.deliver())
    # what each context gathered last
    for r, i in order[2:]:
        w.check(_same(r.read_frame_depth(), _want(truth[i][1], "u16", 2, 8.0)) and _same(r.read_frame(), truth[i][0]), ("shared, last", i))
    for (r, i), k in zip(order, serials):
        s, px, depth = r.acquire(k)
        w.check(_same(px, truth[i][0]) and _same(depth, _want(truth[i][1], "u16", 2, 8.0)), ("shared, ring", i, k))
        r.release(s)
    b.dispose(); a.dispose()


def _overflow(w):
    """6: one rank's lists overflow: every rank refuses that gathered frame's depth, and the repeated frame is exact"""
    gh = w.gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H = cfg["width"], cfg["height"]
    scene = _scene(gh)
    cams = _cams(gh, W, H, cfg["fx"])
    cal = gh.HIPRenderer(W, H, device=0)
    colour, hit = _calibrate(cal, scene, cams[1])
    cal.dispose()
    a = gh.HIPRenderer(W, H, device=0)
    a.join_group_custom(w.rank, w.world, w.bands.band_edges(W, w.world), w.allgather)
    a.render(scene, cams[0])
    a.set_group_depth("f32", 1)
    a.open_delivery_depth(2, depth="f32", depth_step=1)
    _gather(a)
    a.sync()
    if w.rank == w.world - 1:
        a.set_list_capacity(1024)
    a.set_camera(cams[1])
    _gather(a)
    k = a.deliver()
    w.raises(lambda: a.acquire(k), gh.GSR_ERR_OVERFLOW, "not composited", "acquire of the stale frame")
    w.raises(a.read_frame_depth, gh.GSR_ERR_OVERFLOW, "not composited", "read_frame_depth of the stale frame")
    _gather(a)                                           # the lists have been regrown: the group repeats the frame
    s, px, depth = a.acquire(a.deliver())
    w.check(_same(px, colour) and _same(depth, _want(hit, "f32", 1, 0.0)), "the repeated frame through the ring")
    a.release(s)
    w.check(_same(a.read_frame_depth(), _want(hit, "f32", 1, 0.0)), "the repeated frame")
    try:
        a.sync()
    except gh.GsplatError:
        pass                                             # (the overflowing rank reports its lost frame once)
    a.dispose()


def _optin(w):
    """7 / 8: without the option nothing changes; refusals leave the context usable and take no slot"""
    import depth_exchange_reference as X
    gh = w.gh
    cfg = gh.synth.CONFIGS["C1"]
    W, H = cfg["width"], cfg["height"]
    scene = _scene(gh)
    cams = _cams(gh, W, H, cfg["fx"])
    cal = gh.HIPRenderer(W, H, device=0)
    colour, hit = _calibrate(cal, scene, cams[0])
    cal.dispose()
    edges = w.bands.band_edges(W, w.world)
    colour_bytes = X.colour_bytes(X.slab_width(edges), H)
    a = gh.HIPRenderer(W, H, device=0)
    w.raises(lambda: a.set_group_depth("u16", 2), GSR_ERR_ARG, "not in a group", "set_group_depth outside a group")
    a.join_group_custom(w.rank, w.world, edges, w.allgather)
    a.render(scene, cams[0])
    # option off: today's slab, today's refusals
    _gather(a)
    w.check(w.nbytes == colour_bytes == (X.slab_width(edges) * H + 4) * 4 and _same(a.read_frame(), colour), ("bytes_per_rank without the option", w.nbytes))
    w.raises(lambda: a.open_delivery_depth(2, depth="u16"), GSR_ERR_ARG, "depth is not exchanged between ranks", "a depth ring without the option")
    w.raises(a.read_frame_depth, GSR_ERR_ARG, "exchanges no depth", "read_frame_depth without the option")
    w.raises(a.frame_depth_layout, GSR_ERR_ARG, "exchanges no depth", "frame_depth_layout without the option")
    b = gh.HIPRenderer(W, H, device=0)
    b.open_delivery_depth(2, depth="u16", depth_step=2, depth_near=8.0)      # opened BEFORE the context joins
    b.join_group_custom(w.rank, w.world, edges, w.allgather)
    b.render(scene, cams[0])
    _gather(b)
    w.raises(b.deliver, GSR_ERR_ARG, "joined a group after it opened a depth ring", "a ring from before the group, option off")
    b.set_group_depth("u16", 2, 8.0)                     # ... and works once the option matches at the time of the delivery
    w.raises(b.deliver, GSR_ERR_ARG, "no gathered frame yet", "a delivery before anything was gathered under the option")
    _gather(b)
    s, px, depth = b.acquire(b.deliver())
    w.check(s == 1 and _same(px, colour) and _same(depth, _want(hit, "u16", 2, 8.0)), "a ring from before the group, option on")
    b.release(s)
    b.dispose()
    # bad options: refused as gsr_delivery_open_depth refuses them, the option stays what it was
    a.set_group_depth("u16", 2, 0.5)
    for args in ((3, 1, 0.1, 0), (-1, 1, 0.1, 0), (1, 3, 0.1, 0), (2, 0, 0.1, 0), (2, 1, 0.0, 0), (2, 2, -1.0, 0), (2, 1, float("nan"), 0),
                 (2, 1, float("inf"), 0), (1, 1, 0.1, 7)):
        d = gh.GsrDepthDeliveryOptions(*args)
        w.check(a._L.gsr_comm_set_depth(a._ctx, ctypes.byref(d)) == GSR_ERR_ARG, ("bad options accepted", args))
    w.check(a.frame_depth_layout()["format"] == "u16" and a.frame_depth_layout()["step"] == 2, "a refusal changed the option")
    # a ring whose depth options differ from the exchange's
    w.raises(lambda: a.open_delivery_depth(2, depth="f32", depth_step=2), GSR_ERR_ARG, "depth format", "ring format mismatch")
    w.raises(lambda: a.open_delivery_depth(2, depth="u16", depth_step=1, depth_near=0.5), GSR_ERR_ARG, "depth step", "ring step mismatch")
    w.raises(lambda: a.open_delivery_depth(2, depth="u16", depth_step=2, depth_near=0.25), GSR_ERR_ARG, "depth near", "ring near mismatch")
    a.open_delivery_depth(2, depth="u16", depth_step=2, depth_near=0.5)
    # behind a sort-only frame the lists are not this frame's: nothing is enqueued, and the collective is not called
    _gather(a)
    calls = w.nbytes
    w.nbytes = None
    a.sort()
    w.raises(a.allgather_frame_async, GSR_ERR_ARG, "sort-only", "allgather behind a sort-only frame")
    w.check(w.nbytes is None, "the collective ran behind a sort-only frame")
    _gather(a)
    w.check(w.nbytes == calls == X.layout(W, H, edges, 2, "u16")["slab_bytes"], ("bytes_per_rank with the option", w.nbytes))
    s, px, depth = a.acquire(a.deliver())
    w.check(s == 1 and _same(px, colour) and _same(depth, _want(hit, "u16", 2, 0.5)), "the first serial after the refusals")
    a.release(s)
    a.close_delivery()
    # off again: today's slab
    a.set_group_depth(None)
    _gather(a)
    w.check(w.nbytes == colour_bytes and _same(a.read_frame(), colour), "bytes_per_rank after switching the option off")
    a.set_group_depth("f32", 1)
    a.leave_group()                                      # the option goes with the group
    w.raises(a.frame_depth_layout, GSR_ERR_ARG, "exchanges no depth", "the option survived leave_group")
    w.raises(lambda: a.set_group_depth("f32", 1), GSR_ERR_ARG, "not in a group", "set_group_depth after leave_group")
    a.set_band(0, 0)
    a.open_delivery_depth(2, depth="f32", depth_step=1)  # a plain context again: a depth ring of its own
    a.render_async()
    s, px, depth = a.acquire(a.deliver())
    w.check(_same(px, colour) and _same(depth, hit), "a single-context depth ring after leave_group")
    a.release(s)
    a.join_group_custom(w.rank, w.world, edges, w.allgather)              # joining anew starts without the option
    w.raises(a.frame_depth_layout, GSR_ERR_ARG, "exchanges no depth", "the option survived a new join")
    a.dispose()


def _walk(w):
    """9: a seeded walk over option, size, scene and membership; every gathered frame equals a fresh whole-image context's"""
    gh = w.gh
    rng = np.random.default_rng(20240611)                # the same walk on every rank
    fx = gh.synth.CONFIGS["C1"]["fx"]
    sizes = [(640, 480), ODD, (352, 200)]
    rows = [gh.synth.config_rows("C1"), gh.synth.synth_rows(4000, 77, 1.2, 0.01, 0.08)]
    W, H = sizes[0]
    scene = _scene(gh, rows=rows[0])
    a = gh.HIPRenderer(W, H, device=0)
    state = {"opt": None, "scene": 0, "joined": False}

    def join():
        a.join_group_custom(w.rank, w.world, w.bands.band_edges(a.width, w.world), w.allgather)
        state["joined"], state["opt"] = True, None

    join()
    a.render(scene, gh.orbit_camera(0, width=W, height=H, fx=fx))
    ops = ["on", "other", "off", "resize", "scene", "rejoin"]
    for step_no in range(14):
        op = ops[step_no] if step_no < len(ops) else ops[int(rng.integers(len(ops)))]
        if op in ("on", "other"):
            opt = (("u16", "f32")[int(rng.integers(2))], int(rng.integers(1, 3)), float(rng.choice([0.5, 4.0, 8.0])))
            if op == "on" and state["opt"] is None:
                opt = ("u16", 2, 8.0)
            a.set_group_depth(*opt)
            state["opt"] = opt
        elif op == "off":
            a.set_group_depth(None)
            state["opt"] = None
        elif op == "resize":
            a.leave_group()                              # slabs and band edges belong to the old size
            W, H = sizes[(sizes.index((W, H)) + 1) % len(sizes)]
            a.setSize(W, H)
            join()
        elif op == "scene":
            state["scene"] ^= 1
            scene = _scene(gh, rows=rows[state["scene"]])
        elif op == "rejoin":
            a.leave_group()
            join()
        cam = gh.orbit_camera(int(rng.integers(120)), width=W, height=H, fx=fx)
        fresh = gh.HIPRenderer(W, H, device=0)
        colour, hit = _calibrate(fresh, scene, cam)
        fresh.dispose()
        a.render(scene, cam)                             # (uploads the scene when it changed)
        opt = state["opt"]
        if opt:
            a.open_delivery_depth(2, depth=opt[0], depth_step=opt[1], depth_near=opt[2])
        else:
            a.open_delivery(2)
        _gather(a)
        k = a.deliver()
        tag = (step_no, op, W, H, opt)
        if opt:
            s, px, depth = a.acquire(k)
            want = _want(hit, *opt)
            w.check(_same(depth, want) and _same(a.read_frame_depth(), want), ("walk depth", tag))
        else:
            s, px = a.acquire(k)
            w.check(w.nbytes == (max(32, max(b - c for c, b in w.bands.band_edges(W, w.world))) * H + 4) * 4, ("walk bytes", tag, w.nbytes))
        w.check(_same(px, colour) and _same(a.read_frame(), colour), ("walk colour", tag))
        a.release(s)
        a.close_delivery()
    a.dispose()


def _bounds(w):
    """10: one size's frames on the bounds-checked build: no index of the new kernels leaves its array"""
    w.check(os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing")
    _planes_and_slabs(w, lib=BOUNDS_LIB)


SCENARIOS = {"planes_and_slabs": _planes_and_slabs, "ring": _ring, "share": _share, "overflow": _overflow, "optin": _optin, "walk": _walk,
             "bounds": _bounds}


def _worker(rank, world, port, out, scenario):
    w = _World(rank, world, port)
    try:
        try:
            SCENARIOS[scenario](w)
        except Exception:
            import traceback
            w.bad.append(traceback.format_exc())
            open("%s.%d" % (out, rank), "w").write("\n".join(w.bad))
            raise                                        # (the parent ends the other ranks)
        w.finish(out)
    finally:
        w.dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_world(tmp_path, world, scenario):
    import torch.multiprocessing as mp
    out = str(tmp_path / "result")
    ctx = mp.spawn(_worker, args=(world, _free_port(), out, scenario), nprocs=world, join=False)
    deadline = time.time() + JOIN_TIMEOUT
    failure = None
    try:
        while not ctx.join(timeout=5):
            if time.time() > deadline:
                failure = "the world did not finish in %d s" % JOIN_TIMEOUT
                break
    except Exception as e:                               # a rank raised: mp.spawn has ended the others
        failure = str(e)
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join(10)
    results = [open("%s.%d" % (out, r)).read() if os.path.exists("%s.%d" % (out, r)) else "no result" for r in range(world)]
    assert failure is None and results == ["ok"] * world, (failure, results)


# ---- 1. world 1 ----
@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


@pytest.mark.parametrize("fmt,step", COMBOS)
def test_world_of_one_equals_a_depth_ring(gh, fmt, step):
    import torch
    from gsplat_hip import bands
    _paths()
    import depth_exchange_reference as X
    cfg = gh.synth.CONFIGS["C1"]
    W, H = ODD if step == 2 else (cfg["width"], cfg["height"])
    scene = _scene(gh)
    dev = torch.device("cuda:0")
    seen = []

    def allgather(send, recv, nbytes, stream):           # a world of one: the slab is the gathered buffer
        s = torch.cuda.ExternalStream(stream, device=dev)
        with torch.cuda.stream(s):
            torch.as_tensor(bands.DevicePointer(recv, (nbytes,), "|u1"), device=dev).copy_(torch.as_tensor(bands.DevicePointer(send, (nbytes,), "|u1"), device=dev))
        seen.append(nbytes)

    ring = gh.HIPRenderer(W, H, device=0)
    ring.open_delivery_depth(2, depth=fmt, depth_step=step, depth_near=8.0)
    a = gh.HIPRenderer(W, H, device=0)
    a.join_group_custom(0, 1, [(0, W)], allgather)
    a.set_group_depth(fmt, step, 8.0)
    a.open_delivery_depth(2, depth=fmt, depth_step=step, depth_near=8.0)
    assert a.depth_layout() == ring.depth_layout()
    for n, cam in enumerate(_cams(gh, W, H, cfg["fx"])):
        ring.render(scene, cam)
        ring.render_async()
        s, px, depth = ring.acquire(ring.deliver())
        want_px, want = px.copy(), depth.copy()
        ring.release(s)
        assert _same(want, _want(ring.read_depth()[1], fmt, step, 8.0))
        a.render(scene, cam)
        _gather(a)
        got = a.read_frame_depth()
        assert _same(got, want), (n, int((got != want).sum()))
        s, px, depth = a.acquire(a.deliver())
        assert _same(px, want_px) and _same(depth, want), n
        a.release(s)
        assert seen[-1] == X.layout(W, H, [(0, W)], step, fmt)["slab_bytes"]
        # the exchange's pass has planes of its own: read_depth answers as it does without a group
        assert _same(a.read_depth()[1], ring.read_depth()[1])
    a.dispose(); ring.dispose()


# ---- 2 .. 8: worlds 2 and 3 ----
@pytest.mark.parametrize("scenario", ["planes_and_slabs", "ring", "share", "overflow", "optin"])
@pytest.mark.parametrize("world", [2, 3])
def test_larger_worlds(tmp_path, world, scenario):
    _run_world(tmp_path, world, scenario)


# ---- 9. frame-to-frame state ----
def test_a_veteran_group_context_gathers_every_plane_as_a_fresh_one(tmp_path):
    _run_world(tmp_path, 2, "walk")


# ---- 10. the bounds-checked build ----
def test_no_index_of_the_exchange_leaves_its_array(tmp_path):
    _run_world(tmp_path, 2, "bounds")

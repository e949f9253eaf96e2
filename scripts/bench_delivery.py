#!/usr/bin/env python3
"""Frames per second when every frame reaches the host as RGBA8 -- the measurement beside bench.py, whose line leaves the
framebuffer on the device.  The workload is bench.py's: a BASELINE.json configuration, the 120-pose orbit, the scene built on
the device from the seeded .splat rows.  Prints one JSON line:

  render_only                  render_async only, one default context (what bench.py's one_frame_in_flight leg times)
  with_rgba8_readback          gsr_read_pixels_rgba8 behind every frame (conversion + copy into pageable memory + stream wait)
  delivered                    every frame through the library's delivery ring (gsr_deliver_frame_async / gsr_acquire_frame,
                               `--slots` pinned slots, the oldest frame picked up when the ring is full); frame k's copy runs
                               under frame k+1's kernels
  delivered_frame_latency_ms   render_async + deliver + acquire of one frame on an idle GPU, next to frame_latency_ms
                               (render_async + sync)
  delivered_in_flight          F throughput contexts used round-robin, each with its own ring
  other_configs                `delivered` and `render_only` for the other configurations (--other C2,C4)
Every delivered leg compares its last delivered frame with readPixels() of the same pose, byte for byte
(`delivered_equals_read_pixels`).  --format nv12|i420 opens the rings in 4:2:0 Y'CbCr (BT.709 limited range, black background):
the same legs and keys, `bytes_per_frame` of the format, and the comparison goes through the definition in plain numpy
(tests/yuv_reference.py applied to readPixels() of the same pose: `delivered_equals_reference`).
--depth f32|u16 [--depth-step 1|2] [--depth-near X] opens depth rings (gsr_delivery_open_depth): the same legs and keys with a
depth plane beside every frame, `depth_bytes_per_frame`, and the last delivered plane compared with the definition
(tests/depth_delivery_reference.py applied to read_depth() of the same pose: `delivered_depth_equals_reference`).
--timed-only runs nothing but the warm-up and the timed `delivered` loop of the chosen configuration (with
--frames-in-flight F > 1: the F-context loop): the run a profiler wraps.

  python scripts/bench_delivery.py [--config C3] [--frames 480] [--warmup 30] [--slots 3] [--frames-in-flight 3]
                                   [--other C2,C4] [--timed-only] [--format rgba8|nv12|i420]
                                   [--depth f32|u16] [--depth-step 1|2] [--depth-near 0.1]
There is no CPU path: without an MI355X the script fails."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsplat.js_amd", "py"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

ORBIT_FRAMES = 120
SETUP_FRAMES = 4      # per context: the sort-order decision and the graph captures are not a frame's work


def percentiles(lat):
    lat = sorted(lat)
    return {"p50": lat[len(lat) // 2], "p99": lat[min(len(lat) - 1, int(len(lat) * 0.99))], "mean": sum(lat) / len(lat), "frames": len(lat)}


FORMAT = "rgba8"      # --format: what every ring of this run is opened for


def same_key():
    if DEPTH:
        return "delivered_depth_equals_reference"    # (colour and depth both)
    return "delivered_equals_read_pixels" if FORMAT == "rgba8" else "delivered_equals_reference"


DEPTH = None          # --depth: None, or the depth plane every ring of this run carries ("f32" / "u16")
DEPTH_STEP = 1
DEPTH_NEAR = 0.1


def open_ring(r, slots):
    if DEPTH:
        r.open_delivery_depth(slots, format=FORMAT, depth=DEPTH, depth_step=DEPTH_STEP, depth_near=DEPTH_NEAR)
    else:
        r.open_delivery(slots) if FORMAT == "rgba8" else r.open_delivery(slots, format=FORMAT)


def delivered_run(ctxs, poses, fx, count, slots):
    """`count` orbit frames, every one delivered: the contexts round-robin, a context's oldest frame acquired and released only
    when its ring is full.  Returns (frames/s, the last delivered frame equals readPixels() of the same pose -- for a Y'CbCr
    ring: the numpy reference's payload of it; on a depth ring: and its depth plane equals the reference's of read_depth())."""
    pending = [[] for _ in ctxs]
    last = None

    def pick_up(c):
        nonlocal last
        s, px, *depth = ctxs[c].acquire(pending[c].pop(0))
        last = (c, px, depth[0] if depth else None)
        ctxs[c].release(s)

    t0 = time.perf_counter()
    for k in range(count):
        c = k % len(ctxs)
        if len(pending[c]) == slots:
            pick_up(c)
        ctxs[c].set_camera_arrays(*poses[k % ORBIT_FRAMES], fx, fx)
        ctxs[c].render_async()
        pending[c].append(ctxs[c].deliver())
    for j in range(count - min(count, len(ctxs)), count):   # drain in frame order: the last frame is picked up last
        while pending[j % len(ctxs)]:
            pick_up(j % len(ctxs))
    fps = count / (time.perf_counter() - t0)
    c, px, depth = last
    # (its slot is released, but nothing has been delivered since)
    got = px.copy() if FORMAT == "rgba8" else np.concatenate([plane.ravel() for plane in px])
    got_depth = depth.copy() if DEPTH else None
    ctxs[c].set_camera_arrays(*poses[(count - 1) % ORBIT_FRAMES], fx, fx)
    ctxs[c].render_async()
    want = ctxs[c].readPixels()
    if FORMAT != "rgba8":
        import yuv_reference
        want = yuv_reference.payload(want, FORMAT)
    same = bool(np.array_equal(got, want))
    if DEPTH:
        import depth_delivery_reference as ddr
        want_depth = ddr.subsample(ctxs[c].read_depth()[1], DEPTH_STEP)
        if DEPTH == "u16":
            want_depth = ddr.quantise_u16(want_depth, DEPTH_NEAR)
        same = same and got_depth.dtype == want_depth.dtype and bool(np.array_equal(got_depth.view(np.uint8), want_depth.view(np.uint8)))
    return fps, same


def make_contexts(gh, cfg, rows, poses, count, throughput, device):
    rs = [gh.HIPRenderer(cfg["width"], cfg["height"], device=device, throughput=throughput) for _ in range(count)]
    for rr in rs:
        rr.set_scene_rows(rows)
        for j in range(SETUP_FRAMES):
            rr.set_camera_arrays(*poses[j], cfg["fx"], cfg["fx"])
            rr.render_async()
        rr.sync()
    return rs


def measure(gh, name, args, full):
    cfg = gh.synth.CONFIGS[name]
    W, H, fx = cfg["width"], cfg["height"], cfg["fx"]
    rows = gh.synth.config_rows(name)
    poses = [gh.orbit_camera(k, ORBIT_FRAMES, W, H, fx).f32() for k in range(ORBIT_FRAMES)]
    F = max(1, args.frames_in_flight)
    frames = args.frames if W * H <= 1920 * 1080 else max(60, args.frames // 4)
    out = {"workload": "%s: %d synthetic gaussians (seed %d), %dx%d, 120-pose orbit" % (name, cfg["n"], cfg["seed"], W, H),
           "frames": frames, "warmup": args.warmup, "slots": args.slots,
           "bytes_per_frame": W * H * 4 if FORMAT == "rgba8" else W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)}
    if FORMAT != "rgba8":
        out["format"] = FORMAT
    if DEPTH:
        Wd, Hd = (W + DEPTH_STEP - 1) // DEPTH_STEP, (H + DEPTH_STEP - 1) // DEPTH_STEP
        out.update({"depth": DEPTH, "depth_step": DEPTH_STEP, "depth_near": DEPTH_NEAR, "depth_bytes_per_frame": Wd * Hd * (4 if DEPTH == "f32" else 2)})
    if args.timed_only:
        rs = make_contexts(gh, cfg, rows, poses, F, F > 1, args.device)
        for rr in rs:
            open_ring(rr, args.slots)
        delivered_run(rs, poses, fx, args.warmup, args.slots)
        fps, same = delivered_run(rs, poses, fx, frames, args.slots)
        out["delivered_in_flight" if F > 1 else "delivered"] = {"frames_per_sec": fps, "contexts": F, same_key(): same}
        for rr in rs:
            rr.dispose()
        return out
    (r,) = make_contexts(gh, cfg, rows, poses, 1, False, args.device)

    def render_only(count):
        t0 = time.perf_counter()
        for k in range(count):
            r.set_camera_arrays(*poses[k % ORBIT_FRAMES], fx, fx)
            r.render_async()
        r.sync()
        return count / (time.perf_counter() - t0)

    render_only(args.warmup)
    out["render_only"] = {"frames_per_sec": render_only(frames)}
    open_ring(r, args.slots)
    delivered_run([r], poses, fx, args.warmup, args.slots)
    fps, same = delivered_run([r], poses, fx, frames, args.slots)
    out["delivered"] = {"frames_per_sec": fps, "contexts": 1, same_key(): same}
    if full:
        nread = min(frames, 120)
        buf = np.empty((H, W, 4), dtype=np.uint8)
        t0 = time.perf_counter()
        for k in range(nread):
            r.set_camera_arrays(*poses[k % ORBIT_FRAMES], fx, fx)
            r.render_async()
            r.readPixels(buf)
        out["with_rgba8_readback"] = {"frames_per_sec": nread / (time.perf_counter() - t0), "frames": nread}
        lat, lat_d = [], []
        for k in range(ORBIT_FRAMES):
            t0 = time.perf_counter()
            r.set_camera_arrays(*poses[k], fx, fx)
            r.render_async()
            r.sync()
            lat.append((time.perf_counter() - t0) * 1e3)
        for k in range(ORBIT_FRAMES):
            t0 = time.perf_counter()
            r.set_camera_arrays(*poses[k], fx, fx)
            r.render_async()
            s = r.acquire(r.deliver())[0]
            lat_d.append((time.perf_counter() - t0) * 1e3)
            r.release(s)
        out["frame_latency_ms"] = percentiles(lat)
        out["delivered_frame_latency_ms"] = percentiles(lat_d)
    r.dispose()
    if full and F > 1:
        rs = make_contexts(gh, cfg, rows, poses, F, True, args.device)
        for rr in rs:
            open_ring(rr, args.slots)
        delivered_run(rs, poses, fx, args.warmup, args.slots)
        fps, same = delivered_run(rs, poses, fx, frames, args.slots)
        out["delivered_in_flight"] = {"frames_per_sec": fps, "contexts": F, same_key(): same}
        for rr in rs:
            rr.dispose()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--slots", type=int, default=3)
    ap.add_argument("--frames-in-flight", type=int, default=3)
    ap.add_argument("--other", default="C2,C4", help="configurations measured beside --config (delivered and render_only); '' for none")
    ap.add_argument("--timed-only", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--format", default="rgba8", choices=["rgba8", "nv12", "i420"], help="what the rings deliver (default: RGBA8)")
    ap.add_argument("--depth", default=None, choices=["f32", "u16"], help="a depth plane beside every delivered frame (default: none)")
    ap.add_argument("--depth-step", type=int, default=1, choices=[1, 2], help="the depth plane holds every n-th pixel in both directions")
    ap.add_argument("--depth-near", type=float, default=0.1, help="--depth u16: the depth that maps to 65535")
    args = ap.parse_args()
    global FORMAT, DEPTH, DEPTH_STEP, DEPTH_NEAR
    FORMAT, DEPTH, DEPTH_STEP, DEPTH_NEAR = args.format, args.depth, args.depth_step, args.depth_near
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_delivery.py needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")
    import gsplat_hip as gh
    out = {"metric": "frames_per_sec_delivered", "unit": "frames/s", "build_id": gh.build_id()}
    out.update(measure(gh, args.config, args, True))
    out["value"] = (out.get("delivered") or out["delivered_in_flight"])["frames_per_sec"]
    if not args.timed_only and args.other:
        out["other_configs"] = {name: measure(gh, name, args, False) for name in args.other.split(",") if name != args.config}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

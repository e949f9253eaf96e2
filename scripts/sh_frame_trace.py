#!/usr/bin/env python3
"""The projection's cost with an SH frame: C3_sh (bench.py's sh_config: C3 with degree-3 SH on every splat) rendered over the
orbit with an identity frame (`--frame identity`: the path every context takes that never opted in) or after a followed
rotate (`--frame rotated`).  The figure is k_project_key's average in a
`rocprofv3 --kernel-trace --stats -- python scripts/sh_frame_trace.py --frame ...` run; the script prints frames/s only."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat.js_amd", "py"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", choices=("identity", "rotated"), default="identity")
    ap.add_argument("--frames", type=int, default=240)
    args = ap.parse_args()
    import numpy as np
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C3"]
    W, H, N = cfg["width"], cfg["height"], cfg["n"]
    rng = np.random.default_rng(33)
    tex = []
    for _ in range(3):
        w = rng.integers(0, 1 << 32, size=8 * N, dtype=np.uint64).astype(np.uint32)
        ex = rng.integers(9, 13, size=8 * N, dtype=np.uint32)
        ex2 = rng.integers(9, 13, size=8 * N, dtype=np.uint32)
        tex.append((w & np.uint32(0x83FF83FF)) | (ex << np.uint32(10)) | (ex2 << np.uint32(26)))
    r = gh.HIPRenderer(W, H)
    r.set_scene_rows(gh.synth.config_rows("C3"))
    r.set_sh(tex, np.array([-1, -1, -1], dtype=np.int32))
    r.set_sh_follow(True)
    if args.frame == "rotated":      # a tenth of a degree about y: the same splats are drawn, the frame is not the identity
        r.scene_rotate((0.0, 0.0008726645152351496, 0.0, 0.9999996192282494))
    poses = [gh.orbit_camera(k, 120, W, H, cfg["fx"]).f32() for k in range(120)]
    for k in range(8):
        r.set_camera_arrays(*poses[k], cfg["fx"], cfg["fx"])
        r.render_async()
    r.sync()
    t0 = time.perf_counter()
    for k in range(args.frames):
        r.set_camera_arrays(*poses[k % 120], cfg["fx"], cfg["fx"])
        r.render_async()
    r.sync()
    dt = time.perf_counter() - t0
    print(json.dumps({"config": "C3_sh", "frame": args.frame, "frames": args.frames, "frames_per_s": round(args.frames / dt, 1),
                      "sh_frame": r.sh_frame()[0].reshape(-1).tolist()}))
    r.dispose()


if __name__ == "__main__":
    main()

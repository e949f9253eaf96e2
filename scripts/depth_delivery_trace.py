#!/usr/bin/env python3
"""The depth ring's kernels under `rocprofv3 --kernel-trace --stats` (kernel trace only): per configuration, a throughput context
delivers `--frames` orbit frames through a ring with an f32 plane at step 1, then as many through a ring with a u16 plane at step 2.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/depth_delivery_trace.py [--configs C3,C4] [--frames 20]
  python scripts/depth_delivery_trace.py --summarise DIR     # medians per kernel and grid from DIR's *_kernel_trace.csv

A configuration's dispatches are told apart by their grid (one workgroup per bin: 2040 on C3, 8160 on C4).  No CPU path."""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsplat.js_amd", "py")]

KERNELS = re.compile(r"k_depth_planes|k_deliver_depth|k_deliver_yuv|k_deliver_rgba8|k_blend")


def run(configs, frames):
    import gsplat_hip as gh
    for name in configs:
        cfg = gh.synth.CONFIGS[name]
        W, H, fx = cfg["width"], cfg["height"], cfg["fx"]
        r = gh.HIPRenderer(W, H, throughput=True)
        r.set_scene_rows(gh.synth.config_rows(name))
        poses = [gh.orbit_camera(k * 120 // frames, 120, W, H, fx).f32() for k in range(frames)]
        for fmt, step in (("f32", 1), ("u16", 2)):
            r.open_delivery_depth(3, format="nv12", depth=fmt, depth_step=step)
            pending = []
            for pose in poses:
                if len(pending) == 3:
                    r.release(r.acquire(pending.pop(0))[0])
                r.set_camera_arrays(*pose, fx, fx)
                r.render_async()
                pending.append(r.deliver())
            for k in pending:
                r.release(r.acquire(k)[0])
            r.close_delivery()
        r.dispose()
        print(json.dumps({"config": name, "frames_per_ring": frames, "build_id": gh.build_id()}))


def summarise(directory):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True):
        for d in csv.DictReader(open(path)):
            name = d["Kernel_Name"]
            if not KERNELS.search(name):
                continue
            short = re.sub(r"\(.*", "", name).replace("void gsr::", "").replace("gsr::", "")
            wg = int(d["Workgroup_Size_X"]) or 1
            key = (short, int(d["Grid_Size_X"]) // wg)
            rows.setdefault(key, []).append((int(d["End_Timestamp"]) - int(d["Start_Timestamp"])) / 1e3)
    print("%-64s %10s %6s %10s %10s %10s" % ("kernel", "workgroups", "calls", "median us", "min us", "max us"))
    for (short, groups), t in sorted(rows.items()):
        t.sort()
        print("%-64s %10d %6d %10.1f %10.1f %10.1f" % (short, groups, len(t), t[len(t) // 2], t[0], t[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C4")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--summarise", metavar="DIR")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import torch
    if not torch.cuda.is_available():
        sys.exit("depth_delivery_trace.py needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")
    run(args.configs.split(","), args.frames)


if __name__ == "__main__":
    main()

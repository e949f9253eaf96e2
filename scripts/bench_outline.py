#!/usr/bin/env python3
"""What the selection outline costs: the overlay pass of one frame of a BASELINE.json configuration with
the outline off and with every (width, side) of --widths, for a lasso-like selection (the splats whose centres fall into the
middle of the frame), and an overlay ring delivering with and without it.

  python scripts/bench_outline.py [--config C3] [--samples 20] [--widths 1,2,16] [--frames 240]
      one JSON line: per case the host's clock around one enqueue of the pass and the wait for it on a drained stream (smallest
      and median of --samples; a launch's latency is inside, as in bench_cabi's overlay_pass_us), the pixels the outline wrote,
      and frames/s of an RGBA8 overlay ring (three slots, the 120-pose orbit) per case of --ring-cases
  python scripts/bench_outline.py --passes-only ...
      nothing but 3 + --samples passes per case, in order: the run a kernel trace wraps
  python scripts/bench_outline.py --passes-only --off-only
      the same for the pass without an outline alone, calling nothing a build from before the outline lacks
  python scripts/bench_outline.py --summarise DIR [--samples 20] [--widths 1,2,16 | --off-only]
      the kernels' own times from DIR's *_kernel_trace.csv of such a run: the dispatches of k_overlay, k_outline_bits and
      k_outline_apply cut into the cases by their order
There is no CPU path: without an MI355X the first two forms fail."""
import argparse
import collections
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsplat.js_amd", "py")]

WARM = 3
TINT = (1.0, 0.5, 0.0)
RGB, ALPHA, THRESHOLD = (1.0, 1.0, 1.0), 1.0, 0.5


def cases_of(widths):
    return [None] + [(w, side) for w in widths for side in ("outer", "inner")]   # (--off-only: no widths)


def name_of(case):
    return "off" if case is None else "%d %s" % case


def summarise(directory, samples, widths):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [(int(d["Start_Timestamp"]), int(d["End_Timestamp"]), d["Kernel_Name"]) for d in csv.DictReader(f)]
    rows.sort()
    per = collections.OrderedDict((k, []) for k in ("k_overlay", "k_outline_bits", "k_outline_apply"))
    for s, e, n in rows:
        for k in per:
            if k + "<" in n or k + "(" in n or n.endswith(k):
                per[k].append((e - s) / 1e3)
    cases, each = cases_of(widths), WARM + samples
    assert len(per["k_overlay"]) == each * len(cases), (len(per["k_overlay"]), each, len(cases))
    assert len(per["k_outline_bits"]) == len(per["k_outline_apply"]) == each * (len(cases) - 1)
    print("%-10s %12s %16s %17s   (us, median of %d dispatches; smallest in brackets)" % ("outline", "k_overlay", "k_outline_bits", "k_outline_apply", samples))
    for i, case in enumerate(cases):
        cut = lambda k, j: per[k][j * each + WARM:(j + 1) * each]
        cell = lambda v: "%.1f [%.1f]" % (statistics.median(v), min(v)) if v else "--"
        print("%-10s %12s %16s %17s" % (name_of(case), cell(cut("k_overlay", i)), cell(cut("k_outline_bits", i - 1) if case else []),
                                        cell(cut("k_outline_apply", i - 1) if case else [])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--widths", default="1,2,16")
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--ring-cases", default="off;2 outer;16 outer")
    ap.add_argument("--passes-only", action="store_true")
    ap.add_argument("--summarise", metavar="DIR")
    ap.add_argument("--off-only", action="store_true", help="the pass without an outline alone, and no call of the outline's entry point: "
                    "the form a build from before the outline runs too (its k_overlay beside this build's, in one job)")
    args = ap.parse_args()
    widths = [] if args.off_only else [int(w) for w in args.widths.split(",")]
    if args.summarise:
        return summarise(args.summarise, args.samples, widths)

    import numpy as np
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS[args.config]
    W, H = cfg["width"], cfg["height"]
    r = gh.HIPRenderer(W, H)
    r.set_scene_rows(gh.synth.config_rows(args.config))
    poses = [gh.orbit_camera(k, 120, W, H, cfg["fx"]) for k in range(120)]
    r.set_camera(poses[0])
    r.render_async()
    r.sync()
    r.set_overlay(TINT, 0.5)
    selected = r.select_region((W // 3, H // 3, 2 * W // 3, 2 * H // 3))

    def set_outline(case):
        if case is None:
            if not args.off_only:
                r.set_overlay_outline(None)
        else:
            r.set_overlay_outline(RGB, ALPHA, THRESHOLD, case[0], case[1])

    out = {"config": args.config, "width": W, "height": H, "selected": int(selected), "threshold": THRESHOLD, "samples": args.samples,
           "build_id": gh.build_id(), "pass_us": {}, "edge_pixels": {}}
    for case in cases_of(widths):
        set_outline(case)
        times = []
        for k in range(WARM + args.samples):
            r.set_overlay(TINT, 0.5 if k & 1 else 0.25)          # changed options: the image is stale, the next enqueue runs the pass
            r.sync()
            t0 = time.perf_counter()
            r.overlay_async()
            r.sync()
            times.append((time.perf_counter() - t0) * 1e6)
        times = times[WARM:]
        out["pass_us"][name_of(case)] = {"min": round(min(times), 1), "median": round(statistics.median(times), 1)}
    if args.passes_only:
        r.dispose()
        return
    set_outline(None)
    plain = r.read_overlay()[0].view(np.uint32)
    out["inside_pixels"] = int((r.read_overlay()[1] >= np.float32(THRESHOLD)).sum())
    for case in cases_of(widths)[1:]:
        set_outline(case)
        out["edge_pixels"][name_of(case)] = int((r.read_overlay()[0].view(np.uint32) != plain).any(axis=2).sum())

    # an RGBA8 overlay ring: every frame is rendered, the pass (and the outline) runs behind it, the image is converted and copied
    slots = 3
    r.open_delivery(slots)
    r.delivery_set_overlay(True)
    ring_cases = [None if c.strip() == "off" else (int(c.split()[0]), c.split()[1]) for c in args.ring_cases.split(";")]
    fps = {name_of(c): [] for c in ring_cases}
    for leg in range(3):                                          # alternating legs
        for case in ring_cases:
            set_outline(case)
            pending = collections.deque()

            def frame(k):
                r.set_camera(poses[k % 120])
                r.render_async()
                pending.append(r.deliver())
                if len(pending) == slots:
                    s = r.acquire(pending.popleft())
                    r.release(s[0])

            for k in range(20):
                frame(k)
            t0 = time.perf_counter()
            for k in range(args.frames):
                frame(20 + k)
            while pending:
                s = r.acquire(pending.popleft())
                r.release(s[0])
            fps[name_of(case)].append(round(args.frames / (time.perf_counter() - t0), 1))
    out["overlay_ring_frames_per_sec"] = fps
    r.close_delivery()
    r.dispose()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

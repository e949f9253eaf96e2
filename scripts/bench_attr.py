#!/usr/bin/env python3
"""What the splat-data calls cost on C3 (1 M splats): a fixed sequence of gsr_attr_stats / gsr_attr_histogram / gsr_select_attr
calls to be run under a kernel trace, and the summary of that trace.

  python scripts/bench_attr.py [--config C3] [--repeats 5] [--lib PATH]
      the workload: for OPACITY (4 bytes per splat), DISTANCE (12) and SCALE_MAX (16), at 256 and 4096 bins, on three data sets --
      "seeded" (the scene as it is, the range its own [min, max]), "one bin" (the range widened until bin 0 holds every splat:
      every lane of every wave meets in one counter) and "1 % scope" (GSR_SCOPE_SELECTED over a scattered 1 % selection) -- each
      call `repeats` times; the histogram through both of k_attr_hist's forms (a second context created under GSR_ATTR_HIST=peel);
      then gsr_select_contrib of the three stats after a two-pose tour (k_contrib_select, the yardstick of the same one-lane-per-splat
      form).  Prints the plan as one JSON line: the label of every call in the order of its kernel's dispatches.
  python scripts/bench_attr.py --contrib-only --lib PATH --host DIR
      only the tour and the gsr_select_contrib calls: what a library without the splat-data calls (the parent commit's) can run,
      through the Python host of that commit (DIR holds its gsplat_hip package: this one prototypes symbols that library lacks).
  python scripts/bench_attr.py --summarise DIR --plan FILE
      the kernels' own times from DIR's *_kernel_trace.csv of such a run (End - Start of every dispatch, the median over the
      repeats), matched to the plan's labels in dispatch order, with the bytes each kernel must read and the rate that makes."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat.js_amd", "py"))

ATTRS = (("opacity", 4), ("distance", 12), ("scale_max", 16))   # bytes of the scene a splat in scope costs
BINS = (256, 4096)
ORIGIN = (0.5, 0.0, -0.5)
POSES = (3, 40)


def workload(args):
    import numpy as np
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS[args.config]
    n = cfg["n"]
    rows = gh.synth.config_rows(args.config)
    plan = {"n": n, "repeats": args.repeats, "stats": [], "hist_peel": [], "hist_plain": [], "select": [], "contrib_select": []}

    def context(env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        r = gh.HIPRenderer(cfg["width"], cfg["height"], lib_path=args.lib)
        for k in (env or {}):
            del os.environ[k]
        r.set_scene_rows(rows)
        return r

    r = context()
    if not args.contrib_only:
        peel = context({"GSR_ATTR_HIST": "peel"})
        scattered = np.random.default_rng(7).random(n) < 0.01
        for x in (r, peel):
            x.set_selection(scattered)
        for attr, nbytes in ATTRS:
            count, nan, lo, hi = r.attr_stats(attr, origin=ORIGIN)          # (one unlabelled dispatch: the plan counts it)
            plan["stats"].append({"label": "%s (range)" % attr, "bytes": nbytes * n, "calls": 1})
            hi = float(np.nextafter(hi, np.inf))
            for _ in range(args.repeats):
                r.attr_stats(attr, origin=ORIGIN)
            plan["stats"].append({"label": "%s seeded" % attr, "bytes": nbytes * n, "calls": args.repeats})
            for _ in range(args.repeats):
                r.attr_stats(attr, origin=ORIGIN, selected=True)
            plan["stats"].append({"label": "%s 1 %% scope" % attr, "bytes": n // 8 + nbytes * int(scattered.sum()), "calls": args.repeats})
            for bins in BINS:
                sets = (("seeded", lo, hi, False, nbytes * n), ("one bin", lo, lo + (hi - lo) * bins * 2, False, nbytes * n),
                        ("1 % scope", lo, hi, True, n // 8 + nbytes * int(scattered.sum())))
                for name, a, b, sel, nb in sets:
                    for x, key in ((r, "hist_plain"), (peel, "hist_peel")):
                        for _ in range(args.repeats):
                            counts, outside, _ = x.attr_histogram(attr, a, b, bins, origin=ORIGIN, selected=sel)
                        if name == "one bin":
                            assert counts[0] == count - nan and outside[:2] == (0, 0)
                        plan[key].append({"label": "%s %d bins, %s" % (attr, bins, name), "bytes": nb, "calls": args.repeats})
            edges = gh.attr_edges(lo, hi, 256)
            for _ in range(args.repeats):
                r.select_attr(attr, edges[64], edges[192], origin=ORIGIN)
            plan["select"].append({"label": "%s middle half" % attr, "bytes": nbytes * n, "calls": args.repeats})
            r.set_selection(scattered)                                          # (the picker replaced it)
        peel.dispose()
    # the yardstick: gsr_select_contrib after a two-pose tour
    r.contrib_reset()
    for k in POSES:
        r.set_camera(gh.orbit_camera(k, width=cfg["width"], height=cfg["height"], fx=cfg["fx"]))
        r.render_async()
        r.sync()
        r.contrib_accumulate()
    for stat, nbytes in (("weight", 8), ("peak", 4), ("pixels", 4)):
        for _ in range(args.repeats):
            r.select_contrib(stat, below=1.0)
        plan["contrib_select"].append({"label": "select_contrib %s" % stat, "bytes": nbytes * n, "calls": args.repeats})
    r.dispose()
    print(json.dumps(plan))


KERNELS = (("stats", "k_attr_stats("), ("hist_plain", "k_attr_hist<0>"), ("hist_peel", "k_attr_hist<1>"), ("select", "k_attr_select("),
           ("contrib_select", "k_contrib_select("))


def summarise(directory, plan_path):
    plan = json.loads([l for l in open(plan_path).read().splitlines() if l.startswith("{")][-1])
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [(int(d["Start_Timestamp"]), int(d["End_Timestamp"]), d["Kernel_Name"]) for d in csv.DictReader(f)]
    rows.sort()
    for key, needle in KERNELS:
        times = [(e - s) * 1e-3 for s, e, name in rows if needle in name]
        want = sum(p["calls"] for p in plan[key])
        if not want:
            continue
        assert len(times) == want, "%s: %d dispatches in the trace, %d in the plan" % (needle, len(times), want)
        print("%s   (us: median, min over the repeats; bytes the kernel must read; GB/s at the median)" % needle.rstrip("("))
        at = 0
        for p in plan[key]:
            t = times[at:at + p["calls"]]
            at += p["calls"]
            med = statistics.median(t)
            print("  %-34s %8.2f %8.2f   %10d B   %7.1f GB/s" % (p["label"], med, min(t), p["bytes"], p["bytes"] / med * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--contrib-only", action="store_true")
    ap.add_argument("--host", metavar="DIR", default=None)
    ap.add_argument("--summarise", metavar="DIR")
    ap.add_argument("--plan", metavar="FILE")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.plan)
    if args.host:
        sys.path.insert(0, os.path.abspath(args.host))
    return workload(args)


if __name__ == "__main__":
    main()

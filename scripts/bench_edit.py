#!/usr/bin/env python3
"""What editing the selection costs on C3 (1 M splats): the stream interval per call of gsr_scene_translate_selected /
_rotate_selected (pivoted) / _scale_selected (pivoted) / _set_rgba_selected at selection fractions 0, 1 %, 50 % and 100 %, as random
bits and as one contiguous block, beside the whole-scene gsr_scene_rotate of the same build (the yardstick) and the wall time of
the blocking gsr_selection_bounds.  The stream interval per call is the interval between two events on the context's stream around
`batch` back-to-back calls from this Python host, divided by the batch; the figure reported is the median over the repeats.  It is
the larger of the kernel's time and what the host needs to enqueue one call (ctypes, argument conversion, the launch), host
enqueue included: a kernel shorter than that is hidden behind it, so the empty selection's figure is the floor of each call and
figures at that floor are upper bounds of the kernel's time, not measurements of it.  Writes profiles/edit_bench_<build id>.json
(or --out) and prints the same JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat.js_amd", "py"))

Q = (0.0, 0.008726535498373935, 0.0, 0.9999619230641713)   # one degree about y
PIVOT = (0.5, 0.0, -0.5)
FRACTIONS = (0.0, 0.01, 0.5, 1.0)


def summary(ms):
    return {"median_us": round(statistics.median(ms) * 1e3, 3), "min_us": round(min(ms) * 1e3, 3), "max_us": round(max(ms) * 1e3, 3), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--batch", type=int, default=200)   # about 1 to 3 ms between the two events
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS[args.config]
    n = cfg["n"]
    r = gh.HIPRenderer(cfg["width"], cfg["height"])
    r.set_scene_rows(gh.synth.config_rows(args.config))
    stream = torch.cuda.ExternalStream(r.stream_handle())

    def stream_interval(call):
        """median over the repeats of (interval between two events around `batch` calls) / batch: host enqueue included"""
        for _ in range(3):
            call()
        r.sync()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.batch):
                call()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.batch)
        return summary(ms)

    edits = {
        "translate": lambda: r.scene_translate_selected((1e-4, 0.0, -1e-4)),
        "rotate_pivot": lambda: r.scene_rotate_selected(Q, PIVOT),
        "scale_pivot": lambda: r.scene_scale_selected((1.0001, 1.0, 0.9999), PIVOT),
        "set_rgba": lambda: r.scene_set_rgba_selected(0x80000000, "a"),
    }
    out = {"config": args.config, "n": n, "build_id": gh.build_id(), "batch": args.batch, "figure": "stream interval per call, host enqueue included; figures at the empty selection's floor are upper bounds",
           "whole_scene_rotate": stream_interval(lambda: r.scene_rotate(Q)),
           "selected": {}, "selection_bounds_wall": {}}
    rng = np.random.default_rng(7)
    for frac in FRACTIONS:
        for form in ("random", "block"):
            k = int(round(frac * n))
            sel = np.zeros(n, dtype=bool)
            if form == "random":
                sel[rng.permutation(n)[:k]] = True
            else:
                sel[n // 3:n // 3 + k] = True   # (k <= n - n // 3 for every fraction but 1; that one is the whole scene either way)
                if k > n - n // 3:
                    sel[:] = True
            assert r.set_selection(sel) == int(sel.sum())
            key = "%g_%s" % (frac, form)
            out["selected"][key] = {"count": int(sel.sum())}
            for name, call in edits.items():
                out["selected"][key][name] = stream_interval(call)
            wall = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                count = r.selection_bounds()[0]
                wall.append((time.perf_counter() - t0) * 1e3)
            assert count == int(sel.sum())
            out["selection_bounds_wall"][key] = summary(wall)
    # the duplicate leg (last: it grows the scene): the wall time of the blocking gsr_scene_duplicate_selected at the same fractions
    # (random bits), on a scene uploaded afresh for every call, without and with gsr_scene_reserve making room first -- reserved,
    # the call re-allocates nothing of the scene arrays and copies no old row
    out["duplicate_wall"] = {}
    rows = gh.synth.config_rows(args.config)
    for frac in FRACTIONS:
        k = int(round(frac * n))
        sel = np.zeros(n, dtype=bool)
        sel[rng.permutation(n)[:k]] = True
        leg = {"count": k}
        for form in ("plain", "reserved"):
            wall = []
            for _ in range(min(args.repeats, 5)):
                r.set_scene_rows(rows)
                assert r.set_selection(sel) == k
                if form == "reserved":
                    r.scene_reserve(n + k)
                r.sync()
                t0 = time.perf_counter()
                first, count = r.scene_duplicate_selected()
                wall.append((time.perf_counter() - t0) * 1e3)
                assert (first, count) == (n, k) and r.scene_capacity() == (n if not k else n + k if form == "reserved" else max(n + k, n + n // 2))
            leg[form] = summary(wall)
        out["duplicate_wall"]["%g" % frac] = leg
    r.dispose()
    path = args.out or os.path.join(ROOT, "profiles", "edit_bench_%s.json" % out["build_id"])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

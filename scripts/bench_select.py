#!/usr/bin/env python3
"""What a selection costs on C3 (1 M splats) at 1080p: the median wall time of the blocking calls, as a host sees them --
select_region in both modes over the full image and over a 256x256 window, and scene_erase_selected against scene_limit_box of
the SAME kept set (both run the same compaction; the erase reads one bit per splat where limitBox compares three positions).
Writes profiles/select_bench_<build id>.json (or --out) and prints the same JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat.js_amd", "py"))


def timed(call, repeats, before=None):
    ms = []
    for _ in range(repeats):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--pose", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--erase-repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS[args.config]
    W, H = cfg["width"], cfg["height"]
    rows = gh.synth.config_rows(args.config)
    r = gh.HIPRenderer(W, H)
    r.set_scene_rows(rows)
    cam = gh.orbit_camera(args.pose, width=W, height=H, fx=cfg["fx"])

    def frame():
        r.set_camera(cam)
        r.render_async()
        r.sync()

    frame()
    full, window = (0, 0, W, H), (W // 2 - 128, H // 2 - 128, W // 2 + 128, H // 2 + 128)
    out = {"config": args.config, "n": cfg["n"], "width": W, "height": H, "pose": args.pose, "build_id": gh.build_id(), "select_region": {}}
    r.read_depth()                               # the planes are the frame's: HIT below is the selection alone
    for mode in ("centre", "hit"):
        for name, rect in (("full", full), ("window_256", window)):
            r.select_region(rect, mode=mode)     # (first use: allocations)
            res = timed(lambda: r.select_region(rect, mode=mode), args.repeats)
            res["selected"] = r.selection_count()
            out["select_region"]["%s_%s" % (mode, name)] = res
    # the same kept set through both compactions: the splats of a box, restored from the rows before every repeat
    box = (-1.0, 2.5, -0.75, 3.0, -2.0, 1.0)
    kept = []

    def restore(select):
        r.set_scene_rows(rows)
        if select:
            r.select_box(box)

    out["select_box"] = timed(lambda: r.select_box(box), args.repeats)
    out["scene_erase_selected"] = timed(lambda: kept.append(r.scene_erase_selected(keep=True)), args.erase_repeats, before=lambda: restore(True))
    out["scene_limit_box"] = timed(lambda: kept.append(r.scene_limit_box(box)), args.erase_repeats, before=lambda: restore(False))
    assert len(set(kept)) == 1, kept             # the same kept set every time, through both
    out["kept"] = kept[0]
    r.dispose()
    path = args.out or os.path.join(ROOT, "profiles", "select_bench_%s.json" % out["build_id"])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

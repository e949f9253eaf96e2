#!/usr/bin/env python3
"""Host issue time per frame of several library builds in ONE process, alternating rounds: scripts/host_overhead.py's
measurement without the exchange (three throughput band contexts on C1, camera upload + frame enqueue per frame), as an A/B
in the manner of scripts/ab_bench.py -- one process per build varies by more than a build can add.

  [GSR_NO_GRAPH=1] python scripts/host_issue_ab.py base NAME ...

`base` = gsplat.js_amd/lib/libgsplat_hip.so, any other name = gsplat.js_amd/lib_exp/<name>/libgsplat_hip.so
(scripts/build_exp.sh).  Ratios are against the first build named."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "gsplat.js_amd", "py"))
import numpy as np
import torch  # noqa
import gsplat_hip as gh
from gsplat_hip import bands
cfg = gh.synth.CONFIGS["C1"]
W, H = cfg["width"], cfg["height"]
scene = gh.Scene(); scene.setData(gh.synth.config_rows("C1"))
edges = bands.band_edges(W, 8)
F = 3
names = sys.argv[1:]
def lib_of(n): return None if n == "base" else os.path.join(ROOT, "gsplat.js_amd", "lib_exp", n, "libgsplat_hip.so")
ctx = {}
for n in names:
    rs = [gh.HIPRenderer(W, H, band=edges[3], timing=True, throughput=True, lib_path=lib_of(n)) for _ in range(F)]
    for r in rs:
        r.render(scene, gh.orbit_camera(0, 120, W, H, cfg["fx"])); r.set_timing_interval(8)
    ctx[n] = rs
poses = [gh.orbit_camera(k, 120, W, H, cfg["fx"]).f32() for k in range(120)]
N, ROUNDS = 1500, 11
res = {n: [] for n in names}
for rnd in range(ROUNDS + 1):
    for n in names:
        rs = ctx[n]
        t0 = time.perf_counter()
        for k in range(N):
            v, p, vp = poses[k % 120]; r = rs[k % F]
            r.set_camera_arrays(v, p, vp, cfg["fx"], cfg["fx"]); r.render_async()
        t = time.perf_counter() - t0
        for r in rs: r.sync()
        if rnd: res[n].append(t / N * 1e6)
print("host issue us/frame, GSR_NO_GRAPH=%s, %d rounds x %d frames, builds alternating in one process" % (os.environ.get("GSR_NO_GRAPH", ""), ROUNDS, N))
b = np.array(res[names[0]])
for n in names:
    a = np.array(res[n]); q = a / b
    print("%-10s median %.2f us (%.2f .. %.2f)   ratio to %s per round: median %.4f, %.4f .. %.4f" % (n, np.median(a), a.min(), a.max(), names[0], np.median(q), q.min(), q.max()))

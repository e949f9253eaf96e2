#!/usr/bin/env python3
"""Two frames of a configuration in one context, for a kernel trace of exactly one frame in each sort order (the first frame of a
scene sorts in the LSD order, the second in the bucket order):

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/two_frames.py LIB default|throughput [CONFIG]

LIB = base (gsplat.js_amd/lib) or a name under gsplat.js_amd/lib_exp (scripts/build_exp.sh).  profiles/sort_plan_resources.txt
compares the kernel names, counts, grids, workgroup and LDS sizes of a build and its parent this way."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsplat.js_amd", "py")]
import gsplat_hip as gh  # noqa: E402

lib, kind = sys.argv[1], sys.argv[2]
name = sys.argv[3] if len(sys.argv) > 3 else "C3"
cfg = gh.synth.CONFIGS[name]
W, H = cfg["width"], cfg["height"]
scene = gh.Scene()
scene.setData(gh.synth.config_rows(name))
path = None if lib == "base" else os.path.join(ROOT, "gsplat.js_amd", "lib_exp", lib, "libgsplat_hip.so")
r = gh.HIPRenderer(W, H, throughput=kind == "throughput", lib_path=path)
for k in (21, 22):
    r.render(scene, gh.orbit_camera(k, 120, W, H, cfg["fx"]))
print("two frames of %s, %s context, build %s" % (name, kind, lib))
r.dispose()

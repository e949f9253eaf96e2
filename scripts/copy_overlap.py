#!/usr/bin/env python3
"""Summary of a kernel + memory-copy trace of the delivery ring (scripts/gpu.sh copytrace DIR ...): how long the
frames' device-to-host copies take, the rate that is for `bytes` per copy, how much of their time lies under compositor or
front-end kernels of OTHER frames (the point of the ring), and the conversion kernel's (k_deliver_rgba8 / k_deliver_yuv) own time
and rate.
usage: python scripts/copy_overlap.py DIR BYTES_PER_COPY [skip_fraction]      (DIR: the trace task's output directory)"""
import csv
import glob
import sys

root, nbytes = sys.argv[1], int(sys.argv[2])
skip = float(sys.argv[3]) if len(sys.argv) > 3 else 0.3


def load(pattern):
    files = glob.glob(root + "/**/" + pattern, recursive=True)
    if not files:
        sys.exit("no %s under %s" % (pattern, root))
    return list(csv.DictReader(open(files[0])))


ktrace = load("*kernel_trace.csv")
kernels = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].replace("gsr::", "").replace("void ", "").split("(")[0].split("<")[0], r.get("Queue_Id", "?")) for r in ktrace]
copies = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in load("*memory_copy_trace.csv") if "DEVICE_TO_HOST" in r.get("Direction", "").upper()]
how = "copy engine (memory-copy trace)"
if not copies:
    # This runtime moves a pinned device-to-host hipMemcpyAsync with its own blit kernel, which the memory-copy domain does not
    # list: the copies are then kernels of the kernel trace.
    copies = [(k[0], k[1]) for k in kernels if k[2] == "__amd_rocclr_copyBuffer"]
    how = "the runtime's blit kernel __amd_rocclr_copyBuffer (kernel trace; the memory-copy trace lists no device-to-host copy)"
    print("queues: copies on %s, render chain on %s" % (sorted({k[3] for k in kernels if k[2] == "__amd_rocclr_copyBuffer"}),
                                                       sorted({k[3] for k in kernels if k[2].startswith("k_")})))
kernels = [k for k in kernels if k[2].startswith("k_")]
t_first, t_last = min(k[0] for k in kernels), max(k[1] for k in kernels)
t0 = t_first + (t_last - t_first) * skip
kernels = [k for k in kernels if k[0] >= t0]
# the frames' copies: the long ones (the few-byte copies of the frame words are microseconds)
frame_copies = sorted(c for c in copies if c[0] >= t0 and c[1] - c[0] >= 1e-3 * nbytes / 200.0)   # (200 GB/s: no link is that fast)
if not frame_copies:
    sys.exit("no frame-sized device-to-host copy in the trace")
dur = sorted(c[1] - c[0] for c in frame_copies)
med = dur[len(dur) // 2]
# time of every copy during which a kernel of the render chain (anything but the conversion kernel) is running
spans = sorted((k[0], k[1]) for k in kernels if not k[2].startswith("k_deliver"))
merged = []
for s, e in spans:
    if merged and s <= merged[-1][1]:
        merged[-1][1] = max(merged[-1][1], e)
    else:
        merged.append([s, e])
under = 0
total = 0
for cs, ce in frame_copies:
    total += ce - cs
    for s, e in merged:
        if e <= cs:
            continue
        if s >= ce:
            break
        under += min(e, ce) - max(s, cs)
print("frame copies (device to host, %d bytes each) by %s: %d in the steady state" % (nbytes, how, len(frame_copies)))
print("  duration us: median %.1f  p10 %.1f  p90 %.1f  -> %.1f GB/s at the median" % (med / 1e3, dur[len(dur) // 10] / 1e3, dur[len(dur) * 9 // 10] / 1e3, nbytes / med))
print("  share of copy time under render-chain kernels of other frames: %.1f %%" % (100.0 * under / total))
span = frame_copies[-1][1] - frame_copies[0][0]
print("  copy engine busy %.1f %% of the steady state (%.1f us per frame between copy starts)" % (100.0 * total / span, span / 1e3 / max(1, len(frame_copies) - 1)))
# the conversion kernel reads 16 bytes per pixel of the f32 framebuffer and writes the copy's bytes: 4 per pixel as RGBA8, 1.5 as 4:2:0
for name, moved in (("k_deliver_rgba8", nbytes * 5), ("k_deliver_yuv", nbytes * 2 // 3 * 16 + nbytes)):
    dk = sorted(k[1] - k[0] for k in kernels if k[2] == name)
    if dk:
        m = dk[len(dk) // 2]
        print("%s: %d launches, median %.2f us (p90 %.2f): %.0f GB/s for the %d bytes it moves" % (name, len(dk), m / 1e3, dk[len(dk) * 9 // 10] / 1e3, moved / m, moved))
by = {}
for s, e, n, _q in kernels:
    by.setdefault(n, []).append(e - s)
for n, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
    print("  %-28s %6d launches  avg %8.2f us" % (n, len(v), sum(v) / len(v) / 1e3))

#!/usr/bin/env python3
"""Cost of the depth exchange (gsr_comm_set_depth) on one GPU: a world of `--world` ranks (spawned processes, a host-staged gloo
all-gather through gsr_comm_init_custom), `--frames` orbit poses per option: off, then every `--depth FORMAT:STEP` given.
Prints one JSON line per option with the frames/s of rank 0 -- a host-staged collective dominates that figure; the finding is
the kernel times of a `rocprofv3 --kernel-trace --stats -- python scripts/depth_exchange_trace.py ...` run of the same."""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(rank, world, port, args):
    sys.path.insert(0, os.path.join(ROOT, "gsplat.js_amd", "py"))
    import torch
    import torch.distributed as dist
    import gsplat_hip as gh
    from gsplat_hip import bands
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = gh.synth.CONFIGS[args.config]
        W, H = cfg["width"], cfg["height"]
        scene = gh.Scene()
        scene.setData(gh.synth.config_rows(args.config))
        dev = torch.device("cuda:0")

        def allgather(send, recv, nbytes, stream):
            s = torch.cuda.ExternalStream(stream, device=dev)
            s.synchronize()
            mine = torch.as_tensor(bands.DevicePointer(send, (nbytes,), "|u1"), device=dev).cpu()
            every = torch.empty(world * nbytes, dtype=torch.uint8)
            dist.all_gather_into_tensor(every, mine)
            with torch.cuda.stream(s):
                torch.as_tensor(bands.DevicePointer(recv, (world * nbytes,), "|u1"), device=dev).copy_(every)
            s.synchronize()

        a = gh.HIPRenderer(W, H, device=0)
        a.join_group_custom(rank, world, bands.band_edges(W, world), allgather)
        cams = [gh.orbit_camera(k, width=W, height=H, fx=cfg["fx"]) for k in range(args.frames)]
        a.render(scene, cams[0])
        for option in ["off"] + args.depth:
            if option == "off":
                a.set_group_depth(None)
            else:
                fmt, step = option.split(":")
                a.set_group_depth(fmt, int(step), 0.1)
            rates = []
            for rep in range(args.repeats + 1):                  # (the first repeat warms up)
                dist.barrier()
                t0 = time.perf_counter()
                for cam in cams:
                    a.set_camera(cam)
                    a.render_async()
                    a.allgather_frame_async()
                a.sync()
                if rep:
                    rates.append(args.frames / (time.perf_counter() - t0))
            if rank == 0:
                print(json.dumps({"config": args.config, "world": world, "depth": option, "frames_per_s": [round(r, 1) for r in rates]}), flush=True)
        a.dispose()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--depth", action="append", default=[], metavar="FORMAT:STEP", help="u16:2, f32:1, ... (repeatable)")
    args = ap.parse_args()
    args.depth = args.depth or ["u16:2", "f32:1"]
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.spawn(worker, args=(args.world, port, args), nprocs=args.world, join=False)
    deadline = time.time() + 400
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            sys.exit("the world did not finish")


if __name__ == "__main__":
    main()

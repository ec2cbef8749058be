#!/usr/bin/env python
"""Frames/s of host-u8 (rtp_submit_frame) against device-u8 (rtp_submit_frame_device) submission of the same 720p frames.

bench.py's default engine shape (batch_frames 2, frames_in_flight 7, GPU_MAX_HW_QUEUES=8 before the first HIP call); each leg runs in a
fresh process of its own, one after the other on the same box, and prints one JSON line; the parent prints both and their ratio.
  python tools/bench_device_frames.py [--steps 600] [--warmup 60] [--render] [--stamps]
--render: render = 1 and the rendered frame collected too (collect_rendered into host memory / collect_rendered_device into a device
tensor).  --stamps: the legs also report the mean device-side residency (rtp_stamp_probe) of the import or warp, area/pad and export
launches.  --leg host|device runs one leg in this process.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch   # first: one HIP runtime for torch and the engine
    import caffe_rtpose_amd as r
    B, depth = 2, 7
    e = r.Engine(r.Config(batch_frames=B, frames_in_flight=depth, render=1 if args.render else 0))
    imgs = [r.synth_frame(1280, 720, i, seed=3) for i in range(8)]
    side = torch.cuda.Stream()
    if args.leg == "device":
        frames = [torch.from_numpy(im).cuda() for im in imgs]
        out = torch.empty((720, 1280, 3), dtype=torch.uint8, device="cuda")
    host_out = np.empty((720, 1280, 3), np.uint8)
    torch.cuda.synchronize()

    def submit(i):
        if args.leg == "device":
            e.submit_frame_device(frames[i % 8], tag=i, stream=side)
        else:
            e.submit_frame(imgs[i % 8], tag=i)

    def collect():
        if not args.render:
            return e.collect()
        if args.leg == "device":
            return e.collect_rendered_device(out, stream=side)
        t, n, j, img = e.collect_rendered()
        host_out[...] = img
        return t, n, j

    def run(k):
        sub = col = 0
        while col < k:
            while sub < k and e.in_flight() < depth:
                submit(sub)
                sub += 1
            collect()
            col += 1

    run(args.warmup)
    if args.stamps:
        e.stamp_probe(1)
    t = time.perf_counter()
    run(args.steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    res = dict(leg=args.leg, render=bool(args.render), frames=args.steps, fps=round(args.steps / dt, 1), ms_per_frame=round(dt / args.steps * 1e3, 4),
               hw_queues=int(os.environ.get("GPU_MAX_HW_QUEUES", "4")))
    if args.stamps:
        spans = e.stamp_probe(-1)
        e.stamp_probe(0)
        slot = spans[:, 0].astype(int)
        us = spans[:, 2] - spans[:, 1]
        classes = {"import_or_warp": (slot >= 200) & (slot % 2 == 0), "area_pad": (slot >= 200) & (slot % 2 == 1),
                   "export": (slot >= 64) & (slot < 200) & ((slot - 64) % 8 == 5)}
        res["stamps_us"] = {k: (round(float(us[m].mean()), 2) if m.any() else None) for k, m in classes.items()}
        res["stamps_n"] = {k: int(m.sum()) for k, m in classes.items()}
    e.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--render", action="store_true")
    ap.add_argument("--stamps", action="store_true")
    ap.add_argument("--leg", choices=["host", "device"])
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")   # read by the HIP runtime at the leg's first call
    out = {}
    for name in ("host", "device"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--steps", str(args.steps), "--warmup", str(args.warmup)]
        cmd += ["--render"] * args.render + ["--stamps"] * args.stamps
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit(f"{name} leg failed with exit status {p.returncode}")
        out[name] = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    out["device_over_host"] = round(out["device"]["fps"] / out["host"]["fps"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

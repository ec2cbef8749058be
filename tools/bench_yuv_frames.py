#!/usr/bin/env python
"""Frames/s of 720p frames submitted as host I420 (rtp_submit_frame_yuv), as the same pixels in host BGR (rtp_submit_frame) and as
device NV12 (rtp_submit_frame_yuv_device), and the conversion kernel's own time.

One process, one engine of bench.py's default shape (batch_frames 2, frames_in_flight 7, GPU_MAX_HW_QUEUES=8 before the first HIP
call).  Every round runs the legs bgr, i420, nv12, bgr one after the other, so each round has two BGR runs: their difference is the
run-to-run spread the YUV legs are read against.  The BGR frames are rtp_convert_yuv of the I420 planes: all legs compute the same
joints.  The kernel time is HIP-event time over rtp_convert_yuv_device launches at 1280x720 and 1920x1080 that were all queued
behind a sleeping kernel, so the GPU runs them back to back and the host's cost per call (reported next to it) stays outside.
  python tools/bench_yuv_frames.py [--steps 600] [--warmup 60] [--rounds 3] [--kernel_iters 200]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel_iters", type=int, default=200)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # read by the HIP runtime at its first call (bench.py's setting; a caller's value wins)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch   # first: one HIP runtime for torch and the engine
    import caffe_rtpose_amd as r
    import _yuvcases as yc

    B, depth = 2, 7
    e = r.Engine(r.Config(batch_frames=B, frames_in_flight=depth))
    planes = [yc.from_bgr(r.synth_frame(1280, 720, i, seed=3)) for i in range(8)]
    bgr = [r.convert_yuv(*p) for p in planes]
    nv12 = [(torch.from_numpy(y).cuda(), torch.from_numpy(yc.interleave(u, v)).cuda()) for y, u, v in planes]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    submit = {
        "bgr": lambda i: e.submit_frame(bgr[i % 8], tag=i),
        "i420": lambda i: e.submit_frame_yuv(*planes[i % 8], tag=i),
        "nv12": lambda i: e.submit_frame_yuv_device(*nv12[i % 8], tag=i, stream=side),
    }

    def run(leg, k):
        sub = col = 0
        people = 0
        while col < k:
            while sub < k and e.in_flight() < depth:
                submit[leg](sub)
                sub += 1
            people += e.collect()[1]
            col += 1
        return people

    for leg in submit:
        run(leg, args.warmup)
    fps = {"bgr_1": [], "i420": [], "nv12": [], "bgr_2": []}
    people = {}
    for rnd in range(args.rounds):
        for name in fps:
            leg = name.split("_")[0]
            t = time.perf_counter()
            people.setdefault(leg, run(leg, args.steps))
            torch.cuda.synchronize()
            fps[name].append(round(args.steps / (time.perf_counter() - t), 1))
        print(json.dumps({"round": rnd, **{k: v[-1] for k, v in fps.items()}}), flush=True)
    e.synchronize()
    assert len(set(people.values())) == 1, f"the legs found different people: {people}"
    allbgr = fps["bgr_1"] + fps["bgr_2"]
    med = {k: statistics.median(v) for k, v in (("bgr", allbgr), ("i420", fps["i420"]), ("nv12", fps["nv12"]))}
    spread = max(abs(a - b) for a, b in zip(fps["bgr_1"], fps["bgr_2"]))
    summary = dict(frames_per_leg=args.steps, rounds=args.rounds, hw_queues=int(os.environ["GPU_MAX_HW_QUEUES"]), median_fps=med, bgr_min=min(allbgr), bgr_max=max(allbgr),
                   bgr_run_to_run_spread_fps=round(spread, 1), i420_minus_bgr_fps=round(med["i420"] - med["bgr"], 1),
                   nv12_minus_bgr_fps=round(med["nv12"] - med["bgr"], 1),
                   i420_slower_than_bgr_by_more_than_the_spread=bool(med["bgr"] - med["i420"] > spread),
                   h2d_bytes_per_frame=dict(bgr=1280 * 720 * 3, i420=1280 * 720 * 3 // 2, nv12=0))
    print(json.dumps(summary), flush=True)

    # the conversion kernel alone: HIP events around launches queued behind a sleep on one stream (the interval includes the gaps
    # between consecutive kernels of a stream, not the host's cost of a call)
    sleep_cycles = 100_000_000   # ~50 ms: longer than queueing kernel_iters calls takes (checked: all_queued_behind_the_sleep)
    for w, h in ((1280, 720), (1920, 1080)):
        y, u, v = yc.planes(w, h, "420", seed=1)
        out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
        layouts = {"i420": (torch.from_numpy(y).cuda(), torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()),
                   "nv12": (torch.from_numpy(y).cuda(), torch.from_numpy(yc.interleave(u, v)).cuda(), None),
                   # an odd start puts the same frame on the byte-wise kernel
                   "i420_generic": (torch.from_numpy(np.pad(y, ((0, 0), (1, 0)))).cuda()[:, 1:], torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda())}
        for name, (dy, du, dv) in layouts.items():
            with torch.cuda.stream(side):
                for _ in range(20):
                    e.convert_yuv_device(dy, du, dv, out, stream=side)
                side.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda._sleep(sleep_cycles)   # the launches below pile up behind it: the interval a..b holds GPU work only
                a.record(side)
                t = time.perf_counter()
                for _ in range(args.kernel_iters):
                    e.convert_yuv_device(dy, du, dv, out, stream=side)
                host_us = (time.perf_counter() - t) * 1e6 / args.kernel_iters
                queued = not a.query()            # the sleep was still running when the last launch was queued
                b.record(side)
            b.synchronize()
            us = a.elapsed_time(b) * 1e3 / args.kernel_iters
            moved = w * h * 3 // 2 + w * h * 3
            print(json.dumps(dict(kernel=name, size=f"{w}x{h}", us_per_launch_back_to_back=round(us, 2), bytes_moved=moved,
                                  gb_per_s=round(moved / us / 1e3, 1), launches=args.kernel_iters, all_queued_behind_the_sleep=queued,
                                  host_us_per_call=round(host_us, 2))), flush=True)
    e.close()


if __name__ == "__main__":
    main()

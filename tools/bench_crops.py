#!/usr/bin/env python
"""Crops mode (crops.hip): what the kernel costs, and what the mode does to the frame rate.

(a) The kernel alone on a 1280x720 display image for 1, 8 and 96 people (rtp_internal_crops_time: the launches of a round are
    enqueued behind a wave that holds the stream, so that they run back to back and the event pair brackets device work only; the
    figure is a launch's period in the train = kernel + the boundary to the next launch), in four cases:
      hwc128   128x128 HWC_BGR crops of 256-pixel boxes   (a step of 2 pixels: 2 x 2 samples per output)
      chw256   256x256 CHW_RGB crops of 256-pixel boxes   (a step of 1: one sample, the 16-byte planar stores)
      magnify  128x128 HWC_BGR crops of 40-pixel boxes    (a step of 0.31: neighbouring outputs share their taps)
      s4       128x128 HWC_BGR crops of 640-pixel boxes   (a step of 5: 4 x 4 samples per output)
    and the byte-wise store path next to hwc128 (120x128 crops: crop_w no multiple of 16).
(b) One engine (656x368 net, 1280x720 host u8 frames, 7 in flight, batches of 2: bench.py's configuration) with the mode off, and
    with 16 crops of 128x128 in both ways of getting the pixels to the host (a copy of the 16 slots behind the kernel; the kernel
    storing into mapped pinned memory), alternated --runs times in one process: frames/s over --frames frames after a warm-up, each
    frame peeked (rtp_peek_crops) and collected.
  python tools/bench_crops.py [--launches 200] [--rounds 7] [--frames 600] [--runs 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1280, 720
NET_W, NET_H = 656, 368
KERNEL_CASES = [("hwc128", 128, 128, "hwc_bgr", 256.0), ("chw256", 256, 256, "chw_rgb", 256.0), ("magnify", 128, 128, "hwc_bgr", 40.0), ("s4", 128, 128, "hwc_bgr", 640.0),
                ("hwc120_bytewise", 120, 128, "hwc_bgr", 256.0)]


def people(np, n, num_parts, box, aspect):
    """n people whose parts 1 and 8 span a box of `box` pixels height at pseudo-random places of the display"""
    rng = np.random.default_rng(7)
    j = np.zeros((n, num_parts, 3), np.float32)
    cx, cy = rng.uniform(0.15 * W, 0.85 * W, n), rng.uniform(0.2 * H, 0.8 * H, n)
    j[:, 1] = np.stack([cx - box * aspect / 2, cy - box / 2, np.full(n, 0.9)], 1)
    j[:, 8] = np.stack([cx + box * aspect / 2, cy + box / 2, np.full(n, 0.9)], 1)
    return j


def kernel_legs(r, np, args):
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_crops_time
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_ubyte), _lib.fp, C.c_int, C.c_int, C.POINTER(C.c_float)]
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=2))
    img = np.ascontiguousarray(r.synth_frame(W, H, 1, seed=3))
    out = []
    for name, cw, ch, layout, box in KERNEL_CASES:
        for n in (1, 8, 96):
            e.set_crops_output(cw, ch, 96, layout=layout)
            j = people(np, n, e.num_parts, box, cw / ch)
            boxes, crops = e.crops_from_joints(img, j)
            want_b, want_c = r.crop_people(img, j, e.num_parts, cw, ch, 96, layout=layout)
            assert np.array_equal(boxes.view(np.uint32), want_b.view(np.uint32)) and np.array_equal(crops, want_c), name
            us = []
            for _ in range(args.rounds):
                p = C.c_float()
                e._chk(fn(e.h, img.ctypes.data_as(C.POINTER(C.c_ubyte)), j.ctypes.data_as(_lib.fp), n, args.launches, C.byref(p)))
                us.append(p.value)
            step = float(boxes[0][2]) / cw
            out.append(dict(case=name, people=n, crop=f"{cw}x{ch}", layout=layout, step_pixels=round(step, 3), launches=args.launches * args.rounds,
                            kernel_period_us_median=round(float(np.median(us)), 1), kernel_period_us_min=round(min(us), 1), kernel_period_us_max=round(max(us), 1),
                            crop_mb=round(n * cw * ch * 3 / 1e6, 2)))
            print(json.dumps(out[-1]), flush=True)
    e.set_crops_output(None)
    e.close()
    return out


def run_frames(e, frames, n, in_flight, peek):
    t = time.perf_counter()
    for i in range(n):
        if e.in_flight() >= in_flight:
            peek()
            e.collect()
        e.submit_frame(frames[i % len(frames)], tag=i)
    while e.in_flight():
        peek()
        e.collect()
    return n / (time.perf_counter() - t)


def rate_legs(r, np, args):
    from caffe_rtpose_amd import _lib
    direct = _lib.lib.rtp_internal_crops_direct
    direct.restype, direct.argtypes = C.c_int, [C.c_void_p, C.c_int]
    in_flight = 7
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=in_flight, batch_frames=2))
    frames = [r.synth_frame(W, H, i, seed=3) for i in range(8)]
    cases = [("off", None), ("crops16_copy_behind_kernel", 0), ("crops16_kernel_stores_to_pinned", 1)]
    seen = {}

    def set_case(name, how):
        e.set_crops_output(None)
        if how is None:
            return lambda: None
        e._chk(direct(e.h, how))
        e.set_crops_output(128, 128, 16, margin=0.15)

        def peek():
            _, boxes, _ = e.peek_crops()
            seen[name] = seen.get(name, 0) + len(boxes)
        return peek
    out = []
    for name, how in cases:   # warm-up of every case: buffers, code objects
        run_frames(e, frames, 100, in_flight, set_case(name, how))
    seen.clear()
    for run in range(args.runs):
        for name, how in cases:
            fps = run_frames(e, frames, args.frames, in_flight, set_case(name, how))
            out.append(dict(case=name, run=run, frames=args.frames, frames_per_s=round(fps, 1)))
            print(json.dumps(out[-1]), flush=True)
    e.set_crops_output(None)
    e._chk(direct(e.h, 0))
    e.close()
    med = {c[0]: float(np.median([o["frames_per_s"] for o in out if o["case"] == c[0]])) for c in cases}
    print(json.dumps(dict(frames_per_s_median={k: round(v, 1) for k, v in med.items()}, relative_to_off={k: round(v / med["off"], 3) for k, v in med.items()},
                          crops_per_frame={k: round(v / (args.frames * args.runs), 1) for k, v in seen.items()})), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--skip_rate", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch   # first: one HIP runtime for torch and the engine
    import caffe_rtpose_amd as r
    print(json.dumps(dict(library=r.LIB_PATH, device=torch.cuda.get_device_name(0), net=f"{NET_W}x{NET_H}", display=f"{W}x{H}")), flush=True)
    if not args.skip_kernel:
        kernel_legs(r, np, args)
    if not args.skip_rate:
        rate_legs(r, np, args)


if __name__ == "__main__":
    main()

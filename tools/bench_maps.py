#!/usr/bin/env python
"""Maps mode (maps_export.hip): what the kernel costs, what the payloads cost on PCIe, and what the mode does to the frame rate.

(a) The kernel alone at 656x368, 1 scale, for u8 parts+bkg (19 channels), f16 and f32 all channels (57), from HIP events on a stream
    of the caller: one frame is in flight and finished, rtp_peek_maps_device writes its maps into a dense device tensor over and over;
    the launches of a round are enqueued while the stream is held by a sleep kernel, so that they run back to back and the event pair
    brackets device work only.  The figure is a launch's period in a back-to-back train (kernel + the boundary to the next launch).
    Next to it: resize_kernel on all 57 channels (the materialised map of the parity taps, HIP events of rtp_last_stage_ms) followed
    by a separate conversion pass over the 55 MB map (torch: .half(), resp. mul / clamp / round / to(uint8)), i.e. what the same
    output costs without the fused epilogue.
(b) The D2H copy of each payload into pinned memory (HIP events around an async copy on an otherwise idle stream).
(c) One engine (656x368 net, 1280x720 host u8 frames, 7 in flight, batches of 2: bench.py's configuration) with maps off and in
    each of the three cases, alternated --runs times in one process: frames/s over --frames frames after a warm-up, each frame
    peeked (rtp_peek_maps into one reused host array) and collected; f32 also into a fresh array per frame and through
    rtp_peek_maps_device.
  python tools/bench_maps.py [--launches 200] [--rounds 10] [--frames 600] [--runs 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1280, 720
NET_W, NET_H = 656, 368
CASES = [("u8_parts_bkg", "u8", list(range(19))), ("f16_all", "f16", None), ("f32_all", "f32", None)]


def kernel_legs(r, torch, np, args):
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=2))
    frame = r.synth_frame(W, H, 1, seed=3)
    tdt = {"f32": torch.float32, "f16": torch.float16, "u8": torch.uint8}
    s = torch.cuda.Stream()
    out = []
    # resize_kernel on all channels: the resize stage of a materialised frame (event pair around the launch)
    x = r.preprocess_frame(frame, W, H, NET_W, NET_H)[0]
    ms = []
    for _ in range(12):
        e.forward_debug(x)
        ms.append(e.last_stage_ms()["resize"])
    resize_us = float(np.median(ms[2:])) * 1e3
    full = torch.zeros((e.heat_channels, NET_H, NET_W), dtype=torch.float32, device="cuda").uniform_(-1, 1)

    def torch_pass(fn):
        for _ in range(5):
            fn()
        us = []
        for _ in range(args.rounds):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(20):
                fn()
            ev1.record()
            ev1.synchronize()
            us.append(ev0.elapsed_time(ev1) * 1e3 / 20)
        return float(np.median(us))
    convert_us = {"f32": 0.0, "f16": torch_pass(lambda: full.half()),
                  "u8": torch_pass(lambda: (full[:19] * 255).clamp_(0, 255).round_().to(torch.uint8))}
    for name, fmt, ch in CASES:
        e.set_maps_output("net", fmt, ch)
        shape, dt, nbytes = e.maps_info()
        dst = torch.zeros(shape, dtype=tdt[fmt], device="cuda")
        e.submit_frame(frame, tag=1)
        _, host = e.peek_maps()
        for _ in range(20):
            e.peek_maps_device(dst, stream=s)
        s.synchronize()
        assert np.array_equal(dst.cpu().numpy().view(np.uint8), host.view(np.uint8)), name
        us, behind = [], True
        for _ in range(args.rounds):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                torch.cuda._sleep(60_000_000)   # holds the stream while the round is enqueued
                ev0.record()
            for _ in range(args.launches):
                e.peek_maps_device(dst, stream=s)
            behind = behind and not ev0.query()   # the sleep was still running when the last launch was enqueued
            ev1.record(s)
            ev1.synchronize()
            us.append(ev0.elapsed_time(ev1) * 1e3 / args.launches)
        e.collect()
        # the payload's D2H copy into pinned memory
        pinned = torch.empty(shape, dtype=tdt[fmt]).pin_memory()
        d2h = []
        for _ in range(args.rounds + 2):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                ev0.record()
                pinned.copy_(dst, non_blocking=True)
                ev1.record()
            ev1.synchronize()
            d2h.append(ev0.elapsed_time(ev1) * 1e3)
        med, d2h_med = float(np.median(us)), float(np.median(d2h[2:]))
        out.append(dict(case=name, channels=shape[1], payload_mb=round(nbytes / 1e6, 2), launches=args.launches * args.rounds, kernel_period_us_median=round(med, 1),
                        kernel_period_us_min=round(min(us), 1), kernel_period_us_max=round(max(us), 1), all_queued_behind_the_sleep=behind,
                        resize_kernel_57ch_us=round(resize_us, 1), separate_conversion_pass_us=round(convert_us[fmt], 1),
                        resize_then_convert_us=round(resize_us + convert_us[fmt], 1), d2h_us_median=round(d2h_med, 1), d2h_gb_per_s=round(nbytes / d2h_med / 1e3, 1)))
        print(json.dumps(out[-1]), flush=True)
    e.set_maps_output(None)
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


def rate_legs(r, torch, np, args):
    in_flight = 7
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=in_flight, batch_frames=2))
    frames = [r.synth_frame(W, H, i, seed=3) for i in range(8)]
    # how the caller takes the maps: "host" = rtp_peek_maps into ONE reused array, "host_fresh" = into a new array per frame (what
    # Engine.peek_maps() does by default: 55 MB of page faults per f32 frame), "device" = rtp_peek_maps_device into a dense device
    # tensor on a stream of the caller (the kernel runs a second time, nothing more crosses to the caller's side)
    cases = [("off", None, None, None)] + [(n, f, c, "host") for n, f, c in CASES] + [("f32_all_fresh_array", "f32", None, "host_fresh"), ("f32_all_device", "f32", None, "device")]
    tdt = {"f32": torch.float32, "f16": torch.float16, "u8": torch.uint8}
    side = torch.cuda.Stream()

    def set_case(fmt, ch, how):
        if fmt is None:
            e.set_maps_output(None)
            return lambda: None
        e.set_maps_output("net", fmt, ch)
        shape, dt, _ = e.maps_info()
        if how == "host":
            buf = np.zeros(shape, dt)
            return lambda: e.peek_maps(out=buf)
        if how == "host_fresh":
            return e.peek_maps
        dst = torch.zeros(shape, dtype=tdt[fmt], device="cuda")
        return lambda: e.peek_maps_device(dst, stream=side)
    out = []
    for name, fmt, ch, how in cases:   # warm-up of every case: buffers, code objects
        run_frames(e, frames, 100, in_flight, set_case(fmt, ch, how))
    for run in range(args.runs):
        for name, fmt, ch, how in cases:
            fps = run_frames(e, frames, args.frames, in_flight, set_case(fmt, ch, how))
            out.append(dict(case=name, run=run, frames=args.frames, frames_per_s=round(fps, 1)))
            print(json.dumps(out[-1]), flush=True)
    e.set_maps_output(None)
    e.close()
    med = {c[0]: float(np.median([o["frames_per_s"] for o in out if o["case"] == c[0]])) for c in cases}
    print(json.dumps(dict(frames_per_s_median={k: round(v, 1) for k, v in med.items()},
                          relative_to_off={k: round(v / med["off"], 3) for k, v in med.items()})), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--skip_rate", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch   # first: one HIP runtime for torch and the engine
    import caffe_rtpose_amd as r
    print(json.dumps(dict(library=r.LIB_PATH, device=torch.cuda.get_device_name(0), net=f"{NET_W}x{NET_H}", num_scales=1)), flush=True)
    if not args.skip_kernel:
        kernel_legs(r, torch, np, args)
    if not args.skip_rate:
        rate_legs(r, torch, np, args)


if __name__ == "__main__":
    main()

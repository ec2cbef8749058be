#!/usr/bin/env python
"""Smoothing mode (smooth.hip): what the kernel costs, and what the mode does to the frame rate.

(a) The kernel alone, in its two builds (one workgroup of 256 or of 1024 threads; rtp_internal_smooth_variant), the engine's default
    marked (rtp_internal_smooth_time: the launches of a round are enqueued behind a wave that holds the stream, so that they run back
    to back and the event pair brackets device work only; the figure is a launch's period in the train = kernel + the boundary to
    the next launch) for 1, 8 and 96 tracked people, every part measured in every launch (the FILTER step, the most arithmetic).
    The track and smooth kernels of consecutive frames are chained, so 1 / (track period + smooth period) bounds the engine's frame
    rate; the smooth kernel's own bound is printed next to each figure.
(b) One engine (656x368 net, 1280x720 host u8 frames, 7 in flight, batches of 2: bench.py's configuration) with tracking alone and
    with smoothing (apply 0) on top, alternated --runs times in one process: frames/s over --frames frames after a warm-up, each
    frame peeked and collected.
(c) The same on a rendering engine with crops mode on (16 crops of 128x128), tracking alone against smoothing with
    apply = RENDER | CROPS: there the render stage and the crops kernel wait behind the smooth kernel, i.e. behind the previous
    frame's chain.
  python tools/bench_smooth.py [--launches 200] [--rounds 7] [--frames 600] [--runs 3]
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
VARIANTS = [("wg256", 0), ("wg1024", 1)]   # kernels.h RTP_SMOOTH_*


def people(np, n, num_parts, dx=0.0):
    """n people of 60 x 120 pixels on a grid, every part scored"""
    j = np.zeros((n, num_parts, 3), np.float32)
    for k in range(n):
        for p in range(num_parts):
            j[k, p] = (20 + 100 * (k % 12) + 15 * (p % 5) + dx, 10 + 85 * (k // 12) + 30 * (p // 5), 0.9)
    return j


def set_variant(e, v):
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_smooth_variant
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    before = fn(e.h, v)
    assert before >= 0
    return before


def kernel_legs(r, np, args):
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_smooth_time
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, _lib.fp, _lib.ip, C.c_int, C.c_int, C.POINTER(C.c_float)]
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=2))
    out = []
    e.set_tracking()
    default = set_variant(e, 0)
    for n, (vname, v) in [(n, w) for n in (1, 8, 96) for w in VARIANTS]:
        set_variant(e, v)
        e.set_smoothing(None)
        e.track_reset()
        e.set_smoothing()
        j = people(np, n, e.num_parts)
        ts, st = r.TrackState(e.num_parts), r.SmoothState(e.num_parts)
        for dx in (0.0, 1.0):   # born, then matched: every part is filtered from here on
            recs = r.track_update(ts, j + np.float32(dx))
            want = r.smooth_update(st, j + np.float32(dx), None, recs)
            got = e.smooth_from_joints(j + np.float32(dx))
            assert np.array_equal(got[0], recs) and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(want, got[1:])) and e.smooth_state() == st
        assert (want[2] == 2).all()
        us = []
        for _ in range(args.rounds):
            p = C.c_float()
            e._chk(fn(e.h, j.ctypes.data_as(_lib.fp), recs.ctypes.data_as(_lib.ip), n, args.launches, C.byref(p)))
            us.append(p.value)
        assert e.smooth_state() == st, "the timing entry restores the table"
        med = float(np.median(us))
        out.append(dict(variant=vname, default=v == default, people=n, items=n * e.num_parts, launches=args.launches * args.rounds, kernel_period_us_median=round(med, 1),
                        kernel_period_us_min=round(min(us), 1), kernel_period_us_max=round(max(us), 1), frames_per_s_bound=round(1e6 / med)))
        print(json.dumps(out[-1]), flush=True)
    set_variant(e, default)
    e.set_smoothing(None)
    e.set_tracking(None)
    e.close()
    return out


def run_frames(e, frames, n, in_flight, peek, collect):
    t = time.perf_counter()
    for i in range(n):
        if e.in_flight() >= in_flight:
            peek()
            collect()
        e.submit_frame(frames[i % len(frames)], tag=i)
    while e.in_flight():
        peek()
        collect()
    return n / (time.perf_counter() - t)


def rate_legs(r, np, args, render):
    in_flight = 7
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=in_flight, batch_frames=2, render=1 if render else 0))
    frames = [r.synth_frame(W, H, i, seed=3) for i in range(8)]
    seen = {"people": 0, "filtered": 0, "held": 0, "frames": 0}
    apply = (r.SMOOTH_RENDER | r.SMOOTH_CROPS) if render else 0
    if render:
        e.set_crops_output(128, 128, 16, margin=0.15)
    collect = e.collect_rendered if render else e.collect

    def set_case(on):
        e.set_smoothing(None)
        e.set_tracking(None)
        e.set_tracking()
        if not on:
            return lambda: (e.peek_tracks(), e.peek_crops() if render else None)
        e.set_smoothing(apply=apply)

        def peek():
            e.peek_tracks()
            if render:
                e.peek_crops()
            _, js, _, flags = e.peek_smoothed()
            seen["people"] += len(js)
            seen["filtered"] += int((flags == 2).sum())
            seen["held"] += int((flags == 3).sum())
            seen["frames"] += 1
        return peek
    names = ("tracking", "tracking+smoothing" + ("(render|crops)" if render else "(apply 0)"))
    out = []
    for on in (False, True):   # warm-up of both cases: buffers, code objects
        run_frames(e, frames, 100, in_flight, set_case(on), collect)
    for k in seen:
        seen[k] = 0
    for run in range(args.runs):
        for name, on in zip(names, (False, True)):
            fps = run_frames(e, frames, args.frames, in_flight, set_case(on), collect)
            out.append(dict(engine="render+crops" if render else "plain", case=name, run=run, frames=args.frames, frames_per_s=round(fps, 1)))
            print(json.dumps(out[-1]), flush=True)
    e.set_smoothing(None)
    e.set_tracking(None)
    e.close()
    med = {c: float(np.median([o["frames_per_s"] for o in out if o["case"] == c])) for c in names}
    spread = {c: round(max(o["frames_per_s"] for o in out if o["case"] == c) - min(o["frames_per_s"] for o in out if o["case"] == c), 1) for c in names}
    print(json.dumps(dict(engine="render+crops" if render else "plain", frames_per_s_median={k: round(v, 1) for k, v in med.items()}, spread_of_runs=spread,
                          relative_to_tracking=round(med[names[1]] / med[names[0]], 3),
                          per_frame={k: round(v / max(seen["frames"], 1), 1) for k, v in seen.items() if k != "frames"})), flush=True)
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
        rate_legs(r, np, args, render=False)
        rate_legs(r, np, args, render=True)


if __name__ == "__main__":
    main()

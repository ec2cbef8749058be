#!/usr/bin/env python
"""Tracking mode (track.hip): what the kernel costs, and what the mode does to the frame rate.

(a) The kernel alone, in its four builds (the assignment as argmin rounds or as one LDS sort with a one-thread walk, 256 or 1024
    threads; rtp_internal_track_variant), the engine's default marked (rtp_internal_track_time: the launches of a round are enqueued behind a wave that holds the stream, so that they
    run back to back and the event pair brackets device work only; the figure is a launch's period in the train = kernel + the
    boundary to the next launch) for 1, 8 and 96 people against an equally full table (every person matches its own track at
    cost 0: as many assignment rounds as people), for 96 people against 128 live tracks (the most pairs: 12288), and "dense": 8
    and 96 people an eighth of a pixel apart, where EVERY pair is a candidate (the most the sort and the walk can meet).  The track
    kernels of consecutive frames are chained, so 1 / period bounds the engine's frame rate: the bound is printed next to each figure.
(b) One engine (656x368 net, 1280x720 host u8 frames, 7 in flight, batches of 2: bench.py's configuration) with the mode off and
    on, alternated --runs times in one process: frames/s over --frames frames after a warm-up, each frame peeked (rtp_peek_tracks)
    and collected.
  python tools/bench_track.py [--launches 200] [--rounds 7] [--frames 600] [--runs 3]
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


def people(np, n, num_parts, dx=0.0):
    """n people of 60 x 120 pixels on a grid, every part scored"""
    j = np.zeros((n, num_parts, 3), np.float32)
    for k in range(n):
        for p in range(num_parts):
            j[k, p] = (20 + 100 * (k % 12) + 15 * (p % 5) + dx, 10 + 85 * (k // 12) + 30 * (p // 5), 0.9)
    return j


VARIANTS = [("argmin256", 0), ("argmin1024", 1), ("sort256", 2), ("sort1024", 3)]   # kernels.h RTP_TRACK_*


def set_variant(e, v):
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_track_variant
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    before = fn(e.h, v)
    assert before >= 0
    return before


def dense(np, n, num_parts):
    """n people an eighth of a pixel apart: every (track, person) pair is a candidate"""
    j = people(np, 1, num_parts).repeat(n, 0)
    for k in range(n):
        j[k, :, 0] += 0.125 * (k % 12)
        j[k, :, 1] += 0.125 * (k // 12)
    return j


def kernel_legs(r, np, args):
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_track_time
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, _lib.fp, C.c_int, C.c_int, C.POINTER(C.c_float)]
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=2))
    cfg = r.track_config(max_misses=1 << 30)   # (the 32 unmatched tracks of the 96 / 128 case must outlive the trains)
    out = []
    default = set_variant(e, 0)
    for (n, tracks, kind), (vname, v) in [(c, w) for c in ((1, 1, "apart"), (8, 8, "apart"), (96, 96, "apart"), (96, 128, "apart"), (8, 8, "dense"), (96, 96, "dense"))
                                          for w in VARIANTS]:
        set_variant(e, v)
        e.set_tracking(None)
        e.set_tracking(cfg)
        j = people(np, n, e.num_parts) if kind == "apart" else dense(np, n, e.num_parts)
        st = r.TrackState(e.num_parts)
        if tracks > n:    # 32 more live tracks far away from everybody
            extra = people(np, tracks - n, e.num_parts, dx=5000.0)
            assert len(r.track_update(st, extra, cfg=cfg)) == tracks - n
            e.track_from_joints(extra)
        want = r.track_update(st, j, cfg=cfg)
        assert np.array_equal(e.track_from_joints(j), want) and e.track_state() == st and len(st.live()) == tracks
        assert np.array_equal(e.track_from_joints(j), r.track_update(st, j, cfg=cfg)) and e.track_state() == st   # everybody matches
        us = []
        for _ in range(args.rounds):
            p = C.c_float()
            e._chk(fn(e.h, j.ctypes.data_as(_lib.fp), n, args.launches, C.byref(p)))
            us.append(p.value)
        assert e.track_state() == st, "the timing entry restores the table"
        med = float(np.median(us))
        out.append(dict(variant=vname, default=v == default, people=n, live_tracks=tracks, pairs=n * tracks, candidates=n if kind == "apart" else n * tracks, launches=args.launches * args.rounds, kernel_period_us_median=round(med, 1),
                        kernel_period_us_min=round(min(us), 1), kernel_period_us_max=round(max(us), 1), frames_per_s_bound=round(1e6 / med)))
        print(json.dumps(out[-1]), flush=True)
    set_variant(e, default)
    e.set_tracking(None)
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
    in_flight = 7
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=in_flight, batch_frames=2))
    frames = [r.synth_frame(W, H, i, seed=3) for i in range(8)]
    seen = {"people": 0, "tracked": 0, "matched": 0, "frames": 0}

    def set_case(on):
        e.set_tracking(None)
        if not on:
            return lambda: None
        e.set_tracking()

        def peek():
            _, recs = e.peek_tracks()
            seen["people"] += len(recs)
            seen["tracked"] += int((recs[:, 0] != 0).sum())
            seen["matched"] += int((recs[:, 2] >= 2).sum())
            seen["frames"] += 1
        return peek
    out = []
    for on in (False, True):   # warm-up of both cases: buffers, code objects
        run_frames(e, frames, 100, in_flight, set_case(on))
    for k in seen:
        seen[k] = 0
    for run in range(args.runs):
        for name, on in (("off", False), ("tracking", True)):
            fps = run_frames(e, frames, args.frames, in_flight, set_case(on))
            out.append(dict(case=name, run=run, frames=args.frames, frames_per_s=round(fps, 1)))
            print(json.dumps(out[-1]), flush=True)
    e.set_tracking(None)
    e.close()
    med = {c: float(np.median([o["frames_per_s"] for o in out if o["case"] == c])) for c in ("off", "tracking")}
    print(json.dumps(dict(frames_per_s_median={k: round(v, 1) for k, v in med.items()}, relative_to_off=round(med["tracking"] / med["off"], 3),
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
        rate_legs(r, np, args)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Overlay mode (overlay.hip): what its two kernels cost, and what the mode does to the frame rate.

(a) The kernels alone (rtp_internal_overlay_time: the launches of a round are enqueued behind a wave that holds the stream, so that
    they run back to back and the event pair brackets device work only; the figure is a launch's period in the train = kernel + the
    boundary to the next launch) at 1280x720 for 1, 8 and 96 tracked people with trail_len 0 and 32.  The trails are full: the people
    walk for 33 frames through the parity tap first, which is checked against the host definition on the way.  The update kernels of
    consecutive frames are chained with the track kernels; the draw kernel is not.
(b) One rendering engine (656x368 net, 1280x720 host u8 frames, 7 in flight, batches of 2: bench.py's configuration with render = 1)
    with tracking alone and with the overlay on top, alternated --runs times in one process: frames/s over --frames frames after a
    warm-up, each frame peeked and collected.  The mode's cost includes the copy of the list buffer (114 KB) to pinned memory.
  python tools/bench_overlay.py [--launches 200] [--rounds 7] [--frames 600] [--runs 3]
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


def kernel_legs(r, np, args):
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_overlay_time
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, _lib.fp, _lib.ip, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), _lib.ip]
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=2, render=1))
    out = []
    e.set_tracking()
    bg = r.synth_frame(W, H, 0, seed=3)
    for n, trail_len in [(n, t) for n in (1, 8, 96) for t in (0, 32)]:
        ocfg = r.overlay_config(trail_len=trail_len)
        e.set_track_overlay(None)
        e.track_reset()
        e.set_track_overlay(ocfg)
        ts, st = r.TrackState(e.num_parts), r.TrailState(e.num_parts)
        for i in range(33):   # born, then matched: the rings fill
            j = people(np, n, e.num_parts, 2.0 * i)
            recs = r.track_update(ts, j)
            want = r.overlay_update(st, j, None, recs, ocfg)
            got_recs, got, img = e.overlay_from_joints(j, image=bg if i == 32 else None)
            assert np.array_equal(got_recs, recs) and np.array_equal(got, want)
        assert e.overlay_state() == st and np.array_equal(img, r.overlay_draw(want, bg.copy()))
        assert len(want) == n * (max(trail_len - 1, 0) + 2)
        for draw, kernel in ((0, "update"), (1, "draw")):
            us, m = [], C.c_int()
            for _ in range(args.rounds):
                p = C.c_float()
                e._chk(fn(e.h, j.ctypes.data_as(_lib.fp), recs.ctypes.data_as(_lib.ip), n, draw, args.launches, C.byref(p), C.byref(m)))
                us.append(p.value)
            assert e.overlay_state() == st, "the timing entry restores the table"
            med = float(np.median(us))
            out.append(dict(kernel=kernel, people=n, trail_len=trail_len, items=m.value, image=f"{W}x{H}", launches=args.launches * args.rounds,
                            kernel_period_us_median=round(med, 1), kernel_period_us_min=round(min(us), 1), kernel_period_us_max=round(max(us), 1)))
            print(json.dumps(out[-1]), flush=True)
    e.set_track_overlay(None)
    e.set_tracking(None)
    e.close()
    return out


def run_frames(e, frames, n, in_flight, peek):
    t = time.perf_counter()
    for i in range(n):
        if e.in_flight() >= in_flight:
            peek()
            e.collect_rendered()
        e.submit_frame(frames[i % len(frames)], tag=i)
    while e.in_flight():
        peek()
        e.collect_rendered()
    return n / (time.perf_counter() - t)


def rate_legs(r, np, args):
    in_flight = 7
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=in_flight, batch_frames=2, render=1))
    frames = [r.synth_frame(W, H, i, seed=3) for i in range(8)]
    seen = {"items": 0, "frames": 0}

    def set_case(on):
        e.set_track_overlay(None)
        e.set_tracking(None)
        e.set_tracking()
        if not on:
            return e.peek_tracks
        e.set_track_overlay()

        def peek():
            e.peek_tracks()
            seen["items"] += len(e.peek_overlay_items()[1])
            seen["frames"] += 1
        return peek
    names = ("tracking", "tracking+overlay")
    out = []
    for on in (False, True):   # warm-up of both cases: buffers, code objects
        run_frames(e, frames, 100, in_flight, set_case(on))
    seen["items"] = seen["frames"] = 0
    for run in range(args.runs):
        for name, on in zip(names, (False, True)):
            fps = run_frames(e, frames, args.frames, in_flight, set_case(on))
            out.append(dict(engine="render", case=name, run=run, frames=args.frames, frames_per_s=round(fps, 1)))
            print(json.dumps(out[-1]), flush=True)
    e.set_track_overlay(None)
    e.set_tracking(None)
    e.close()
    med = {c: float(np.median([o["frames_per_s"] for o in out if o["case"] == c])) for c in names}
    spread = {c: round(max(o["frames_per_s"] for o in out if o["case"] == c) - min(o["frames_per_s"] for o in out if o["case"] == c), 1) for c in names}
    print(json.dumps(dict(engine="render", frames_per_s_median={k: round(v, 1) for k, v in med.items()}, spread_of_runs=spread,
                          relative_to_tracking=round(med[names[1]] / med[names[0]], 3), items_per_frame=round(seen["items"] / max(seen["frames"], 1), 1))), flush=True)
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

#!/usr/bin/env python
"""Appearance-aided tracking (appearance.hip, track.hip's appearance form): what the kernels cost, and what the mode does to the frame rate.

(a) appear_describe alone (rtp_internal_appearance_time: a train of launches behind a wave that holds the stream; the figure is a
    launch's period in the train) for 1, 8 and 96 people on a 1280x720 display image.
(b) The track kernel without and with the appearance path in its four builds (rtp_internal_track_variant, rtp_internal_track_time),
    for the cases of tools/bench_track.py: 1, 8 and 96 people against an equally full table, 96 people against 128 live tracks, and
    the all-candidates cases of 8 and 96 people an eighth of a pixel apart.  With the mode on every track has a descriptor and every
    person a valid one, so every pair that passes the motion gate takes the 128-bin distance.  Table and descriptors are read through
    L2; a build that stages the descriptors in LDS does not exist, so there is nothing to compare it with.
(c) One engine (656x368 net, 1280x720 host u8 frames, 7 in flight, batches of 2: bench.py's configuration) with tracking alone and
    with the mode on (all parts listed, so that the noise maps' people have descriptors), alternated --runs times in one process:
    frames/s over --frames frames after a warm-up, each frame peeked and collected.
  python tools/bench_appearance.py [--launches 200] [--rounds 7] [--frames 600] [--runs 4]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_track as bt   # noqa: E402  (the people, the variants and the frame loop of the tracking benchmark)

W, H = bt.W, bt.H


def describe_legs(r, np, args, e):
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_appearance_time
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_ubyte), _lib.fp, C.c_int, C.c_int, C.POINTER(C.c_float)]
    img = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    acfg = r.appearance_config(parts=list(range(e.num_parts)))
    e.set_tracking()
    e.set_track_appearance(acfg)
    for n in (1, 8, 96):
        j = bt.people(np, n, e.num_parts)
        got, want = e.appearance_from_joints(img, j), r.appearance_describe(img, j, e.num_parts, acfg)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[1].all()
        us = []
        for _ in range(args.rounds):
            p = C.c_float()
            e._chk(fn(e.h, img.ctypes.data_as(C.POINTER(C.c_ubyte)), j.ctypes.data_as(_lib.fp), n, args.launches, C.byref(p)))
            us.append(p.value)
        print(json.dumps(dict(kernel="appear_describe", people=n, launches=args.launches * args.rounds, period_us_median=round(float(np.median(us)), 1),
                              period_us_min=round(min(us), 1), period_us_max=round(max(us), 1))), flush=True)
    e.set_track_appearance(None)
    e.set_tracking(None)


def track_legs(r, np, args, e):
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_track_time
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, _lib.fp, C.c_int, C.c_int, C.POINTER(C.c_float)]
    img = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    tcfg = r.track_config(max_misses=1 << 30)
    acfg = r.appearance_config(parts=list(range(e.num_parts)))
    default = bt.set_variant(e, 0)
    for (n, tracks, kind), (vname, v), appear in [(c, w, a) for c in ((1, 1, "apart"), (8, 8, "apart"), (96, 96, "apart"), (96, 128, "apart"), (8, 8, "dense"), (96, 96, "dense"))
                                                  for w in bt.VARIANTS for a in (False, True)]:
        bt.set_variant(e, v)
        e.set_track_appearance(None)
        e.set_tracking(None)
        e.set_tracking(tcfg)
        if appear:
            e.set_track_appearance(acfg)
        j = bt.people(np, n, e.num_parts) if kind == "apart" else bt.dense(np, n, e.num_parts)
        step = (lambda x: e.track_from_frame(img, x)[0]) if appear else e.track_from_joints
        if tracks > n:    # 32 more live tracks far away from everybody
            step(bt.people(np, tracks - n, e.num_parts, dx=5000.0))
        step(j)
        recs = step(j)   # everybody matches; in appearance mode slot 0 now holds the frame's descriptors for the train
        assert (recs[:, 2] >= 2).all() and len(e.track_state().live()) == tracks
        if appear:
            assert (e.appearance_state().owner == e.track_state().id).all()
        before = e.track_state()
        us = []
        for _ in range(args.rounds):
            p = C.c_float()
            e._chk(fn(e.h, j.ctypes.data_as(_lib.fp), n, args.launches, C.byref(p)))
            us.append(p.value)
        assert e.track_state() == before, "the timing entry restores the table"
        print(json.dumps(dict(kernel="track", appearance=appear, variant=vname, default=v == default, people=n, live_tracks=tracks,
                              candidates=n if kind == "apart" else n * tracks, launches=args.launches * args.rounds, period_us_median=round(float(np.median(us)), 1),
                              period_us_min=round(min(us), 1), period_us_max=round(max(us), 1))), flush=True)
    bt.set_variant(e, default)
    e.set_track_appearance(None)
    e.set_tracking(None)


def rate_legs(r, np, args):
    in_flight = 7
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=in_flight, batch_frames=2))
    frames = [r.synth_frame(W, H, i, seed=3) for i in range(8)]
    seen = {"people": 0, "matched": 0, "valid": 0, "frames": 0}

    def set_case(appear):
        e.set_track_appearance(None)
        e.set_tracking(None)
        e.set_tracking()
        if appear:
            e.set_track_appearance(r.appearance_config(parts=list(range(e.num_parts)), min_parts=2))

        def peek():
            _, recs = e.peek_tracks()
            if appear:
                _, _, valid = e.peek_appearance()
                seen["people"] += len(recs)
                seen["matched"] += int((recs[:, 2] >= 2).sum())
                seen["valid"] += int(valid.sum())
                seen["frames"] += 1
        return peek
    out = []
    for appear in (False, True):   # warm-up of both cases: buffers, code objects
        bt.run_frames(e, frames, 100, in_flight, set_case(appear))
    for k in seen:
        seen[k] = 0
    for run in range(args.runs):
        for name, appear in (("tracking", False), ("appearance", True)):
            fps = bt.run_frames(e, frames, args.frames, in_flight, set_case(appear))
            out.append(dict(case=name, run=run, frames=args.frames, frames_per_s=round(fps, 1)))
            print(json.dumps(out[-1]), flush=True)
    e.set_track_appearance(None)
    e.set_tracking(None)
    e.close()
    runs = {c: [o["frames_per_s"] for o in out if o["case"] == c] for c in ("tracking", "appearance")}
    print(json.dumps(dict(frames_per_s_median={k: round(float(np.median(v)), 1) for k, v in runs.items()}, spread={k: round(max(v) - min(v), 1) for k, v in runs.items()},
                          relative_to_tracking=round(float(np.median(runs["appearance"]) / np.median(runs["tracking"])), 3),
                          per_frame={k: round(v / max(seen["frames"], 1), 1) for k, v in seen.items() if k != "frames"})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--skip_rate", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch   # first: one HIP runtime for torch and the engine
    import caffe_rtpose_amd as r
    print(json.dumps(dict(library=r.LIB_PATH, device=torch.cuda.get_device_name(0), net=f"{bt.NET_W}x{bt.NET_H}", display=f"{W}x{H}")), flush=True)
    if not args.skip_kernel:
        e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=2))
        describe_legs(r, np, args, e)
        track_legs(r, np, args, e)
        e.close()
    if not args.skip_rate:
        rate_legs(r, np, args)


if __name__ == "__main__":
    main()

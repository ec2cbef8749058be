#!/usr/bin/env python
"""Redaction mode (redact.hip): what its kernels cost, and what the mode does to the frame rate.

(a) The kernels alone (rtp_internal_redact_time: the launches of a round are enqueued behind a wave that holds the stream, so that
    they run back to back and the event pair brackets device work only; the figure is one application's period in the train = kernel +
    the boundary to the next launch; the blur's figure holds BOTH its launches) at 1280x720 for 1, 8 and 96 people, per effect: mosaic
    at cell 8 and 32, blur at radius 4 and 16, fill; with head-sized regions (the head parts, rx about 20) and with body-sized ones
    (every part listed).  The parity tap is checked against the host definition on the way.  The regions kernel is timed once per
    people count.
(b) One rendering engine (656x368 net, 1280x720 host u8 frames, 7 in flight, batches of 2: bench.py's configuration with render = 1)
    with the mode off and on (the default mosaic, and the blur at radius 8, every part listed so that the noise maps' people have
    regions), alternated --runs times in one process: frames/s over --frames frames after a warm-up, each frame peeked and collected.
  python tools/bench_redact.py [--launches 200] [--rounds 7] [--frames 600] [--runs 4]
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
EFFECTS = [("mosaic_cell8", dict(effect=0, cell=8)), ("mosaic_cell32", dict(effect=0, cell=32)), ("blur_radius4", dict(effect=1, radius=4)),
           ("blur_radius16", dict(effect=1, radius=16)), ("fill", dict(effect=2, colour=0x202020))]


def people(np, n, num_parts):
    """n people of 60 x 120 pixels on a grid, every part scored; the head parts of either model span 26 pixels: rx = 21"""
    j = np.zeros((n, num_parts, 3), np.float32)
    for k in range(n):
        x, y = 20 + 100 * (k % 12), 10 + 85 * (k // 12)
        for p in range(num_parts):
            j[k, p] = (x + 15 * (p % 5), y + 30 * (p // 5), 0.9)
        if num_parts == 18:
            for p, (dx, dy) in {0: (30, 12), 14: (24, 6), 15: (36, 6), 16: (17, 12), 17: (43, 12)}.items():
                j[k, p, :2] = (x + dx, y + dy)
        else:
            j[k, 0, :2], j[k, 1, :2] = (x + 30, y), (x + 30, y + 26)
    return j


def kernel_legs(r, np, args):
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_redact_time
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, _lib.fp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), _lib.ip]
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=2, render=1))
    bg = r.synth_frame(W, H, 0, seed=3)
    out = []

    def timed(j, n, regions):
        us, m = [], C.c_int()
        for _ in range(args.rounds):
            p = C.c_float()
            e._chk(fn(e.h, j.ctypes.data_as(_lib.fp), n, regions, args.launches, C.byref(p), C.byref(m)))
            us.append(p.value)
        return dict(valid_regions=m.value, launches=args.launches * args.rounds, kernel_period_us_median=round(float(np.median(us)), 1), kernel_period_us_min=round(min(us), 1),
                    kernel_period_us_max=round(max(us), 1))
    for n in (1, 8, 96):
        j = people(np, n, e.num_parts)
        for size, parts in (("head", None), ("body", list(range(e.num_parts)))):
            for name, eff in EFFECTS:
                cfg = r.redact_config(parts=parts, **eff)
                e.set_redaction(cfg)
                want = r.redact_regions(j, e.num_parts, cfg=cfg)
                got, img = e.redact_from_joints(j, image=bg)
                assert np.array_equal(got, want) and np.array_equal(img, r.redact_apply(want, bg.copy(), cfg)), (n, size, name)
                out.append(dict(kernel="apply", effect=name, regions=size, rx=int(want[0, 2]), ry=int(want[0, 3]), people=n, image=f"{W}x{H}", **timed(j, n, 0)))
                print(json.dumps(out[-1]), flush=True)
        out.append(dict(kernel="regions", people=n, **timed(j, n, 1)))
        print(json.dumps(out[-1]), flush=True)
    e.set_redaction(None)
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
    seen = {}
    cases = {"off": None, "mosaic": r.redact_config(parts=list(range(e.num_parts))), "blur_radius8": r.redact_config(parts=list(range(e.num_parts)), effect=1, radius=8)}

    def set_case(name):
        e.set_redaction(cases[name])
        if cases[name] is None:
            return lambda: None
        s = seen.setdefault(name, {"valid": 0, "frames": 0})

        def peek():
            regs = e.peek_redactions()[1]
            s["valid"] += int(regs[:, 5].sum()) if len(regs) else 0
            s["frames"] += 1
        return peek
    out = []
    for name in cases:   # warm-up of every case: buffers, code objects
        run_frames(e, frames, 100, in_flight, set_case(name))
    seen.clear()
    for run in range(args.runs):
        for name in cases:
            fps = run_frames(e, frames, args.frames, in_flight, set_case(name))
            out.append(dict(engine="render", case=name, run=run, frames=args.frames, frames_per_s=round(fps, 1)))
            print(json.dumps(out[-1]), flush=True)
    e.set_redaction(None)
    e.close()
    med = {c: float(np.median([o["frames_per_s"] for o in out if o["case"] == c])) for c in cases}
    spread = {c: round(max(o["frames_per_s"] for o in out if o["case"] == c) - min(o["frames_per_s"] for o in out if o["case"] == c), 1) for c in cases}
    print(json.dumps(dict(engine="render", frames_per_s_median={k: round(v, 1) for k, v in med.items()}, spread_of_runs=spread,
                          relative_to_off={c: round(med[c] / med["off"], 3) for c in cases if c != "off"},
                          valid_regions_per_frame={c: round(s["valid"] / max(s["frames"], 1), 1) for c, s in seen.items()})), flush=True)
    return out


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
    print(json.dumps(dict(library=r.LIB_PATH, device=torch.cuda.get_device_name(0), net=f"{NET_W}x{NET_H}", display=f"{W}x{H}")), flush=True)
    if not args.skip_kernel:
        kernel_legs(r, np, args)
    if not args.skip_rate:
        rate_legs(r, np, args)


if __name__ == "__main__":
    main()

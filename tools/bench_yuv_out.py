#!/usr/bin/env python
"""YUV output (yuv_export.hip): what the conversion kernel costs, and what the YUV mode of the renderer does to the frame rate.

(a) The conversion alone at 1280x720 (2.76 MB read, 1.38 MB written per 4:2:0 frame) and at 3840x2160, for the 4 x 2 kernel (planar
    and NV12 planes) and the generic kernel (the same planes one byte off their alignment; a BGRA source), from HIP events on a stream
    of the caller:
    the launches of a round are enqueued while the stream is held by a sleep kernel, so that they run back to back and the event pair
    brackets device work only (a Python Engine.convert_to_yuv_device call costs the host more than the kernel runs); --rounds rounds of
    --launches launches each, the median round.  The figure is a launch's period in a back-to-back train (kernel + the boundary to
    the next launch); bytes / period is therefore a LOWER bound of the kernel's streaming rate.
(b) One engine with render = 1 (656x368 net, 1280x720 host u8 frames, 7 in flight, batches of 2: bench.py's configuration) in raw
    mode (rtp_collect_rendered: 3 bytes per pixel to the host), YUV mode (rtp_collect_rendered_yuv: 1.5) and JPEG mode
    (rtp_collect_rendered_jpeg, quality 98), alternated --runs times in one process: frames/s over --frames frames after a warm-up,
    and in YUV mode the kernel's residency per frame from the stamp probe (slot 64 + 8 j + 7: first workgroup start to last
    workgroup end) in a run of its own.
  python tools/bench_yuv_out.py [--launches 400] [--rounds 10] [--frames 600] [--runs 3] [--modes raw,yuv,jpeg]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1280, 720
FRAME_BYTES = W * H * 3 + W * H * 3 // 2   # read + written per 4:2:0 frame
HBM_BYTES_PER_S = 6.29e12                  # measured float4 copy rate of the chip (MI355X: 8.0 TB/s peak)


def kernel_legs(r, torch, np, args, e, W, H):
    frame_bytes = W * H * 3 + W * H * 3 // 2
    img = r.synth_frame(W, H, 1, seed=3)
    src = torch.from_numpy(img).cuda()
    bgra = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    bgra[..., :3] = src

    def planes(layout, off):
        """planes inside wider tensors: off = 0 keeps every pitch and pointer aligned, off = 1 starts every plane one byte later"""
        y = torch.zeros((H, W + 64), dtype=torch.uint8, device="cuda")[:, off:off + W]
        if layout == "planar":
            return (y,) + tuple(torch.zeros((H // 2, W // 2 + 32), dtype=torch.uint8, device="cuda")[:, off:off + W // 2] for _ in range(2))
        return y, torch.zeros((H // 2, W // 2 + 32, 2), dtype=torch.uint8, device="cuda")[:, off:off + W // 2], None

    cases = [("block_4x2_planar", src, planes("planar", 0)), ("block_4x2_nv12", src, planes("nv12", 0)),
             ("generic_planar_unaligned", src, planes("planar", 1)), ("generic_nv12_bgra_source", bgra[..., :3], planes("nv12", 0))]
    if (W, H) != (1280, 720):
        cases = [cases[0], cases[2]]
    want = r.convert_bgr_to_yuv(img)
    s = torch.cuda.Stream()
    out = []
    for name, frame, dst in cases:
        for _ in range(50):
            e.convert_to_yuv_device(frame, *dst, stream=s)
        s.synchronize()
        got = [p.cpu().numpy() for p in dst if p is not None]
        if len(got) == 2:
            got = [got[0], got[1][..., 0], got[1][..., 1]]
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), name
        us, behind = [], True
        for _ in range(args.rounds):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                torch.cuda._sleep(60_000_000)   # holds the stream while the round is enqueued
                ev0.record()
            for _ in range(args.launches):
                e.convert_to_yuv_device(frame, *dst, stream=s)
            behind = behind and not ev0.query()   # the sleep was still running when the last launch was enqueued
            ev1.record(s)
            ev1.synchronize()
            us.append(ev0.elapsed_time(ev1) * 1e3 / args.launches)
        med = float(np.median(us))
        out.append(dict(kernel=name, size=f"{W}x{H}", mb_per_frame=round(frame_bytes / 1e6, 2), launches=args.launches * args.rounds,
                        period_us_median=round(med, 2), period_us_min=round(min(us), 2), period_us_max=round(max(us), 2), all_queued_behind_the_sleep=behind, gb_per_s_at_median=round(frame_bytes / med / 1e3, 1),
                        share_of_hbm_rate=round(frame_bytes / (med * 1e-6) / HBM_BYTES_PER_S, 3)))
        print(json.dumps(out[-1]), flush=True)
    return out


def set_mode(e, mode):
    """raw, yuv or jpeg; a library without the YUV mode (an older build under RTP_LIB / an older tree) runs raw and jpeg only"""
    if hasattr(e, "set_render_yuv"):
        e.set_render_yuv(0)
    e.set_render_jpeg(0)
    if mode == "yuv":
        e.set_render_yuv(420)
    elif mode == "jpeg":
        e.set_render_jpeg(98)
    return {"raw": e.collect_rendered, "jpeg": e.collect_rendered_jpeg, "yuv": getattr(e, "collect_rendered_yuv", None)}[mode]


def run_frames(e, collect, frames, n, in_flight):
    t = time.perf_counter()
    for i in range(n):
        if e.in_flight() >= in_flight:
            collect()
        e.submit_frame(frames[i % len(frames)], tag=i)
    while e.in_flight():
        collect()
    return n / (time.perf_counter() - t)


def mode_legs(r, np, args, modes):
    in_flight = 7
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=in_flight, batch_frames=2, render=1))
    frames = [r.synth_frame(W, H, i, seed=3) for i in range(8)]
    out = []
    for mode in modes:
        run_frames(e, set_mode(e, mode), frames, 100, in_flight)   # warm-up of every mode: buffers, code objects
    for run in range(args.runs):
        for mode in modes:
            fps = run_frames(e, set_mode(e, mode), frames, args.frames, in_flight)
            out.append(dict(mode=mode, run=run, frames=args.frames, frames_per_s=round(fps, 1)))
            print(json.dumps(out[-1]), flush=True)
    if "yuv" in modes:   # the kernel inside the frame path: residency stamps, in a run of their own (the probe re-captures nothing here, but harvests per batch)
        collect = set_mode(e, "yuv")
        e.stamp_probe(1)
        run_frames(e, collect, frames, 200, in_flight)
        spans = e.stamp_probe(-1)
        e.stamp_probe(0)
        slot = spans[:, 0].astype(int)
        m = (slot >= 64) & (slot < 200) & ((slot - 64) % 8 == 7)
        us = spans[m, 2] - spans[m, 1]
        out.append(dict(kernel="block_4x2_planar_in_frame_path", frames=int(m.sum()), residency_us_mean=round(float(us.mean()), 2),
                        residency_us_p90=round(float(np.percentile(us, 90)), 2), gb_per_s_at_mean=round(FRAME_BYTES / float(us.mean()) / 1e3, 1),
                        share_of_hbm_rate=round(FRAME_BYTES / (float(us.mean()) * 1e-6) / HBM_BYTES_PER_S, 3)))
        print(json.dumps(out[-1]), flush=True)
    set_mode(e, "raw")
    e.close()
    summary = {m: round(float(np.median([o["frames_per_s"] for o in out if o.get("mode") == m])), 1) for m in modes}
    print(json.dumps(dict(frames_per_s_median=summary, d2h_bytes_per_frame=dict(raw=W * H * 3, yuv=W * H * 3 // 2))), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default="raw,yuv,jpeg")
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--package_root", default=ROOT, help="the tree whose caffe_rtpose_amd package is measured (an older checkout for an A/B in one session)")
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import numpy as np
    import torch   # first: one HIP runtime for torch and the engine
    import caffe_rtpose_amd as r
    print(json.dumps(dict(library=r.LIB_PATH, device=torch.cuda.get_device_name(0))), flush=True)
    if not args.skip_kernel:
        e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=2, render=1))
        for w, h in ((W, H), (3840, 2160)):   # 2160p: nine times the bytes per launch, so the boundary between launches weighs less
            kernel_legs(r, torch, np, args, e, w, h)
        e.close()
    modes = [m for m in args.modes.split(",") if m]
    if modes:
        mode_legs(r, np, args, modes)


if __name__ == "__main__":
    main()

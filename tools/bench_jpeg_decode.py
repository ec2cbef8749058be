#!/usr/bin/env python
"""GPU JPEG decoder (jpeg_dec.hip) against the host decoder (rtp_decode_image), 1280x720 files written by rtp_encode_jpeg.

(a) Per quality (75, 95): the file size; rtp_decode_image on this box's CPU (one thread); Engine.decode_jpeg_device: host wall time of
    the call (parse, staging, copy, kernels, status) and the device time between an event pair around it; the rounds of the
    synchronisation kernel that did work / that were enqueued; the device time of a frame's decode kernels inside the engine from the
    residency stamps (rtp_stamp_probe slot 232 + j: first workgroup start of the first kernel to last workgroup end of the last).
(b) A sweep of S (bits per subsequence) and subsequences per workgroup on the q75 and q95 files: event time of the call, rounds.
(c) Engine frames/s from JPEG bytes (submit_frame_jpeg) against frames/s from the decoded BGR frames (submit_frame), same images,
    alternated, 7 frames in flight, batches of 2.
(d) rtpose.bin --video clip.mjpeg (the q75 file repeated; one producer thread reads a video) and rtpose.bin --image_dir with the same
    files (decoded ahead by the default producer pool), each with --gpu_decode and --host_decode alternated: frames/s (first frame
    committed -> last frame written) at the default producer thread count, and a hash of the JSON files.  The faster decoder of each
    source is the CLI's default for it.
  python tools/bench_jpeg_decode.py [--frames 300] [--cli_frames 1200] [--runs 3] [--skip_cli]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
W, H = 1280, 720


def files():
    sys.path.insert(0, ROOT)
    import caffe_rtpose_amd as r
    return {q: r.encode_jpeg(r.synth_frame(W, H, 1, seed=3), q) for q in (75, 95)}


def _timed_decode(e, r, torch, data, out, sub_bits, group, n):
    """(event ms per call, wall us per call, rounds) of the internal entry behind rtp_decode_jpeg_device"""
    from caffe_rtpose_amd.engine import _view_struct, frame_view
    v = _view_struct(frame_view(out))
    path, rounds = C.c_int(), (C.c_int * 2)()
    st = torch.cuda.Stream()
    call = lambda: r.lib.rtp_internal_jpeg_decode_device(e.h, data, C.c_size_t(len(data)), C.byref(v), C.c_void_p(st.cuda_stream), sub_bits, group, 0,
                                                         C.byref(path), rounds)
    for _ in range(5):
        assert call() == 0, r.lib.rtp_last_error(e.h).decode()
    assert path.value == 0, "the file took the host entropy path"
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = 0.0
    t = time.perf_counter()
    for _ in range(n):
        a.record(st)
        call()
        b.record(st)
        b.synchronize()
        ms += a.elapsed_time(b)
    wall = (time.perf_counter() - t) / n * 1e6
    return ms / n, wall, list(rounds)


def decoder_legs(args):
    import numpy as np
    import torch   # first: one HIP runtime for torch and the engine
    sys.path.insert(0, ROOT)
    import caffe_rtpose_amd as r
    fs = files()
    e = r.Engine(r.Config(disp_w=W, disp_h=H, frames_in_flight=7, batch_frames=2))
    out = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    for q, data in fs.items():
        want = r.decode_image(data)
        t = time.perf_counter()
        for _ in range(5):
            r.decode_image(data)
        cpu_ms = (time.perf_counter() - t) / 5 * 1e3
        ev_ms, wall_us, rounds = _timed_decode(e, r, torch, data, out, 0, 0, args.frames)
        assert np.array_equal(out.cpu().numpy(), want)
        # stamps of the decode kernels inside the engine
        for i in range(20):
            e.submit_frame_jpeg(data, tag=i)
            e.collect()
        e.stamp_probe(1)
        for i in range(args.frames):
            e.submit_frame_jpeg(data, tag=i)
            e.collect()
        spans = e.stamp_probe(-1)
        e.stamp_probe(0)
        slot = spans[:, 0].astype(int)
        m = (slot >= 232) & (slot < 248)
        dev_us = spans[m, 2] - spans[m, 1]
        print(json.dumps(dict(leg="decode", quality=q, file_bytes=len(data), rtp_decode_image_cpu_ms=round(cpu_ms, 2),
                              decode_jpeg_device_event_us=round(ev_ms * 1e3, 1), decode_jpeg_device_call_us=round(wall_us, 1),
                              rounds_worked=rounds[0], rounds_enqueued=rounds[1], stamp_frames=int(m.sum()),
                              decode_kernels_stamp_us=round(float(dev_us.mean()), 1) if m.any() else None,
                              decode_kernels_stamp_us_p90=round(float(np.percentile(dev_us, 90)), 1) if m.any() else None, bgr_bytes=W * H * 3)), flush=True)
    for q, data in fs.items():
        for s in (128, 256, 512, 1024, 2048):
            for g in (128, 256, 512, 1024):
                ev_ms, wall_us, rounds = _timed_decode(e, r, torch, data, out, s, g, max(args.frames // 6, 20))
                print(json.dumps(dict(leg="sweep", quality=q, S=s, group=g, event_us=round(ev_ms * 1e3, 1), call_us=round(wall_us, 1),
                                      rounds_worked=rounds[0], rounds_enqueued=rounds[1])), flush=True)
    # engine frames/s: JPEG bytes against the decoded frames
    imgs = {q: r.decode_image(d) for q, d in fs.items()}

    def rate(submit, x, n):
        t = time.perf_counter()
        done = 0
        for i in range(n):
            submit(x, tag=i)
            while e.in_flight() >= 7:
                e.collect()
                done += 1
        while e.in_flight():
            e.collect()
            done += 1
        return done / (time.perf_counter() - t)
    for q in fs:
        rate(e.submit_frame, imgs[q], 100)
        for run in range(args.runs):
            a = rate(e.submit_frame, imgs[q], args.frames * 3)
            b = rate(e.submit_frame_jpeg, fs[q], args.frames * 3)
            print(json.dumps(dict(leg="engine", quality=q, run=run, submit_frame_fps=round(a, 1), submit_frame_jpeg_fps=round(b, 1))), flush=True)
    e.close()


def cli_run(src, host_decode):
    """src: ["--video", clip] or ["--image_dir", dir]; the decoder is named explicitly (the default differs by source)"""
    tmp = tempfile.mkdtemp(prefix="rtp_jdec_")
    try:
        cmd = [BIN] + src + ["--model", "coco", "--write_json", tmp, "--no_display", "--no_frame_drops", "--frames_in_flight", "7",
                             "--batch_frames", "2", "--host_decode" if host_decode else "--gpu_decode"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit(f"rtpose.bin exited with {p.returncode}")
        fps = re.search(r"([0-9.]+) FPS first frame committed -> last frame written", p.stdout + p.stderr)
        names = sorted(os.listdir(tmp))
        h = hashlib.sha256()
        for f in names:
            h.update(f.encode() + b"\0" + open(os.path.join(tmp, f), "rb").read())
        return dict(leg="cli", source=src[0][2:], mode="host_decode" if host_decode else "gpu_decode", fps=float(fps.group(1)) if fps else None, files=len(names),
                    files_sha256=h.hexdigest()[:16])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--cli_frames", type=int, default=1200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--leg", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        decoder_legs(args)
        return
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "--frames", str(args.frames), "--runs", str(args.runs)], capture_output=True,
                       text=True, timeout=1100)
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        sys.exit(f"decoder leg exited with {p.returncode}")
    if not args.skip_cli:
        data = files()[75]
        tmp = tempfile.mkdtemp(prefix="rtp_jclip_")
        try:
            clip = os.path.join(tmp, "clip.mjpeg")
            with open(clip, "wb") as f:
                for _ in range(args.cli_frames):
                    f.write(data)
            imgs = os.path.join(tmp, "imgs")
            os.mkdir(imgs)
            for i in range(args.cli_frames):
                with open(os.path.join(imgs, f"f{i:06d}.jpg"), "wb") as f:
                    f.write(data)
            for src in (["--video", clip], ["--image_dir", imgs]):
                runs = []
                for _ in range(args.runs):
                    for host in (False, True):
                        runs.append(cli_run(src, host))
                        print(json.dumps(runs[-1]), flush=True)
                print(json.dumps(dict(source=src[0][2:], cli_files_identical=len({r["files_sha256"] for r in runs}) == 1)))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""GPU JPEG encoder (jpeg_enc.hip) against the host encoder (rtp_encode_jpeg), quality 98.

(a) Per frame size (1280x720, 1920x1080) and content (smooth = synth_frame, noise): an engine in JPEG mode (render = 1,
    rtp_set_render_jpeg 98) whose display image is the submitted frame plus the overlay; after a warm-up, the device time of the
    encoder's seven launches per frame from the residency stamps (rtp_stamp_probe slot 64 + 8 j + 6: first workgroup start to last
    workgroup end) over >= 200 frames; the host wall time of Engine.encode_jpeg_device on that frame (launch, device work, file on the
    host); rtp_encode_jpeg of the same frame on this box's CPU (one thread); the file size.
(b) rtpose.bin --video synthetic:1280x720:N --write_frames <tmp> --no_display --no_frame_drops, the GPU encoder (default) and
    --host_jpeg alternated, 3 runs each: frames/s (first frame committed -> last frame written), the count and a hash of the files
    (written to a temporary directory, deleted afterwards), raw vs compressed bytes copied device to host per frame.
  python tools/bench_jpeg.py [--frames 200] [--cli_frames 1200] [--runs 3] [--skip_cli]
"""
import argparse
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


def encoder_legs(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch   # first: one HIP runtime for torch and the engine
    import caffe_rtpose_amd as r
    out = []
    for w, h in ((1280, 720), (1920, 1080)):
        for content in ("smooth", "noise"):
            img = r.synth_frame(w, h, 1, seed=3) if content == "smooth" else np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
            e = r.Engine(r.Config(disp_w=w, disp_h=h, frames_in_flight=2, render=1))
            e.set_render_jpeg(98)
            for i in range(20):
                e.submit_frame(img, tag=i)
                e.collect_rendered_jpeg()
            e.stamp_probe(1)
            sizes = []
            for i in range(args.frames):
                e.submit_frame(img, tag=i)
                sizes.append(len(e.collect_rendered_jpeg()[3]))
            spans = e.stamp_probe(-1)
            e.stamp_probe(0)
            slot = spans[:, 0].astype(int)
            m = (slot >= 64) & (slot < 200) & ((slot - 64) % 8 == 6)
            dev_us = spans[m, 2] - spans[m, 1]
            d = torch.from_numpy(img).cuda()
            torch.cuda.synchronize()
            for _ in range(20):
                e.encode_jpeg_device(d, 98)
            t = time.perf_counter()
            for _ in range(args.frames):
                data = e.encode_jpeg_device(d, 98)
            call_us = (time.perf_counter() - t) / args.frames * 1e6
            assert data == r.encode_jpeg(img, 98)
            e.close()
            r.encode_jpeg(img, 98)
            t = time.perf_counter()
            for _ in range(10):
                r.encode_jpeg(img, 98)
            cpu_us = (time.perf_counter() - t) / 10 * 1e6
            out.append(dict(size=f"{w}x{h}", content=content, frames=int(m.sum()), encoder_device_us=round(float(dev_us.mean()), 1),
                            encoder_device_us_p90=round(float(np.percentile(dev_us, 90)), 1), encode_jpeg_device_call_us=round(call_us, 1),
                            encode_jpeg_device_bytes=len(data), rendered_file_bytes=int(np.mean(sizes)), rtp_encode_jpeg_cpu_us=round(cpu_us, 1),
                            raw_d2h_bytes=w * h * 3))
            print(json.dumps(out[-1]), flush=True)
    return out


def cli_run(n, host_jpeg):
    tmp = tempfile.mkdtemp(prefix="rtp_jpeg_")
    try:
        cmd = [BIN, "--video", f"synthetic:1280x720:{n}", "--model", "coco", "--write_frames", tmp, "--no_display", "--no_frame_drops",
               "--frames_in_flight", "7", "--batch_frames", "2"] + (["--host_jpeg"] if host_jpeg else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit(f"rtpose.bin exited with {p.returncode}")
        fps = re.search(r"([0-9.]+) FPS first frame committed -> last frame written", p.stdout + p.stderr)
        names = sorted(os.listdir(tmp))
        h = hashlib.sha256()
        total = 0
        for f in names:
            data = open(os.path.join(tmp, f), "rb").read()
            total += len(data)
            h.update(f.encode() + b"\0" + data)
        return dict(mode="host_jpeg" if host_jpeg else "gpu", fps=float(fps.group(1)) if fps else None, files=len(names),
                    mean_file_bytes=total // max(len(names), 1), files_sha256=h.hexdigest()[:16])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--cli_frames", type=int, default=1200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--leg", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        encoder_legs(args)
        return
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "--frames", str(args.frames)], capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        sys.exit(f"encoder leg exited with {p.returncode}")
    res = dict(encoder=[json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")])
    if not args.skip_cli:
        runs = []
        for _ in range(args.runs):
            for host in (False, True):
                runs.append(cli_run(args.cli_frames, host))
                print(json.dumps(runs[-1]), flush=True)
        res["cli"] = runs
        res["cli_files_identical"] = len({r["files_sha256"] for r in runs}) == 1
    print(json.dumps(res))


if __name__ == "__main__":
    main()

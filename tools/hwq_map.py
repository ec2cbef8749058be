#!/usr/bin/env python
"""Which of an engine's streams share a hardware queue, measured (rtp_debug_stream_queues):  python tools/hwq_map.py [B] [IN_FLIGHT] [frames] [reps] [net_w] [net_h]
Run it once per GPU_MAX_HW_QUEUES value, each time in a fresh process (the HIP runtime reads the variable once).  Prints the map and one
JSON line: the streams' owners (context, frame; frame 0 = the conv stream; context -1 = the legacy stream), the pair / single ratio matrix (median of 5; ~1 = side by side,
~2 = one queue), the queue classes read from it, how often every context was opened by `frames` frames pushed through in bench.py's loop
order, and a hash of their joints."""
import hashlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import caffe_rtpose_amd as r  # noqa: E402

APART, SHARED = 1.35, 1.65


def classes(ratio):
    """queue class per stream (the lowest stream it shares a queue with), or None where a pair is inconclusive"""
    n = len(ratio)
    cls = list(range(n))
    for a in range(n):
        for b in range(a):
            if APART <= ratio[a][b] <= SHARED:
                return None
            if ratio[a][b] > SHARED and cls[a] == a:
                cls[a] = cls[b]
    return cls


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    depth = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    nframes = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5          # pair timings per pair (their median counts); 0 = no map, frames only
    net_w = int(sys.argv[5]) if len(sys.argv) > 5 else 160
    net_h = int(sys.argv[6]) if len(sys.argv) > 6 else 96
    t0 = time.perf_counter()
    e = r.Engine(r.Config(net_w=net_w, net_h=net_h, precision=r.PREC_MIXED, frames_in_flight=depth, batch_frames=B))
    create_s = time.perf_counter() - t0
    owner, ratio, _ = e.stream_queues(reps)
    frames = [r.synth_frame(320, 240, i, seed=5) for i in range(nframes)]
    h = hashlib.sha256()
    sub = col = 0
    while col < nframes:                       # bench.py's loop: fill the pipeline, collect one
        while sub < nframes and e.in_flight() < depth:
            e.submit_frame(frames[sub], tag=sub)
            sub += 1
        tag, n, j = e.collect()
        assert tag == col
        h.update(np.int64(tag).tobytes() + np.int64(n).tobytes() + j.tobytes())
        col += 1
    opens = e.stream_queues(0)[2]
    e.close()
    if ratio is None:
        ratio = []
    cls = classes(ratio) if len(ratio) else None
    print("GPU_MAX_HW_QUEUES=%s B %d in flight %d: engine created in %.2f s" % (os.environ.get("GPU_MAX_HW_QUEUES", "(unset)"), B, depth, create_s))
    for k, (c, f) in enumerate(owner if len(ratio) else []):
        print("  %-5s %-6s queue class %s  | " % ("ctx %d" % c if c >= 0 else "", "legacy" if c < 0 else "conv" if f == 0 else "chain%d" % f, "?" if cls is None else cls[k]) + " ".join("%4.2f" % v for v in ratio[k]))
    print(json.dumps(dict(queues=os.environ.get("GPU_MAX_HW_QUEUES"), B=B, in_flight=depth, owner=owner, ratio=[[round(float(v), 3) for v in row] for row in ratio],
                          classes=cls, opens=opens, hash=h.hexdigest()[:24], create_s=round(create_s, 3))))


if __name__ == "__main__":
    main()

"""GPU JPEG encoder, host side: rtp_jpeg_max_bytes bounds every file rtp_encode_jpeg writes, the new symbols are exported and the CLI
names --host_jpeg.  No GPU needed."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")


def test_max_bytes_bounds_adversarial_q100_files():
    import caffe_rtpose_amd as r
    rng = np.random.default_rng(3)
    for w, h in ((1, 1), (2, 1), (7, 5), (17, 17), (33, 31), (65, 9), (301, 173), (640, 368)):
        y, x = np.mgrid[0:h, 0:w]
        checker = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
        for img in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), checker, np.full((h, w, 3), 255, np.uint8)):
            n = len(r.encode_jpeg(img, 100))
            assert r.jpeg_max_bytes(w, h) >= n, (w, h, n)


def test_max_bytes_is_monotone():
    import caffe_rtpose_amd as r
    assert r.jpeg_max_bytes(0, 5) == 0 and r.jpeg_max_bytes(5, 0) == 0
    for w in range(1, 70, 3):
        for h in range(1, 70, 5):
            b = r.jpeg_max_bytes(w, h)
            assert r.jpeg_max_bytes(w + 1, h) >= b and r.jpeg_max_bytes(w, h + 1) >= b
    assert r.jpeg_max_bytes(1920, 1080) > r.jpeg_max_bytes(1280, 720) > r.jpeg_max_bytes(640, 368)


def test_symbols_are_exported():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd._lib import lib
    for name in ("rtp_jpeg_max_bytes", "rtp_encode_jpeg_device", "rtp_set_render_jpeg", "rtp_collect_rendered_jpeg"):
        assert hasattr(lib, name), name
    for name in ("set_render_jpeg", "collect_rendered_jpeg", "encode_jpeg_device"):
        assert callable(getattr(r.Engine, name)), name
    with open(os.path.join(ROOT, "include", "rtpose_mi355x.h")) as f:
        header = f.read()
    for name in ("rtp_jpeg_max_bytes", "rtp_encode_jpeg_device", "rtp_set_render_jpeg", "rtp_collect_rendered_jpeg"):
        assert name + "(" in header, name


def test_cli_help_names_host_jpeg():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert "--host_jpeg" in p.stdout + p.stderr

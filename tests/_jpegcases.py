"""Files and ctypes helpers shared by test_jpeg_decode_cpu.py and test_jpeg_decode.py: the baseline / progressive fixtures of
tests/golden/codecs, a grid of files written by rtp_encode_jpeg, and the internal entries of the GPU JPEG decoder's host side."""
import ctypes as C
import functools
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "codecs")
BASELINE = ["j420_q75", "j420_q30_opt", "j420_rst", "j444_q90", "j422_q85", "j422_w3", "jgray_q88", "j420_tiny", "j420_16x16"]
SIZES = [(1, 1), (7, 5), (17, 17), (33, 31), (65, 9), (301, 173)]
KINDS = ["noise", "checker", "flat"]
QUALITIES = [25, 75, 100]
DEVICE, HOST = 0, 1   # RTP_JPEG_ENTROPY_*


def fixture(name):
    return open(os.path.join(GOLD, name + ".jpg"), "rb").read()


def progressive_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "jprog*.jpg")))


def content(kind, w, h):
    rng = np.random.default_rng(w * 7919 + h)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "checker":   # 1-pixel black / white: long codes, many 0xFF bytes
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    return np.full((h, w, 3), 93, np.uint8)


@functools.lru_cache(maxsize=None)
def grid():
    """[(name, file bytes)] of the generated grid (rtp_encode_jpeg: baseline 4:2:0, one scan)"""
    import caffe_rtpose_amd as r
    return [(f"{kind}_{w}x{h}_q{q}", r.encode_jpeg(content(kind, w, h), q)) for (w, h) in SIZES for kind in KINDS for q in QUALITIES]


def _lib():
    import caffe_rtpose_amd as r
    return r.lib


def codec_error():
    lib = _lib()
    lib.rtp_codec_last_error.restype = C.c_char_p
    return lib.rtp_codec_last_error().decode()


def host_decode(data):
    """(rc, message) of rtp_decode_image on the whole file"""
    lib = _lib()
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    w, h = C.c_int(), C.c_int()
    rc = lib.rtp_decode_image(buf, len(data), None, 0, C.byref(w), C.byref(h))
    if rc:
        return rc, codec_error()
    out = np.empty((h.value, w.value, 3), np.uint8)
    rc = lib.rtp_decode_image(buf, len(data), out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.size, C.byref(w), C.byref(h))
    return rc, (codec_error() if rc else "")


def plan(data):
    """(rc, info) of the planner: info = [path, W, H, components, segments, subsequences, staged words, blocks]"""
    lib = _lib()
    info = (C.c_int * 8)()
    rc = lib.rtp_internal_jpeg_coefficients(data, C.c_size_t(len(data)), 0, None, C.c_size_t(0), info)
    return rc, list(info)


def host_coefficients(data):
    """(rc, coefficients) of the factored host entropy decoder (headers and scans -> coefficients)"""
    lib = _lib()
    info = (C.c_int * 8)()
    rc = lib.rtp_internal_jpeg_coefficients(data, C.c_size_t(len(data)), 1, None, C.c_size_t(0), info)
    if rc:
        return rc, None
    coef = np.zeros(info[7] * 64, np.int16)
    rc = lib.rtp_internal_jpeg_coefficients(data, C.c_size_t(len(data)), 1, coef.ctypes.data_as(C.c_void_p), C.c_size_t(coef.size), info)
    return rc, coef


def emulate(data, sub_bits, group, blocks):
    """(rc, coefficients, info, rounds) of the serial emulation of the device's entropy decoder"""
    lib = _lib()
    info = (C.c_int * 8)()
    rounds = (C.c_int * 2)()
    coef = np.full(max(blocks, 1) * 64, 0x5a5a, np.int16)
    rc = lib.rtp_internal_jpeg_entropy_emulate(data, C.c_size_t(len(data)), sub_bits, group, coef.ctypes.data_as(C.c_void_p), C.c_size_t(coef.size), info, rounds)
    return rc, coef[: blocks * 64], list(info), list(rounds)


def scan_start(data):
    """offset of the first entropy-coded byte of a single-scan file"""
    i = data.index(b"\xff\xda")
    return i + 2 + ((data[i + 2] << 8) | data[i + 3])

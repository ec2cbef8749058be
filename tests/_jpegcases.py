"""Files and ctypes helpers shared by test_jpeg_decode_cpu.py and test_jpeg_decode.py: the baseline / progressive fixtures of
tests/golden/codecs, the layout fixtures of tests/golden/codecs/layouts, a grid of files written by rtp_encode_jpeg, and the internal entries of the GPU JPEG decoder's host side."""
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
# tests/golden/codecs/layouts (tools/make_codec_fixtures.py --layouts; pixels = libjpeg's): where the planner sends the entropy decoding.
# DEVICE: one interleaved scan of at most 10 blocks per MCU with nothing irregular.  Y / Cb / Cr (h, v) in the comments.
LAYOUTS = {
    "l440_37x29": DEVICE, "l440_2x9": DEVICE, "l440_1x5": DEVICE,   # (1,2)(1,1)(1,1): h1v2 fancy up-sampling
    "l411_37x9": DEVICE,                                            # (4,1)
    "l42_40x20": DEVICE, "l24_21x40": DEVICE,                       # (4,2), (2,4): 10 blocks per MCU
    "l14_9x40": DEVICE, "l31_37x29": DEVICE,                        # (1,4), (3,1)
    "lmixed_33x17": DEVICE, "lmixed_3x9": DEVICE,                   # (2,2)(2,1)(1,2): 8 blocks
    "llumaup_37x29": DEVICE,                                        # (1,1)(2,2)(2,2): 9 blocks, luma up-sampled
    "lgray_h2v2_37x29": DEVICE,                                     # one component declared (2,2)
    "l420_3scans": HOST, "l440_3scans_dri5": HOST,                  # one scan per component
    "l420_dri1_40x24": DEVICE, "l42_dri1_40x20": DEVICE,            # a restart marker behind every MCU
    "l420_dri2_fill": HOST,                                         # FF FF in front of every RSTn
    "lsof1_tables3": DEVICE, "lsof0_tables3": DEVICE,               # chroma quantiser and Huffman tables under id 3
    "lq16_300_260": DEVICE, "lq8_255": DEVICE,                      # 16-bit DQT; 8-bit tables of 255
    "l3scans_requant": HOST,                                        # table 1 redefined between the Cb scan and the Cr scan
    "lq_twice": DEVICE,                                             # table 1 defined twice in front of the only scan
    "ladobe0_rgb": DEVICE, "ladobe1_420": DEVICE, "ladobe2_ycc": DEVICE, "lids_rgb": DEVICE, "lids_012_ycc": DEVICE,   # no JFIF
    "ljfif_adobe0_ycc": DEVICE, "ljfif_ids_rgb_ycc": DEVICE,        # JFIF wins over the Adobe transform and the ids
    "lkeep_rgb_q85": DEVICE,                                        # Pillow's own keep_rgb file
}


def fixture(name):
    return open(os.path.join(GOLD, name + ".jpg"), "rb").read()


def layout(name):
    """(file bytes, libjpeg's pixels as BGR) of a layout fixture"""
    base = os.path.join(GOLD, "layouts", name)
    return open(base + ".jpg", "rb").read(), np.load(base + ".npy")


def layout_files():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "layouts", "*.jpg")))


def frame_components(data):
    """[(id, h, v, tq)] of the frame header"""
    i = 2
    while data[i + 1] not in (0xC0, 0xC1, 0xC2):
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    return [(data[i + 10 + 3 * c], data[i + 11 + 3 * c] >> 4, data[i + 11 + 3 * c] & 15, data[i + 12 + 3 * c]) for c in range(data[i + 9])]


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

"""Shared by the YUV tests (test_yuv_frames_cpu.py, test_yuv_frames.py): test planes, the formula of rtp_convert_yuv restated in numpy,
and a Y4M writer."""
import functools

import numpy as np

SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
Y4M_TAG = {"420": b"C420jpeg", "422": b"C422", "444": b"C444", "mono": b"Cmono"}
ODD_SIZES = [(1, 1), (2, 2), (3, 3), (5, 4), (16, 8), (67, 45)]   # (w, h)


def chroma_shape(w, h, fmt):
    sx, sy = SHIFTS[fmt]
    return (h + sy) >> sy, (w + sx) >> sx


def planes(w, h, fmt, seed=0):
    """(y, u, v) of full-range random bytes (the clamps are exercised); u = v = None for "mono"."""
    rs = np.random.RandomState(1000 * seed + 7 * w + h)
    y = rs.randint(0, 256, (h, w)).astype(np.uint8)
    if fmt == "mono":
        return y, None, None
    ch, cw = chroma_shape(w, h, fmt)
    return y, rs.randint(0, 256, (ch, cw)).astype(np.uint8), rs.randint(0, 256, (ch, cw)).astype(np.uint8)


def interleave(u, v, order="uv"):
    """(ch, cw, 2) chroma of NV12 ("uv") or NV21 ("vu")."""
    return np.ascontiguousarray(np.stack([u, v] if order == "uv" else [v, u], -1))


def ref_bgr(y, u, v, fmt):
    """The issue's formula: c = 298 (Y - 16), d = U - 128, e = V - 128; arithmetic shift, clamp to 0..255."""
    h, w = y.shape
    c = 298 * (y.astype(np.int32) - 16)
    if u is None:
        d = e = np.zeros_like(c)
    else:
        sx, sy = SHIFTS[fmt]
        yy, xx = np.arange(h)[:, None] >> sy, np.arange(w)[None, :] >> sx
        d = u.astype(np.int32)[yy, xx] - 128
        e = v.astype(np.int32)[yy, xx] - 128
    out = np.empty((h, w, 3), np.uint8)
    out[..., 2] = np.clip((c + 409 * e + 128) >> 8, 0, 255)
    out[..., 1] = np.clip((c - 100 * d - 208 * e + 128) >> 8, 0, 255)
    out[..., 0] = np.clip((c + 516 * d + 128) >> 8, 0, 255)
    return out


@functools.lru_cache(maxsize=1)
def exhaustive():
    """All 2^24 (Y, U, V) triples as one 4096 x 4096 4:4:4 image: pixel i = row * 4096 + col holds Y = i & 255, U = (i >> 8) & 255,
    V = i >> 16.  Returns read-only (y, u, v)."""
    i = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    out = tuple(np.ascontiguousarray(a.astype(np.uint8)) for a in (i & 255, (i >> 8) & 255, i >> 16))
    for a in out:
        a.setflags(write=False)
    return out


def write_y4m(path, w, h, fmt, n, seed=0):
    """A Y4M file of n random frames; returns their planes."""
    frames = []
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 %s\n" % (w, h, Y4M_TAG[fmt]))
        for i in range(n):
            y, u, v = planes(w, h, fmt, seed=seed + i)
            f.write(b"FRAME\n" + y.tobytes() + (b"" if u is None else u.tobytes() + v.tobytes()))
            frames.append((y, u, v))
    return frames


def from_bgr(img, fmt="420"):
    """Planes of a BGR image (BT.601 limited range in floating point, chroma taken at the even positions): test input only — what the
    tests compare is always what the library makes of THESE planes."""
    b, g, r_ = (img[..., c].astype(np.float64) for c in range(3))
    y = np.clip(np.rint(0.257 * r_ + 0.504 * g + 0.098 * b + 16), 0, 255).astype(np.uint8)
    if fmt == "mono":
        return y, None, None
    sx, sy = SHIFTS[fmt]
    u = np.clip(np.rint(-0.148 * r_ - 0.291 * g + 0.439 * b + 128), 0, 255).astype(np.uint8)
    v = np.clip(np.rint(0.439 * r_ - 0.368 * g - 0.071 * b + 128), 0, 255).astype(np.uint8)
    return y, np.ascontiguousarray(u[::1 << sy, ::1 << sx]), np.ascontiguousarray(v[::1 << sy, ::1 << sx])


@functools.lru_cache(maxsize=1)
def exhaustive_420():
    """All 2^24 (Y, U, V) triples once more, as one 4096 x 4096 4:2:0 image (what the 4 x 2 kernel accepts): chroma sample
    j = row * 2048 + col holds U = j & 255, V = (j >> 8) & 255, and the four luma pixels under it hold Y = 4 (j >> 16) + 2 dy + dx,
    so each of the 64 samples of a (U, V) pair meets four other Y values.  Returns read-only (y, u, v)."""
    j = np.arange(1 << 22, dtype=np.uint32).reshape(2048, 2048)
    u, v = (j & 255).astype(np.uint8), ((j >> 8) & 255).astype(np.uint8)
    k = (4 * (j >> 16)).astype(np.uint8)
    y = np.empty((4096, 4096), np.uint8)
    for dy in range(2):
        for dx in range(2):
            y[dy::2, dx::2] = k + (2 * dy + dx)
    for a in (y, u, v):
        a.setflags(write=False)
    return y, u, v


LAYOUT_GENERIC, LAYOUT_420_PLANAR, LAYOUT_420_NV12, LAYOUT_420_NV21 = 0, 1, 2, 3


def layout(y, u, v, out, order="bgr", interleaved_order="uv"):
    """The kernel rtp_convert_yuv_device would launch for these planes and this destination (kernels.h YuvLayout), from the library's
    own host-side choice: nothing is dereferenced, so stand-in objects do."""
    import ctypes as C
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    from caffe_rtpose_amd.engine import _view_struct, _yuv_struct
    fn = _lib.lib.rtp_internal_yuv_layout
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(_lib.rtp_yuv_view), C.POINTER(_lib.rtp_frame_view)]
    s = _yuv_struct(r.yuv_view(y, u, v, interleaved_order=interleaved_order))
    d = _view_struct(r.frame_view(out, order))
    return fn(C.byref(s), C.byref(d))

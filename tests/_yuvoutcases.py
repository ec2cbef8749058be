"""Shared by the YUV-output tests (test_yuv_out_cpu.py, test_yuv_out.py): the formulas of rtp_convert_bgr_to_yuv restated in numpy, test
images, the whole BGR cube, destination planes with guard bytes, and a Y4M parser."""
import functools

import numpy as np

SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
GUARD = 0xA5


def image(w, h, seed=0):
    """Full-range random BGR pixels, with a few saturated and grey ones."""
    rs = np.random.RandomState(977 * seed + 13 * w + h)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    flat = img.reshape(-1, 3)
    for i, px in enumerate(((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (128, 128, 128))):
        if i < len(flat):
            flat[(i * 7) % len(flat)] = px
    return img


def ref_planes(bgr, fmt):
    """The issue's formulas: Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16 per pixel; U, V from the rounded mean of each chroma cell, with
    coordinates clamped to the last column / row; arithmetic shifts.  fmt "420", "422", "444" or "mono" -> (y, u, v), u = v = None for mono."""
    p = bgr.astype(np.int32)
    b, g, r_ = p[..., 0], p[..., 1], p[..., 2]
    y = (((66 * r_ + 129 * g + 25 * b + 128) >> 8) + 16).astype(np.uint8)
    if fmt == "mono":
        return y, None, None
    h, w = y.shape
    sx, sy = SHIFTS[fmt]
    cw, ch = (w + sx) >> sx, (h + sy) >> sy
    s = np.zeros((ch, cw, 3), np.int32)
    for dy in range(1 << sy):
        for dx in range(1 << sx):
            yy = np.minimum((np.arange(ch) << sy) + dy, h - 1)[:, None]
            xx = np.minimum((np.arange(cw) << sx) + dx, w - 1)[None, :]
            s += p[yy, xx]
    n = (1 << sx) * (1 << sy)
    m = (s + 2) >> 2 if n == 4 else ((s + 1) >> 1 if n == 2 else s)
    mb, mg, mr = m[..., 0], m[..., 1], m[..., 2]
    u = (((-38 * mr - 74 * mg + 112 * mb + 128) >> 8) + 128).astype(np.uint8)
    v = (((112 * mr - 94 * mg - 18 * mb + 128) >> 8) + 128).astype(np.uint8)
    return y, u, v


@functools.lru_cache(maxsize=1)
def cube():
    """Every BGR triple once, as a read-only 4096 x 4096 image: pixel i = row * 4096 + col holds B = i & 255, G = (i >> 8) & 255,
    R = i >> 16."""
    i = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    img = np.stack([(i & 255).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i >> 16).astype(np.uint8)], -1)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=2)
def cube_planes(fmt):
    """rtp_convert_bgr_to_yuv of the cube (computed once per format, read-only)."""
    import caffe_rtpose_amd as r
    out = r.convert_bgr_to_yuv(cube(), int(fmt))
    for a in out:
        a.setflags(write=False)
    return out


def chroma_shape(w, h, fmt):
    sx, sy = SHIFTS[fmt]
    return (h + sy) >> sy, (w + sx) >> sx


class HostPlanes:
    """Destination planes on the host inside guard arrays: `extra` columns of pitch padding, 2 guard rows above and below, first column
    dx.  layout "planar", "nv12", "nv21" or "mono"; .out = the (y, u, v) arguments yuv_view takes, .order its interleaved_order."""

    def __init__(self, w, h, fmt, layout="planar", extra=0, dx=0):
        self.w, self.h, self.fmt, self.layout, self.dx = w, h, fmt, layout, dx
        self.order = "vu" if layout == "nv21" else "uv"
        self.big = [np.full((h + 4, w + extra + dx), GUARD, np.uint8)]
        if layout == "mono":
            self.ch = self.cw = 0
        else:
            self.ch, self.cw = chroma_shape(w, h, fmt)
            if layout == "planar":
                self.big += [np.full((self.ch + 4, self.cw + extra + dx), GUARD, np.uint8) for _ in range(2)]
            else:
                self.big.append(np.full((self.ch + 4, self.cw + extra + dx, 2), GUARD, np.uint8))
        win = [self.big[0][2:2 + h, dx:dx + w]] + [a[2:2 + self.ch, dx:dx + self.cw] for a in self.big[1:]]
        self.out = (tuple(win) + (None, None))[:3]   # (y, u, v), (y, uv, None) or (y, None, None)
        self.win = win

    def planes(self):
        """(y, u, v) as written (copies); u = v = None for mono"""
        if self.layout == "mono":
            return self.win[0].copy(), None, None
        if self.layout == "planar":
            return tuple(a.copy() for a in self.win)
        a, b = self.win[1][..., 0].copy(), self.win[1][..., 1].copy()
        return (self.win[0].copy(), a, b) if self.layout == "nv12" else (self.win[0].copy(), b, a)

    def guards_intact(self):
        for big, win_rows, win_cols in zip(self.big, [self.h] + [self.ch] * 2, [self.w] + [self.cw] * 2):
            mask = np.ones(big.shape, bool)
            mask[2:2 + win_rows, self.dx:self.dx + win_cols] = False
            if not (big[mask] == GUARD).all():
                return False
        return True


def parse_y4m(data):
    """(w, h, header tags, [(y, u, v)]) of an 8-bit 4:2:0 Y4M byte string."""
    nl = data.index(b"\n")
    tags = data[:nl].split(b" ")
    assert tags[0] == b"YUV4MPEG2", tags
    w = int([t for t in tags if t[:1] == b"W"][0][1:])
    h = int([t for t in tags if t[:1] == b"H"][0][1:])
    cw, ch = (w + 1) // 2, (h + 1) // 2
    pos, frames = nl + 1, []
    while pos < len(data):
        assert data[pos:pos + 6] == b"FRAME\n", data[pos:pos + 16]
        pos += 6
        a = np.frombuffer(data, np.uint8, w * h + 2 * cw * ch, pos)
        pos += a.size
        frames.append((a[:w * h].reshape(h, w), a[w * h:w * h + cw * ch].reshape(ch, cw), a[w * h + cw * ch:].reshape(ch, cw)))
    return w, h, tags, frames


LAYOUT_GENERIC, LAYOUT_420_PLANAR, LAYOUT_420_NV12, LAYOUT_420_NV21 = 0, 1, 2, 3


def layout(frame, y, u, v, order="bgr", interleaved_order="uv"):
    """The kernel rtp_convert_to_yuv_device would launch for this frame and these planes (kernels.h YuvLayout), from the library's own
    host-side choice: nothing is dereferenced."""
    import ctypes as C
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    from caffe_rtpose_amd.engine import _view_struct, _yuv_struct
    fn = _lib.lib.rtp_internal_yuv_export_layout
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(_lib.rtp_frame_view), C.POINTER(_lib.rtp_yuv_view)]
    s = _view_struct(r.frame_view(frame, order))
    d = _yuv_struct(r.yuv_view(y, u, v, interleaved_order=interleaved_order))
    return fn(C.byref(s), C.byref(d))

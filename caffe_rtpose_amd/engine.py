"""ctypes mirror of include/rtpose_mi355x.h (numpy in / numpy out).  Plumbing only."""
import ctypes as C
import os
import sys

import numpy as np

from ._lib import lib, rtp_config, rtp_frame_view, rtp_yuv_view, rtp_maps_config, rtp_maps_view, rtp_crops_config, rtp_crops_view, rtp_track_config, rtp_track_state, rtp_appearance_config, rtp_appearance_state, rtp_smooth_config, rtp_smooth_state, rtp_overlay_config, rtp_trail_state, rtp_redact_config, fp, ip

MODEL_COCO_18, MODEL_MPI_15 = 0, 1
PREC_FP16, PREC_FP32, PREC_MIXED, PREC_F16X3 = 0, 1, 2, 3
EXEC_GRAPH, EXEC_EAGER = 0, 1
MAX_PEOPLE = 96
MAX_NUM_PARTS = 70
MAPS_GRIDS = {"net": 0, "lowres": 1}              # RTP_MAPS_GRID_*
MAPS_FORMATS = {"f32": 0, "f16": 1, "u8": 2}      # RTP_MAPS_F32 / F16 / U8
_MAPS_DTYPES = {0: np.float32, 1: np.float16, 2: np.uint8}
CROPS_LAYOUTS = {"hwc_bgr": 0, "chw_rgb": 1}      # RTP_CROPS_HWC_BGR / CHW_RGB
CROP_BOX_FLOATS = 6                               # left, top, width, height, counting parts, valid


# error codes of include/rtpose_mi355x.h
RTP_OK, RTP_EINVAL, RTP_ENOMEM, RTP_ENODEV, RTP_EIO, RTP_EAGAIN, RTP_EHIP, RTP_ERANGE = 0, -22, -12, -19, -5, -11, -70, -34


class RtpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rtp error {code}: {msg}")
        self.code = code


def _f(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(fp)


class Config:
    def __init__(self, **kw):
        self.c = rtp_config()
        lib.rtp_config_default(C.byref(self.c))
        self._keep = []
        for k, v in kw.items():
            self.set(k, v)

    def set(self, k, v):
        if k in ("proto_path", "weights_path", "split_layers"):
            v = None if v is None else str(v).encode()
            self._keep.append(v)
        setattr(self.c, k, v)
        return self


def model_tables(model):
    npart, nlimb = C.c_int(), C.c_int()
    limb = (C.c_int * 38)()
    mp = (C.c_int * 38)()
    rc = lib.rtp_model_tables(model, C.byref(npart), C.byref(nlimb), limb, mp)
    if rc:
        raise RtpError(rc, "bad model")
    n = nlimb.value * 2
    return npart.value, nlimb.value, list(limb)[:n], list(mp)[:n]


def default_thresholds(model):
    a, b, e = C.c_float(), C.c_float(), C.c_float()
    c, d = C.c_int(), C.c_int()
    rc = lib.rtp_default_thresholds(model, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e))
    if rc:
        raise RtpError(rc, "bad model")
    return dict(nms_threshold=a.value, inter_threshold=b.value, inter_min_above=c.value, min_subset_cnt=d.value,
                min_subset_score=e.value)


def process_and_pad_image(img_u8, tw, th, normalize):
    oh, ow, _ = img_u8.shape
    out = np.empty((3, th, tw), np.float32)
    img = np.ascontiguousarray(img_u8, np.uint8)
    rc = lib.rtp_process_and_pad_image(_f(out), img.ctypes.data_as(C.POINTER(C.c_ubyte)), ow, oh, tw, th, int(normalize))
    if rc:
        raise RtpError(rc, "Image too big for target size.")
    return out


def format_json(joints, num_people, num_parts, frame_scale):
    buf = C.create_string_buffer(1 << 20)
    j = np.ascontiguousarray(joints, np.float32).reshape(-1)
    if j.size == 0:
        j = np.zeros(1, np.float32)
    n = lib.rtp_format_json(buf, len(buf), _f(j), num_people, num_parts, C.c_float(frame_scale))
    if n < 0:
        raise RtpError(n, "format_json")
    return buf.raw[:n]


def _u8(a):
    assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_ubyte))


def resize_area(img, dw, dh):
    img = np.ascontiguousarray(img, np.uint8)
    out = np.empty((dh, dw, 3), np.uint8)
    rc = lib.rtp_resize_area(_u8(img), img.shape[1], img.shape[0], _u8(out), dw, dh)
    if rc:
        raise RtpError(rc, "resize_area")
    return out


def warp_display(img, disp_w, disp_h):
    img = np.ascontiguousarray(img, np.uint8)
    out = np.empty((disp_h, disp_w, 3), np.uint8)
    s = C.c_double()
    rc = lib.rtp_warp_display(_u8(img), img.shape[1], img.shape[0], _u8(out), disp_w, disp_h, C.byref(s))
    if rc:
        raise RtpError(rc, "warp_display")
    return out, s.value


def preprocess_frame(img, disp_w, disp_h, net_w, net_h, num_scales=1, start_scale=1.0, scale_gap=0.3):
    img = np.ascontiguousarray(img, np.uint8)
    out = np.empty((num_scales, 3, net_h, net_w), np.float32)
    disp = np.empty((disp_h, disp_w, 3), np.uint8)
    fs = C.c_float()
    rc = lib.rtp_preprocess_frame(_u8(img), img.shape[1], img.shape[0], disp_w, disp_h, net_w, net_h, num_scales, start_scale, scale_gap,
                                  _f(out), _u8(disp), C.byref(fs))
    if rc:
        raise RtpError(rc, "preprocess_frame")
    return out, disp, fs.value


def synth_frame(w, h, index, seed=2):
    out = np.empty((h, w, 3), np.uint8)
    rc = lib.rtp_synth_frame(_u8(out), w, h, index, seed)
    if rc:
        raise RtpError(rc, "synth_frame")
    return out


def load_image(path):
    w, h = C.c_int(), C.c_int()
    rc = lib.rtp_load_image(str(path).encode(), None, 0, C.byref(w), C.byref(h))
    if rc:
        raise RtpError(rc, f"cannot decode {path}")
    out = np.empty((h.value, w.value, 3), np.uint8)
    rc = lib.rtp_load_image(str(path).encode(), _u8(out), out.size, C.byref(w), C.byref(h))
    if rc:
        raise RtpError(rc, f"cannot decode {path}")
    return out


def prototxt_summary(path):
    nl, nc, npart, mp, hc = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    thr = C.c_float()
    rc = lib.rtp_prototxt_summary(str(path).encode(), C.byref(nl), C.byref(nc), C.byref(npart), C.byref(mp), C.byref(thr), C.byref(hc))
    if rc:
        raise RtpError(rc, lib.rtp_last_error(None).decode())
    return dict(num_layers=nl.value, num_conv=nc.value, num_parts=npart.value, max_peaks=mp.value,
                nms_threshold=thr.value, heat_channels=hc.value)


def synth_weights(seed, name, cout, cin, k):
    w = np.empty((cout, cin, k, k), np.float32)
    b = np.empty((cout,), np.float32)
    rc = lib.rtp_synth_weights(seed, name.encode(), cout, cin, k, _f(w), _f(b))
    if rc:
        raise RtpError(rc, "synth_weights")
    return w, b


def write_synthetic_caffemodel(model, seed, path):
    rc = lib.rtp_write_synthetic_caffemodel(model, seed, str(path).encode())
    if rc:
        raise RtpError(rc, lib.rtp_last_error(None).decode())


def write_builtin_prototxt(model, path):
    rc = lib.rtp_write_builtin_prototxt(model, str(path).encode())
    if rc:
        raise RtpError(rc, lib.rtp_last_error(None).decode())


def read_caffemodel_layers(path):
    n = lib.rtp_caffemodel_layer(str(path).encode(), -1, None, 0, None, None, None, None)
    if n < 0:
        raise RtpError(n, lib.rtp_last_error(None).decode())
    out = []
    name = C.create_string_buffer(128)
    nb = C.c_int()
    c0, c1 = C.c_long(), C.c_long()
    head = np.zeros(8, np.float32)
    for i in range(n):
        lib.rtp_caffemodel_layer(str(path).encode(), i, name, 128, C.byref(nb), C.byref(c0), C.byref(c1), _f(head))
        out.append(dict(name=name.value.decode(), num_blobs=nb.value, count0=c0.value, count1=c1.value, head0=head.copy()))
    return out


def decode_image(data):
    """cv::imread(IMREAD_COLOR) of an encoded PNG / JPEG byte string -> BGR HWC u8."""
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    w, h = C.c_int(), C.c_int()
    rc = lib.rtp_decode_image(buf, len(data), None, 0, C.byref(w), C.byref(h))
    if rc:
        raise RtpError(rc, lib.rtp_codec_last_error().decode())
    out = np.empty((h.value, w.value, 3), np.uint8)
    rc = lib.rtp_decode_image(buf, len(data), _u8(out), out.size, C.byref(w), C.byref(h))
    if rc:
        raise RtpError(rc, lib.rtp_codec_last_error().decode())
    return out


def encode_jpeg(bgr, quality=98):
    """cv::imwrite(.jpg) of a BGR HWC u8 image -> bytes."""
    img = np.ascontiguousarray(bgr, np.uint8)
    out = np.empty(img.size * 2 + 4096, np.uint8)   # generous: one pass instead of a size query + encode
    n = lib.rtp_encode_jpeg(_u8(img), img.shape[1], img.shape[0], quality, _u8(out), out.size)
    if n < 0:
        raise RtpError(n, lib.rtp_codec_last_error().decode())
    return out[:n].tobytes()


def jpeg_max_bytes(w, h):
    """rtp_jpeg_max_bytes: the largest JPEG file encode_jpeg / the GPU encoder can write for a w x h image."""
    return int(lib.rtp_jpeg_max_bytes(int(w), int(h)))


JPEG_ENTROPY_DEVICE, JPEG_ENTROPY_HOST = 0, 1   # RTP_JPEG_ENTROPY_*: where a file's Huffman decoding ran (Engine.decode_jpeg_device)


class Video:
    """cv::VideoCapture for Y4M / raw MJPEG files."""

    def __init__(self, path):
        self.h = C.c_void_p()
        w, h, n = C.c_int(), C.c_int(), C.c_int()
        rc = lib.rtp_video_open(str(path).encode(), C.byref(self.h), C.byref(w), C.byref(h), C.byref(n))
        if rc:
            self.h = C.c_void_p()
            raise RtpError(rc, lib.rtp_codec_last_error().decode())
        self.w, self.h_, self.nframes = w.value, h.value, n.value

    def read(self):
        out = np.empty((self.h_, self.w, 3), np.uint8)
        rc = lib.rtp_video_read(self.h, _u8(out), out.size)
        if rc == -11:
            return None
        if rc:
            raise RtpError(rc, lib.rtp_codec_last_error().decode())
        return out

    def chroma(self):
        return video_chroma(self)

    def read_yuv(self):
        return video_read_yuv(self)

    def read_jpeg(self):
        """rtp_video_read_jpeg: the next frame of a raw MJPEG stream as the bytes of its file (None at the end), not decoded."""
        p, n = C.POINTER(C.c_ubyte)(), C.c_size_t()
        rc = lib.rtp_video_read_jpeg(self.h, C.byref(p), C.byref(n))
        if rc == -11:
            return None
        if rc:
            raise RtpError(rc, lib.rtp_codec_last_error().decode())
        return C.string_at(p, n.value)

    def close(self):
        if self.h:
            lib.rtp_video_close(self.h)
            self.h = C.c_void_p()


def device_local_cpus(device_id):
    """rtp_device_local_cpus: the CPUs next to a GPU's PCI function as a list of ints ([] where the platform does not say)."""
    buf = C.create_string_buffer(1024)
    if lib.rtp_device_local_cpus(int(device_id), buf, len(buf)) <= 0:
        return []
    cpus = []
    for part in buf.value.decode().split(","):
        a, _, b = part.partition("-")
        cpus += list(range(int(a), int(b or a) + 1))
    return cpus


def plan_summary(cfg):
    buf = C.create_string_buffer(1 << 20)
    n = lib.rtp_plan_summary(C.byref(cfg.c), buf, len(buf))
    if n < 0:
        raise RtpError(n, lib.rtp_last_error(None).decode())
    return buf.raw[:n].decode()


def frame_view(obj, order="bgr"):
    """The rtp_frame_view fields of a u8 frame in device memory, from its __cuda_array_interface__ (nothing touches the GPU).

    Shapes: (H, W, 3|4) HWC or (3, H, W) planar CHW (HWC wins where both would fit); any strides, so a crop of a larger tensor
    keeps its parent's row pitch.  order = the frame's channel order, "bgr" or "rgb" (a 4th channel is never read or written).
    Returns a dict: data, width, height, row_stride, pixel_stride, channel_offset = byte offsets of (B, G, R) from a pixel."""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if cai is None:
        raise TypeError(f"{type(obj).__name__} has no __cuda_array_interface__: device frames only (host arrays go to submit_frame)")
    if order not in ("bgr", "rgb"):
        raise ValueError(f"order {order!r}: 'bgr' or 'rgb'")
    if cai["typestr"][1:] != "u1":
        raise ValueError(f"dtype {cai['typestr']}: frames are u8")
    shape = tuple(int(d) for d in cai["shape"])
    if len(shape) != 3:
        raise ValueError(f"shape {shape}: (H, W, 3|4) or (3, H, W)")
    strides = cai.get("strides")
    if strides is None:   # C-contiguous
        strides = (shape[1] * shape[2], shape[2], 1)
    strides = tuple(int(s) for s in strides)
    if shape[2] in (3, 4):
        (h, w, _), (rs, ps, cs) = shape, strides
    elif shape[0] == 3:
        (_, h, w), (cs, rs, ps) = shape, strides
    else:
        raise ValueError(f"shape {shape}: 3 or 4 channels, (H, W, 3|4) or (3, H, W)")
    offs = (0, cs, 2 * cs) if order == "bgr" else (2 * cs, cs, 0)
    return dict(data=int(cai["data"][0]), width=w, height=h, row_stride=rs, pixel_stride=ps, channel_offset=offs)


def _view_struct(f):
    v = rtp_frame_view()
    v.struct_size = C.sizeof(rtp_frame_view)
    v.data, v.width, v.height = f["data"], f["width"], f["height"]
    v.row_stride, v.pixel_stride = f["row_stride"], f["pixel_stride"]
    for c in range(3):
        v.channel_offset[c] = f["channel_offset"][c]
    return v


def _plane(obj, name, ndim):
    """(pointer, shape, strides, on the device?) of one u8 plane: a host numpy array or a __cuda_array_interface__ object."""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if cai is not None:
        typestr, shape, strides, ptr = cai["typestr"], cai["shape"], cai.get("strides"), int(cai["data"][0])
    elif isinstance(obj, np.ndarray):
        typestr, shape, strides, ptr = obj.dtype.str, obj.shape, obj.strides, obj.ctypes.data
    else:
        raise TypeError(f"{name}: {type(obj).__name__} is neither a numpy array nor a __cuda_array_interface__ object")
    if typestr[1:] != "u1":
        raise ValueError(f"{name}: dtype {typestr}: planes are u8")
    shape = tuple(int(d) for d in shape)
    if len(shape) != ndim or min(shape) < 1:
        raise ValueError(f"{name}: shape {shape}: " + ("(H, W)" if ndim == 2 else "(H/2, W/2, 2)"))
    if strides is None:   # C-contiguous
        strides = tuple(int(np.prod(shape[i + 1:])) for i in range(ndim))
    return ptr, shape, tuple(int(s) for s in strides), cai is not None


def yuv_view(y, u, v=None, *, interleaved_order="uv"):
    """The rtp_yuv_view fields of an 8-bit YUV frame: host numpy arrays or __cuda_array_interface__ objects (nothing touches the GPU).

    (y, u, v): planar; y is (H, W), u and v have one shape, from which the sampling is inferred — ((H+1)//2, (W+1)//2) 4:2:0,
    (H, (W+1)//2) 4:2:2, (H, W) 4:4:4.  (y, uv) with uv of shape (ch, cw, 2): interleaved pairs, NV12 (interleaved_order "uv") or
    NV21 ("vu").  (y, None): luma only.  Any row pitch (a crop keeps its parent's); luma columns must be contiguous.
    Returns a dict: y, u, v (addresses or None), width, height, chroma_shift_x, chroma_shift_y, y_stride, uv_stride, uv_pixel_stride,
    device (whether the planes are device memory)."""
    if interleaved_order not in ("uv", "vu"):
        raise ValueError(f"interleaved_order {interleaved_order!r}: 'uv' (NV12) or 'vu' (NV21)")
    yp, (h, w), (yrs, yps), dev = _plane(y, "y", 2)
    if yps != 1 and w > 1:
        raise ValueError(f"y: column stride {yps}: luma columns must be contiguous (shape (H, W))")
    f = dict(y=yp, u=None, v=None, width=w, height=h, chroma_shift_x=0, chroma_shift_y=0, y_stride=yrs, uv_stride=0, uv_pixel_stride=1,
             device=dev)
    if u is None:
        if v is not None:
            raise ValueError("v without u: pass (y, u, v), (y, uv) or (y, None)")
        return f
    if v is None:   # interleaved
        up, ushape, (urs, ups, ucs), udev = _plane(u, "uv", 3)
        if ushape[2] != 2 or (ucs, ups) != (1, 2):
            raise ValueError(f"uv: shape {ushape}, strides {(urs, ups, ucs)}: interleaved chroma is (ch, cw, 2) with pairs of neighbouring bytes")
        (ch, cw), ps, planes = ushape[:2], 2, ((up, up + 1) if interleaved_order == "uv" else (up + 1, up))
        devs = (udev,)
    else:
        up, ushape, (urs, ups), udev = _plane(u, "u", 2)
        vp_, vshape, (vrs, vps), vdev = _plane(v, "v", 2)
        if ushape != vshape:
            raise ValueError(f"u and v: shapes {ushape} and {vshape} differ")
        if ushape[0] > 1 and urs != vrs or ushape[1] > 1 and ups != vps:
            raise ValueError(f"u and v: strides {(urs, ups)} and {(vrs, vps)} differ (rtp_yuv_view has one chroma pitch)")
        if ushape[1] == 1:
            ups = 1
        if ups not in (1, 2):
            raise ValueError(f"u, v: column stride {ups}: 1 (planar) or 2")
        (ch, cw), ps, planes = ushape, ups, (up, vp_)
        devs = (udev, vdev)
    if any(d != dev for d in devs):
        raise ValueError("planes in host and in device memory mixed in one frame")
    for sx, sy in ((1, 1), (1, 0), (0, 0)):
        if cw == (w + sx) >> sx and ch == (h + sy) >> sy:
            break
    else:
        raise ValueError(f"chroma shape {(ch, cw)} for a {h} x {w} luma plane matches no supported sampling (4:2:0, 4:2:2, 4:4:4)")
    f.update(u=planes[0], v=planes[1], chroma_shift_x=sx, chroma_shift_y=sy, uv_stride=urs, uv_pixel_stride=ps)
    return f


def _yuv_struct(f):
    s = rtp_yuv_view()
    s.struct_size = C.sizeof(rtp_yuv_view)
    s.matrix = 0   # RTP_YUV_BT601_LIMITED
    s.y, s.u, s.v = f["y"], f["u"], f["v"]
    s.width, s.height = f["width"], f["height"]
    s.chroma_shift_x, s.chroma_shift_y = f["chroma_shift_x"], f["chroma_shift_y"]
    s.y_stride, s.uv_stride, s.uv_pixel_stride = f["y_stride"], f["uv_stride"], f["uv_pixel_stride"]
    return s


def convert_yuv(y, u, v=None, *, interleaved_order="uv"):
    """rtp_convert_yuv: host planes (see yuv_view) -> BGR HWC u8, BT.601 limited range — the pixels every YUV entry works on."""
    f = yuv_view(y, u, v, interleaved_order=interleaved_order)
    if f["device"]:
        raise TypeError("convert_yuv takes host arrays (device planes: Engine.convert_yuv_device)")
    out = np.empty((f["height"], f["width"], 3), np.uint8)
    s = _yuv_struct(f)
    rc = lib.rtp_convert_yuv(C.byref(s), _u8(out), out.size)
    if rc:
        raise RtpError(rc, lib.rtp_codec_last_error().decode())
    return out


def yuv_bytes(w, h, chroma=420):
    """rtp_yuv_bytes: bytes of a w x h frame's planes without pitches (chroma 420, 422, 444 or 400); 0 for bad arguments."""
    return int(lib.rtp_yuv_bytes(int(w), int(h), int(chroma)))


def convert_bgr_to_yuv(bgr, chroma=420, *, out=None, interleaved_order="uv"):
    """rtp_convert_bgr_to_yuv: a BGR HWC u8 host image (any row pitch) -> planes, BT.601 limited range — the bytes every YUV output
    of the library holds.  chroma 420, 422, 444 or 400 (luma only): returns new (y, u, v) numpy planes (u = v = None for 400).
    out = (y, u, v), (y, uv) or (y, None) as yuv_view takes them: the conversion is written into those host planes (pitched,
    interleaved, ...) instead, and `out` is returned."""
    img = np.asarray(bgr)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.strides[2] != 1 or (img.shape[1] > 1 and img.strides[1] != 3) or img.strides[0] < 0:
        img = np.ascontiguousarray(bgr, np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"shape {img.shape}: (H, W, 3)")
    h, w = img.shape[:2]
    if out is None:
        shifts = {420: (1, 1), 422: (1, 0), 444: (0, 0), 400: None}.get(int(chroma), 0)
        if shifts == 0:
            raise ValueError(f"chroma {chroma!r}: 420, 422, 444 or 400")
        y = np.empty((h, w), np.uint8)
        if shifts is None:
            out = (y, None, None)
        else:
            cs = ((h + shifts[1]) >> shifts[1], (w + shifts[0]) >> shifts[0])
            out = (y, np.empty(cs, np.uint8), np.empty(cs, np.uint8))
    planes = tuple(out) + (None,) * (3 - len(out))
    f = yuv_view(planes[0], planes[1], planes[2], interleaved_order=interleaved_order)
    if f["device"]:
        raise TypeError("convert_bgr_to_yuv takes host arrays (device frames: Engine.convert_to_yuv_device)")
    s = _yuv_struct(f)
    rc = lib.rtp_convert_bgr_to_yuv(C.cast(img.ctypes.data, C.POINTER(C.c_ubyte)), w, h, img.strides[0] if h > 1 else 3 * w, C.byref(s))
    if rc:
        raise RtpError(rc, lib.rtp_codec_last_error().decode())
    return out


VIDEO_Y4M, VIDEO_MJPEG = 1, 2   # RTP_VIDEO_*


class VideoWriter:
    """rtp_video_create: an append-only Y4M (8-bit 4:2:0) or raw MJPEG stream that Video reads back; the path may be a FIFO.

    kind: VIDEO_Y4M / VIDEO_MJPEG, or None = by the suffix (.y4m, .mjpeg / .mjpg).  fps: an int or a (num, den) pair."""

    def __init__(self, path, w, h, kind=None, fps=30):
        if kind is None:
            suffix = os.path.splitext(str(path))[1].lower()
            kind = {".y4m": VIDEO_Y4M, ".mjpeg": VIDEO_MJPEG, ".mjpg": VIDEO_MJPEG}.get(suffix)
            if kind is None:
                raise ValueError(f"{path}: the suffix names no format (.y4m, .mjpeg, .mjpg): pass kind")
        num, den = fps if isinstance(fps, (tuple, list)) else (fps, 1)
        self.h = C.c_void_p()
        self.kind, self.w, self.h_ = int(kind), int(w), int(h)
        rc = lib.rtp_video_create(str(path).encode(), self.w, self.h_, self.kind, int(num), int(den), C.byref(self.h))
        if rc:
            self.h = C.c_void_p()
            raise RtpError(rc, lib.rtp_codec_last_error().decode())

    def write_yuv(self, y, u, v=None, *, interleaved_order="uv"):
        """rtp_video_write_yuv: one 4:2:0 frame from host planes (see yuv_view; any pitches, planar or interleaved)."""
        f = yuv_view(y, u, v, interleaved_order=interleaved_order)
        if f["device"]:
            raise TypeError("VideoWriter.write_yuv takes host planes")
        s = _yuv_struct(f)
        rc = lib.rtp_video_write_yuv(self.h, C.byref(s))
        if rc:
            raise RtpError(rc, lib.rtp_codec_last_error().decode())

    def write_bgr(self, bgr, quality=98):
        """One BGR HWC u8 host frame, converted (Y4M: convert_bgr_to_yuv) or encoded (MJPEG: encode_jpeg) on the host."""
        if self.kind == VIDEO_Y4M:
            self.write_yuv(*convert_bgr_to_yuv(bgr, 420))
        else:
            self.write_jpeg(encode_jpeg(bgr, quality))

    def write_jpeg(self, data):
        """rtp_video_write_jpeg: append one JPEG file (bytes)."""
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        rc = lib.rtp_video_write_jpeg(self.h, buf, len(data))
        if rc:
            raise RtpError(rc, lib.rtp_codec_last_error().decode())

    def close(self):
        """rtp_video_finish: flush and close; raises RtpError(RTP_EIO) if a write to the stream failed."""
        if self.h:
            h, self.h = self.h, C.c_void_p()
            rc = lib.rtp_video_finish(h)
            if rc:
                raise RtpError(rc, lib.rtp_codec_last_error().decode())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def video_chroma(video):
    """rtp_video_chroma: 420, 422, 444 or 400 for a Y4M Video, 0 for anything else."""
    return int(lib.rtp_video_chroma(video.h))


def video_read_yuv(video):
    """rtp_video_read_yuv: the next Y4M frame as (y, u, v) numpy planes (u = v = None for a luma-only stream), copied out of the
    reader's buffer; None at the end of the stream."""
    s = rtp_yuv_view()
    rc = lib.rtp_video_read_yuv(video.h, C.byref(s))
    if rc == RTP_EAGAIN:
        return None
    if rc:
        raise RtpError(rc, lib.rtp_codec_last_error().decode())

    def plane(ptr, rows, cols, pitch):
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_ubyte)), shape=(rows * pitch,))
        return a.reshape(rows, pitch)[:, :cols].copy()

    y = plane(s.y, s.height, s.width, s.y_stride)
    if not s.u:
        return y, None, None
    cw, ch = (s.width + s.chroma_shift_x) >> s.chroma_shift_x, (s.height + s.chroma_shift_y) >> s.chroma_shift_y
    return y, plane(s.u, ch, cw, s.uv_stride), plane(s.v, ch, cw, s.uv_stride)


def maps_quantize_u8(v, is_paf):
    """rtp_maps_quantize_u8: the u8 format of maps mode on the host, rint(clip(v * 255, 0, 255)) for confidence and background
    channels, rint(clip((v + 1) * 127.5, 0, 255)) for PAF channels (is_paf), float32 arithmetic, ties to even, NaN -> 0."""
    a = np.ascontiguousarray(v, np.float32)
    out = np.empty(a.shape, np.uint8)
    rc = lib.rtp_maps_quantize_u8(_f(a), a.size, 1 if is_paf else 0, _u8(out))
    if rc:
        raise RtpError(rc, "rtp_maps_quantize_u8")
    return out


def maps_to_f16(v):
    """rtp_maps_to_f16: float32 -> IEEE binary16, round to nearest even (the f16 format of maps mode), as a float16 array."""
    a = np.ascontiguousarray(v, np.float32)
    out = np.empty(a.shape, np.uint16)
    rc = lib.rtp_maps_to_f16(_f(a), a.size, out.ctypes.data_as(C.POINTER(C.c_uint16)))
    if rc:
        raise RtpError(rc, "rtp_maps_to_f16")
    return out.view(np.float16)


def maps_view(obj, shape, dtype):
    """The rtp_maps_view fields of a device array that receives maps of `shape` (4 dims, leading 1s allowed to be absent in obj) and
    `dtype`, from its __cuda_array_interface__ (nothing touches the GPU): strides are taken from it, so a window of a larger
    tensor keeps its parent's pitches.  Elements of a row must be adjacent; planes (and, on the LOWRES grid, scales) evenly spaced."""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if cai is None:
        raise TypeError(f"{type(obj).__name__} has no __cuda_array_interface__: device arrays only (host arrays: peek_maps)")
    dt = np.dtype(dtype)
    if np.dtype(cai["typestr"]) != dt:
        raise ValueError(f"dtype {cai['typestr']}: the maps are {dt.str}")
    want = tuple(int(d) for d in shape)
    have = tuple(int(d) for d in cai["shape"])
    while len(have) < 4:
        have = (1,) + have
    if have != want:
        raise ValueError(f"shape {tuple(cai['shape'])}: the maps have {want}")
    strides = cai.get("strides")
    if strides is None:   # C-contiguous
        strides = tuple(int(np.prod(cai["shape"][i + 1:])) * dt.itemsize for i in range(len(cai["shape"])))
    strides = tuple(int(x) for x in strides)
    strides = (0,) * (4 - len(strides)) + strides
    ss, cs, rs, es = strides
    if want[3] > 1 and es != dt.itemsize:
        raise ValueError(f"element stride {es}: the elements of a row must be adjacent")
    if want[0] > 1 and ss != want[1] * cs:
        raise ValueError(f"scale stride {ss} is not {want[1]} channel strides of {cs}: planes must be evenly spaced")
    return dict(data=int(cai["data"][0]), channel_stride=cs, row_stride=rs)


def crops_head_parts(model):
    """The part indices of --crop_parts head: nose, eyes and ears (COCO), head and neck (MPI)."""
    parts = (C.c_int * 8)()
    n = lib.rtp_crops_head_parts(int(model), parts)
    if n < 0:
        raise RtpError(n, "bad model")
    return list(parts)[:n]


def _crops_config(crop_w, crop_h, max_crops, parts, min_score, min_parts, margin, layout):
    """(rtp_crops_config, what keeps its part list alive); layout: a CROPS_LAYOUTS name or its number"""
    cfg = rtp_crops_config()
    cfg.struct_size = C.sizeof(rtp_crops_config)
    cfg.crop_w, cfg.crop_h, cfg.max_crops = int(crop_w), int(crop_h), int(max_crops)
    cfg.min_score, cfg.min_parts, cfg.margin = float(min_score), int(min_parts), float(margin)
    if isinstance(layout, str):
        if layout not in CROPS_LAYOUTS:
            raise ValueError(f"layout {layout!r}: 'hwc_bgr' or 'chw_rgb'")
        layout = CROPS_LAYOUTS[layout]
    cfg.layout = int(layout)
    keep = None
    if parts is not None:
        keep = (C.c_int * max(len(parts), 1))(*[int(p) for p in parts])
        cfg.parts, cfg.num_parts = keep, len(parts)
    return cfg, keep


def _crops_shape(crop_w, crop_h, layout):
    return (crop_h, crop_w, 3) if layout == 0 else (3, crop_h, crop_w)


def crop_people(display_bgr, joints, num_parts, crop_w, crop_h, max_crops=MAX_PEOPLE, parts=None, min_score=0.0, min_parts=1, margin=0.0,
                layout="hwc_bgr", pixels=True):
    """rtp_crop_people, the host definition of crops mode: (boxes [n][6], crops [n][crop_h][crop_w][3] or [n][3][crop_h][crop_w]) for
    joints [people][num_parts][3] on the u8 BGR display image; n = min(people, max_crops).  pixels=False: boxes only (crops None,
    display_bgr may be None)."""
    cfg, keep = _crops_config(crop_w, crop_h, max_crops, parts, min_score, min_parts, margin, layout)
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, int(num_parts), 3)
    people = j.shape[0]
    n = min(people, max(int(max_crops), 0))
    boxes = np.zeros((n, CROP_BOX_FLOATS), np.float32)
    img, w, h = None, 1, 1
    if display_bgr is not None:
        img = np.ascontiguousarray(display_bgr, np.uint8)
        h, w = img.shape[:2]
    crops = np.zeros((n,) + _crops_shape(int(crop_w), int(crop_h), cfg.layout), np.uint8) if pixels else None
    jj = j if people else np.zeros((1, int(num_parts), 3), np.float32)
    bb = boxes if n else np.zeros((1, CROP_BOX_FLOATS), np.float32)
    rc = lib.rtp_crop_people(_u8(img) if img is not None else None, w, h, _f(jj), people, int(num_parts), C.byref(cfg), _f(bb),
                             _u8(crops if n else np.zeros(1, np.uint8)) if pixels else None)
    if rc < 0:
        raise RtpError(rc, "rtp_crop_people: an argument is out of range")
    assert rc == n
    return boxes, crops


MAX_TRACKS = 128
TRACK_REC_INTS = 4


def track_config(min_score=None, min_parts=None, min_common=None, max_cost=None, max_misses=None):
    """rtp_track_config: rtp_track_config_default's values (min_score 0, min_parts 3, min_common 2, max_cost 0.0625, max_misses 15),
    each replaced where an argument is given."""
    cfg = rtp_track_config()
    lib.rtp_track_config_default(C.byref(cfg))
    for name, v, conv in (("min_score", min_score, float), ("min_parts", min_parts, int), ("min_common", min_common, int), ("max_cost", max_cost, float),
                          ("max_misses", max_misses, int)):
        if v is not None:
            setattr(cfg, name, conv(v))
    return cfg


class TrackState:
    """rtp_track_state, the track table as plain data: num_parts, next_id, frames and numpy views id / hits / misses [128] and
    joints [128][70][3] onto the structure itself (writes through them change it).  == compares every byte's worth: the integers,
    and the joints bit for bit."""

    def __init__(self, num_parts=18, c=None):
        if c is None:
            c = rtp_track_state()
            if lib.rtp_track_state_init(C.byref(c), int(num_parts)):
                raise RtpError(RTP_EINVAL, f"rtp_track_state_init: num_parts {num_parts} outside 1 .. 70")
        self.c = c
        self.id = np.ctypeslib.as_array(c.id)
        self.hits = np.ctypeslib.as_array(c.hits)
        self.misses = np.ctypeslib.as_array(c.misses)
        self.joints = np.ctypeslib.as_array(c.joints).reshape(MAX_TRACKS, 70, 3)

    num_parts = property(lambda self: self.c.num_parts)
    next_id = property(lambda self: self.c.next_id, lambda self, v: setattr(self.c, "next_id", int(v)))
    frames = property(lambda self: self.c.frames, lambda self, v: setattr(self.c, "frames", int(v)))

    def copy(self):
        c = rtp_track_state()
        C.memmove(C.byref(c), C.byref(self.c), C.sizeof(c))
        return TrackState(c=c)

    def tobytes(self):
        return C.string_at(C.byref(self.c), C.sizeof(self.c))

    def __eq__(self, other):
        return isinstance(other, TrackState) and self.tobytes() == other.tobytes()

    def live(self):
        """{slot: id} of the live tracks"""
        return {int(t): int(self.id[t]) for t in np.nonzero(self.id)[0]}


def track_update(state, joints, num_people=None, cfg=None):
    """rtp_track_update, the host definition of tracking mode: advances `state` (a TrackState) by one frame of joints
    [people][state.num_parts][3] and returns the records [n][4] int32 {id, slot, hits, cost bits}.  num_people: the frame's count
    where it is not the array's (above 96 or negative, as the device may hold it); cfg: a track_config() (None = the defaults)."""
    cfg = cfg if cfg is not None else track_config()
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, state.num_parts, 3)
    people = j.shape[0] if num_people is None else int(num_people)
    n = min(max(people, 0), MAX_PEOPLE)
    if n > j.shape[0]:
        raise ValueError(f"num_people {people}: the array holds {j.shape[0]} people")
    recs = np.zeros((max(n, 1), TRACK_REC_INTS), np.int32)
    rc = lib.rtp_track_update(C.byref(state.c), C.byref(cfg), _f(j) if j.size else None, people, recs.ctypes.data_as(ip))
    if rc < 0:
        raise RtpError(rc, "rtp_track_update: an argument is out of range")
    assert rc == n
    return recs[:n].copy()


def format_json_tracked(joints, num_parts, frame_scale, recs=None):
    """rtp_format_json_tracked: the JSON body text (bytes) of joints [people][num_parts][3]; recs [people][4] adds "id" members."""
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, int(num_parts), 3)
    buf = C.create_string_buffer(256 + j.shape[0] * (64 + 48 * int(num_parts)))
    r = None
    if recs is not None:
        r = np.ascontiguousarray(recs, np.int32).reshape(-1, TRACK_REC_INTS)
        assert r.shape[0] >= j.shape[0]
    n = lib.rtp_format_json_tracked(buf, len(buf), _f(j) if j.size else None, j.shape[0], int(num_parts), float(frame_scale),
                                    r.ctypes.data_as(ip) if r is not None else None)
    if n < 0:
        raise RtpError(n, "rtp_format_json_tracked")
    return buf.raw[:n]


APPEARANCE_BINS = 128


def appearance_torso_parts(model):
    """rtp_appearance_torso_parts: neck, shoulders and hips (COCO), and the chest (MPI)."""
    parts = (C.c_int * 8)()
    n = lib.rtp_appearance_torso_parts(int(model), parts)
    if n < 0:
        raise RtpError(n, "bad model")
    return list(parts)[:n]


def appearance_config(parts=None, min_score=None, min_parts=None, margin=None, weight=None, max_dist=None, unknown=None, rate=None):
    """rtp_appearance_config: rtp_appearance_config_default's values (the torso parts, min_score 0, min_parts 3, margin 0, weight 0.125,
    max_dist 1, unknown 0.25, rate 32), each replaced where an argument is given.  The part list lives as long as the result."""
    cfg = rtp_appearance_config()
    lib.rtp_appearance_config_default(C.byref(cfg))
    for name, v, conv in (("min_score", min_score, float), ("min_parts", min_parts, int), ("margin", margin, float), ("weight", weight, float),
                          ("max_dist", max_dist, float), ("unknown", unknown, float), ("rate", rate, int)):
        if v is not None:
            setattr(cfg, name, conv(v))
    if parts is not None:
        cfg._keep = (C.c_int * max(len(parts), 1))(*[int(p) for p in parts])
        cfg.parts, cfg.num_parts = cfg._keep, len(parts)
    return cfg


class AppearanceState:
    """rtp_appearance_state, the descriptor table as plain data: numpy views owner [128] and desc [128][128] (Q4) onto the structure
    itself (writes through them change it).  == compares every byte."""

    def __init__(self, c=None):
        if c is None:
            c = rtp_appearance_state()
            lib.rtp_appearance_state_init(C.byref(c))
        self.c = c
        self.owner = np.ctypeslib.as_array(c.owner)
        self.desc = np.ctypeslib.as_array(c.desc).reshape(MAX_TRACKS, APPEARANCE_BINS)

    def copy(self):
        c = rtp_appearance_state()
        C.memmove(C.byref(c), C.byref(self.c), C.sizeof(c))
        return AppearanceState(c=c)

    def tobytes(self):
        return C.string_at(C.byref(self.c), C.sizeof(self.c))

    def __eq__(self, other):
        return isinstance(other, AppearanceState) and self.tobytes() == other.tobytes()


def _u16(a):
    assert a.dtype == np.uint16 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_uint16))


def appearance_describe(display_bgr, joints, num_parts, cfg=None):
    """rtp_appearance_describe, the host definition of the descriptor: (bins [n][128] uint16, valid [n] uint8) of joints
    [people][num_parts][3] on the u8 BGR display image [h][w][3]; cfg: an appearance_config() (None = the defaults)."""
    cfg = cfg if cfg is not None else appearance_config()
    img = np.ascontiguousarray(display_bgr, np.uint8)
    h, w = img.shape[:2]
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, int(num_parts), 3)
    people = j.shape[0]
    n = min(people, MAX_PEOPLE)
    bins = np.zeros((max(n, 1), APPEARANCE_BINS), np.uint16)
    valid = np.zeros(max(n, 1), np.uint8)
    rc = lib.rtp_appearance_describe(_u8(img), w, h, _f(j) if j.size else None, people, int(num_parts), C.byref(cfg), _u16(bins), _u8(valid))
    if rc < 0:
        raise RtpError(rc, "rtp_appearance_describe: an argument is out of range")
    assert rc == n
    return bins[:n].copy(), valid[:n].copy()


def track_update_appearance(track_state, appearance_state, joints, num_people=None, bins=None, valid=None, track_cfg=None, appearance_cfg=None):
    """rtp_track_update_appearance, the host definition of appearance-aided tracking: advances both states (a TrackState and an
    AppearanceState) by one frame of joints [people][num_parts][3] with their descriptors (appearance_describe's; bins None = a
    frame without a display image) and returns the records [n][4] int32 {id, slot, hits, total cost bits}."""
    tcfg = track_cfg if track_cfg is not None else track_config()
    acfg = appearance_cfg if appearance_cfg is not None else appearance_config()
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, track_state.num_parts, 3)
    people = j.shape[0] if num_people is None else int(num_people)
    n = min(max(people, 0), MAX_PEOPLE)
    if n > j.shape[0]:
        raise ValueError(f"num_people {people}: the array holds {j.shape[0]} people")
    b = v = None
    if bins is not None:
        b = np.ascontiguousarray(bins, np.uint16).reshape(-1, APPEARANCE_BINS)
        v = np.ascontiguousarray(valid, np.uint8).reshape(-1)
        if b.shape[0] < n or v.shape[0] < n:
            raise ValueError(f"{n} people, {b.shape[0]} descriptors and {v.shape[0]} valid bytes")
        if not n:
            b, v = np.zeros((1, APPEARANCE_BINS), np.uint16), np.zeros(1, np.uint8)
    recs = np.zeros((max(n, 1), TRACK_REC_INTS), np.int32)
    rc = lib.rtp_track_update_appearance(C.byref(track_state.c), C.byref(appearance_state.c), C.byref(tcfg), C.byref(acfg), _f(j) if j.size else None, people,
                                         _u16(b) if b is not None else None, _u8(v) if v is not None else None, recs.ctypes.data_as(ip))
    if rc < 0:
        raise RtpError(rc, "rtp_track_update_appearance: an argument is out of range")
    assert rc == n
    return recs[:n].copy()


SMOOTH_RENDER, SMOOTH_CROPS = 1, 2
_SMOOTH_CELL = np.dtype([("owner", np.int32), ("last", np.uint32), ("pos", np.float32, 2), ("vel", np.float32, 2), ("score", np.float32)])


def smooth_config(min_score=None, min_cutoff=None, beta=None, d_cutoff=None, max_hold=None, apply=None):
    """rtp_smooth_config: rtp_smooth_config_default's values (min_score 0, min_cutoff and d_cutoff 1/30 cycles per frame, beta 0.01,
    max_hold 5, apply 0), each replaced where an argument is given.  apply: a mask of SMOOTH_RENDER and SMOOTH_CROPS."""
    cfg = rtp_smooth_config()
    lib.rtp_smooth_config_default(C.byref(cfg))
    for name, v, conv in (("min_score", min_score, float), ("min_cutoff", min_cutoff, float), ("beta", beta, float), ("d_cutoff", d_cutoff, float),
                          ("max_hold", max_hold, int), ("apply", apply, int)):
        if v is not None:
            setattr(cfg, name, conv(v))
    return cfg


class SmoothState:
    """rtp_smooth_state, the filter table as plain data: num_parts, frames and `cell`, a numpy structured view [128][70] with the fields
    owner, last, pos [2], vel [2] and score onto the structure itself (writes through it change it).  == compares every byte."""

    def __init__(self, num_parts=18, c=None):
        if c is None:
            c = rtp_smooth_state()
            if lib.rtp_smooth_state_init(C.byref(c), int(num_parts)):
                raise RtpError(RTP_EINVAL, f"rtp_smooth_state_init: num_parts {num_parts} outside 1 .. 70")
        self.c = c
        self.cell = np.frombuffer(c, dtype=_SMOOTH_CELL, count=MAX_TRACKS * 70, offset=rtp_smooth_state.cell.offset).reshape(MAX_TRACKS, 70)   # (holds a reference to c)

    num_parts = property(lambda self: self.c.num_parts)
    frames = property(lambda self: self.c.frames, lambda self, v: setattr(self.c, "frames", int(v)))

    def copy(self):
        c = rtp_smooth_state()
        C.memmove(C.byref(c), C.byref(self.c), C.sizeof(c))
        return SmoothState(c=c)

    def tobytes(self):
        return C.string_at(C.byref(self.c), C.sizeof(self.c))

    def __eq__(self, other):
        return isinstance(other, SmoothState) and self.tobytes() == other.tobytes()


def smooth_update(state, joints, num_people=None, recs=None, cfg=None):
    """rtp_smooth_update, the host definition of smoothing mode: advances `state` (a SmoothState) by one frame of joints
    [people][state.num_parts][3] with their track records [n][4] (track_update's) and returns (joints_s [n][P][3] float32,
    vel [n][P][2] float32, flags [n][P] uint8).  num_people: the frame's count where it is not the array's (above 96 or negative, as
    the device may hold it); cfg: a smooth_config() (None = the defaults)."""
    cfg = cfg if cfg is not None else smooth_config()
    P = state.num_parts
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, P, 3)
    people = j.shape[0] if num_people is None else int(num_people)
    n = min(max(people, 0), MAX_PEOPLE)
    if n > j.shape[0]:
        raise ValueError(f"num_people {people}: the array holds {j.shape[0]} people")
    r = np.ascontiguousarray(recs if recs is not None else np.zeros((0, TRACK_REC_INTS)), np.int32).reshape(-1, TRACK_REC_INTS)
    if n > r.shape[0]:
        raise ValueError(f"{n} people, {r.shape[0]} records")
    js, vel, flags = np.zeros((max(n, 1), P, 3), np.float32), np.zeros((max(n, 1), P, 2), np.float32), np.zeros((max(n, 1), P), np.uint8)
    rc = lib.rtp_smooth_update(C.byref(state.c), C.byref(cfg), _f(j) if j.size else None, people, r.ctypes.data_as(ip) if r.size else None, _f(js), _f(vel),
                               flags.ctypes.data_as(C.POINTER(C.c_ubyte)))
    if rc < 0:
        raise RtpError(rc, "rtp_smooth_update: an argument is out of range")
    assert rc == n
    return js[:n].copy(), vel[:n].copy(), flags[:n].copy()


OVERLAY_BOX, OVERLAY_LABEL, OVERLAY_TRAIL = 1, 2, 4
OVERLAY_KIND_CAPSULE, OVERLAY_KIND_RECT, OVERLAY_KIND_LABEL = 1, 2, 3
TRAIL_MAX, OVERLAY_ITEM_INTS = 32, 9
OVERLAY_MAX_ITEMS = MAX_PEOPLE * (TRAIL_MAX + 1)
# RTP_OVERLAY_PALETTE (packed b | g << 8 | r << 16) and RTP_OVERLAY_FONT (seven row bytes per digit, bit 4 = the leftmost column)
OVERLAY_PALETTE = (0x3C14DC, 0x32CD32, 0xFF901E, 0x00D7FF, 0xD355BA, 0xD1CE00, 0x008CFF, 0x9314FF, 0x578B2E, 0xE16941, 0x20A5DA, 0xCC3299, 0xAAB220, 0x2D52A0,
                   0x7FFF00, 0xB469FF)
OVERLAY_FONT = ((0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E), (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E), (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F),
                (0x1E, 0x01, 0x01, 0x0E, 0x01, 0x01, 0x1E), (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02), (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),
                (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E), (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08), (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E),
                (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C))
_TRAIL_SLOT = np.dtype([("owner", np.int32), ("count", np.int32), ("head", np.int32), ("pts", np.int32, (TRAIL_MAX, 2))])


def overlay_config(what=None, min_score=None, box_margin=None, line_width=None, label_scale=None, trail_len=None, trail_radius=None, alpha=None):
    """rtp_overlay_config: rtp_overlay_config_default's values (everything drawn, min_score 0, box_margin 4, line_width 2, label_scale 1,
    trail_len 16, trail_radius 1, alpha 192), each replaced where an argument is given.  what: a mask of OVERLAY_BOX, OVERLAY_LABEL and
    OVERLAY_TRAIL."""
    cfg = rtp_overlay_config()
    lib.rtp_overlay_config_default(C.byref(cfg))
    for name, v, conv in (("what", what, int), ("min_score", min_score, float), ("box_margin", box_margin, int), ("line_width", line_width, int),
                          ("label_scale", label_scale, int), ("trail_len", trail_len, int), ("trail_radius", trail_radius, int), ("alpha", alpha, int)):
        if v is not None:
            setattr(cfg, name, conv(v))
    return cfg


class TrailState:
    """rtp_trail_state, the trail table as plain data: num_parts, frames and `slot`, a numpy structured view [128] with the fields owner,
    count, head and pts [32][2] onto the structure itself (writes through it change it).  == compares every byte."""

    def __init__(self, num_parts=18, c=None):
        if c is None:
            c = rtp_trail_state()
            if lib.rtp_trail_state_init(C.byref(c), int(num_parts)):
                raise RtpError(RTP_EINVAL, f"rtp_trail_state_init: num_parts {num_parts} outside 1 .. 70")
        self.c = c
        self.slot = np.frombuffer(c, dtype=_TRAIL_SLOT, count=MAX_TRACKS, offset=rtp_trail_state.slot.offset)   # (holds a reference to c)

    num_parts = property(lambda self: self.c.num_parts)
    frames = property(lambda self: self.c.frames, lambda self, v: setattr(self.c, "frames", int(v)))

    def copy(self):
        c = rtp_trail_state()
        C.memmove(C.byref(c), C.byref(self.c), C.sizeof(c))
        return TrailState(c=c)

    def tobytes(self):
        return C.string_at(C.byref(self.c), C.sizeof(self.c))

    def __eq__(self, other):
        return isinstance(other, TrailState) and self.tobytes() == other.tobytes()


def overlay_update(state, joints, num_people=None, recs=None, cfg=None, capacity=OVERLAY_MAX_ITEMS):
    """rtp_overlay_update, the host definition of overlay mode's draw list: advances `state` (a TrailState) by one frame of joints
    [people][state.num_parts][3] with their track records [n][4] and returns the frame's items [m][9] int32.  num_people: the frame's
    count where it is not the array's; cfg: an overlay_config() (None = the defaults)."""
    cfg = cfg if cfg is not None else overlay_config()
    P = state.num_parts
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, P, 3)
    people = j.shape[0] if num_people is None else int(num_people)
    n = min(max(people, 0), MAX_PEOPLE)
    if n > j.shape[0]:
        raise ValueError(f"num_people {people}: the array holds {j.shape[0]} people")
    r = np.ascontiguousarray(recs if recs is not None else np.zeros((0, TRACK_REC_INTS)), np.int32).reshape(-1, TRACK_REC_INTS)
    if n > r.shape[0]:
        raise ValueError(f"{n} people, {r.shape[0]} records")
    items = np.zeros((max(int(capacity), 1), OVERLAY_ITEM_INTS), np.int32)
    m = C.c_int(0)
    rc = lib.rtp_overlay_update(C.byref(state.c), C.byref(cfg), _f(j) if j.size else None, people, r.ctypes.data_as(ip) if r.size else None, items.ctypes.data_as(ip),
                                C.byref(m), int(capacity))
    if rc < 0:
        raise RtpError(rc, f"rtp_overlay_update: {'the frame has %d items' % m.value if rc == RTP_ERANGE else 'an argument is out of range'}")
    return items[: m.value].copy()


def overlay_draw(items, image, num_items=None):
    """rtp_overlay_draw, the host definition of overlay mode's pixels: draws items [m][9] int32 in order into `image`, a uint8 array
    [h][w][3] (BGR) whose rows may be strided, IN PLACE; returns it."""
    it = np.ascontiguousarray(items, np.int32).reshape(-1, OVERLAY_ITEM_INTS)
    m = it.shape[0] if num_items is None else int(num_items)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or image.strides[2] != 1 or image.strides[1] != 3 or not image.flags.writeable:
        raise ValueError("image: a writeable uint8 array [h][w][3] with dense rows")
    rc = lib.rtp_overlay_draw(it.ctypes.data_as(ip) if it.size else None, m, image.ctypes.data_as(C.POINTER(C.c_ubyte)), image.shape[1], image.shape[0], image.strides[0])
    if rc < 0:
        raise RtpError(rc, "rtp_overlay_draw: an argument is out of range")
    return image


REDACT_MOSAIC, REDACT_BLUR, REDACT_FILL = 0, 1, 2
REDACT_ELLIPSE, REDACT_RECT = 0, 1
REDACT_REGION_INTS, REDACT_MAX_RADIUS = 6, 4096


def redact_config(effect=None, shape=None, parts=None, min_score=None, min_parts=None, scale_q8=None, aspect_q8=None, pad=None, min_radius=None, cell=None, radius=None,
                  colour=None):
    """rtp_redact_config: rtp_redact_config_default's values (mosaic, ellipse, the model's head parts, min_score 0, min_parts 1, scale_q8 384,
    aspect_q8 320, pad 2, min_radius 4, cell 8, radius 8, black), each replaced where an argument is given.  effect: REDACT_MOSAIC, REDACT_BLUR or
    REDACT_FILL; shape: REDACT_ELLIPSE or REDACT_RECT; parts: a list of part indices (None = the model's head parts), kept alive by the
    returned structure; colour: packed b | g << 8 | r << 16."""
    cfg = rtp_redact_config()
    lib.rtp_redact_config_default(C.byref(cfg))
    for name, v, conv in (("effect", effect, int), ("shape", shape, int), ("min_score", min_score, float), ("min_parts", min_parts, int), ("scale_q8", scale_q8, int),
                          ("aspect_q8", aspect_q8, int), ("pad", pad, int), ("min_radius", min_radius, int), ("cell", cell, int), ("radius", radius, int), ("colour", colour, int)):
        if v is not None:
            setattr(cfg, name, conv(v))
    if parts is not None:
        cfg._parts = (C.c_int * max(len(parts), 1))(*[int(p) for p in parts])
        cfg.parts = C.cast(cfg._parts, C.POINTER(C.c_int))
        cfg.num_parts = len(parts)
    return cfg


def redact_regions(joints, num_parts, num_people=None, cfg=None):
    """rtp_redact_regions, the host definition of redaction mode's regions: joints [people][num_parts][3] -> records [n][6] int32
    {cx, cy, rx, ry, count, valid}.  num_people: the frame's count where it is not the array's (above 96 or negative, as the device may
    hold it); cfg: a redact_config() (None = the defaults)."""
    cfg = cfg if cfg is not None else redact_config()
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, int(num_parts), 3)
    people = j.shape[0] if num_people is None else int(num_people)
    n = min(max(people, 0), MAX_PEOPLE)
    if n > j.shape[0]:
        raise ValueError(f"num_people {people}: the array holds {j.shape[0]} people")
    regions = np.zeros((max(n, 1), REDACT_REGION_INTS), np.int32)
    rc = lib.rtp_redact_regions(_f(j) if j.size else None, people, int(num_parts), C.byref(cfg), regions.ctypes.data_as(ip))
    if rc < 0:
        raise RtpError(rc, "rtp_redact_regions: an argument is out of range")
    assert rc == n
    return regions[:n].copy()


def redact_apply(regions, image, cfg=None, num_regions=None):
    """rtp_redact_apply, the host definition of redaction mode's pixels: every pixel of `image`, a uint8 array [h][w][3] (BGR) whose rows
    may be strided, that a valid region covers is replaced by the effect's value computed from the image as it was, IN PLACE; returns it."""
    cfg = cfg if cfg is not None else redact_config()
    rg = np.ascontiguousarray(regions, np.int32).reshape(-1, REDACT_REGION_INTS)
    m = rg.shape[0] if num_regions is None else int(num_regions)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or image.strides[2] != 1 or image.strides[1] != 3 or not image.flags.writeable:
        raise ValueError("image: a writeable uint8 array [h][w][3] with dense rows")
    rc = lib.rtp_redact_apply(rg.ctypes.data_as(ip) if rg.size else None, m, C.byref(cfg), image.ctypes.data_as(C.POINTER(C.c_ubyte)), image.shape[1], image.shape[0],
                              image.strides[0])
    if rc < 0:
        raise RtpError(rc, "rtp_redact_apply: an argument is out of range")
    return image


def _stream_of(obj, stream):
    """(handle or None, torch default stream?) of the stream a device frame is ordered on.  stream: a torch.cuda.Stream, a raw
    hipStream_t as int, or None = torch's current stream of a tensor's device, else the interface's `stream` entry, else NULL."""
    if stream is not None:
        return getattr(stream, "cuda_stream", stream) or None, False
    torch = sys.modules.get("torch")   # never imported here: a torch tensor means torch is loaded already
    if torch is not None and isinstance(obj, torch.Tensor):
        h = torch.cuda.current_stream(obj.device).cuda_stream
        return h or None, not h
    s = obj.__cuda_array_interface__.get("stream")
    return (None if s in (None, 1) else s), False   # 1 = the legacy default stream: NULL


class Engine:
    """One engine per GPU worker, like one caffe::Net per processFrame thread (rtpose.cpp:1463-1472)."""

    def __init__(self, cfg=None, **kw):
        self.cfg = cfg or Config(**kw)
        self.h = C.c_void_p()
        rc = lib.rtp_engine_create(C.byref(self.cfg.c), C.byref(self.h))
        if rc:
            self.h = C.c_void_p()
            raise RtpError(rc, lib.rtp_last_error(None).decode())
        a, b, c, d, e = (C.c_int() for _ in range(5))
        lib.rtp_engine_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e))
        self.num_parts, self.max_peaks, self.heat_channels, self.low_w, self.low_h = a.value, b.value, c.value, d.value, e.value
        self.N = self.cfg.c.num_scales
        self.net_w, self.net_h = self.cfg.c.net_w, self.cfg.c.net_h

    def _chk(self, rc):
        if rc:
            raise RtpError(rc, lib.rtp_last_error(self.h).decode())

    def close(self):
        if self.h:
            lib.rtp_engine_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- hot loop
    def submit(self, x, tag=0):
        x = np.ascontiguousarray(x, np.float32)
        assert x.size == self.N * 3 * self.net_h * self.net_w
        self._chk(lib.rtp_submit(self.h, _f(x), tag))

    def submit_device(self, dptr, tag=0):
        self._chk(lib.rtp_submit_device(self.h, C.c_void_p(dptr), tag))

    def submit_frame(self, img_u8, tag=0):
        img = np.ascontiguousarray(img_u8, np.uint8)
        fs = C.c_float()
        self._chk(lib.rtp_submit_frame(self.h, img.ctypes.data_as(C.POINTER(C.c_ubyte)), img.shape[1], img.shape[0], tag, C.byref(fs)))
        return fs.value

    def submit_frame_device(self, frame, tag=0, stream=None, order="bgr"):
        """rtp_submit_frame_device: a u8 frame in device memory (see frame_view), read on the GPU in order with `stream` (see
        _stream_of).  On torch's legacy default stream the frame is made complete first (the NULL-stream contract: it must then
        stay unmodified until its collect); a side stream needs no host wait.  Returns Frame::scale."""
        v = _view_struct(frame_view(frame, order))
        st, legacy = _stream_of(frame, stream)
        if legacy:
            sys.modules["torch"].cuda.current_stream(frame.device).synchronize()
        fs = C.c_float()
        self._chk(lib.rtp_submit_frame_device(self.h, C.byref(v), st, tag, C.byref(fs)))
        return fs.value

    def submit_frame_yuv(self, y, u, v=None, tag=0, *, interleaved_order="uv"):
        """rtp_submit_frame_yuv: submit_frame of convert_yuv's pixels from HOST planes (see yuv_view); the planes cross PCIe and are
        converted on the GPU.  Returns Frame::scale."""
        f = yuv_view(y, u, v, interleaved_order=interleaved_order)
        if f["device"]:
            raise TypeError("submit_frame_yuv takes host arrays (device planes go to submit_frame_yuv_device)")
        s = _yuv_struct(f)
        fs = C.c_float()
        self._chk(lib.rtp_submit_frame_yuv(self.h, C.byref(s), tag, C.byref(fs)))
        return fs.value

    def submit_frame_yuv_device(self, y, u, v=None, tag=0, stream=None, *, interleaved_order="uv"):
        """rtp_submit_frame_yuv_device: a YUV frame in device memory (see yuv_view), read on the GPU in order with `stream` (as
        submit_frame_device).  Returns Frame::scale."""
        f = yuv_view(y, u, v, interleaved_order=interleaved_order)
        if not f["device"]:
            raise TypeError("submit_frame_yuv_device takes device planes (__cuda_array_interface__); host arrays go to submit_frame_yuv")
        s = _yuv_struct(f)
        st, legacy = _stream_of(y, stream)
        if legacy:
            sys.modules["torch"].cuda.current_stream(y.device).synchronize()
        fs = C.c_float()
        self._chk(lib.rtp_submit_frame_yuv_device(self.h, C.byref(s), st, tag, C.byref(fs)))
        return fs.value

    def convert_yuv_device(self, y, u, v, out, stream=None, order="bgr", *, interleaved_order="uv"):
        """rtp_convert_yuv_device: device planes (see yuv_view; v = None: interleaved or luma only) -> the u8 device frame `out`
        (see frame_view) of the same size, on the GPU in order with `stream`."""
        f = yuv_view(y, u, v, interleaved_order=interleaved_order)
        if not f["device"]:
            raise TypeError("convert_yuv_device takes device planes (host arrays: convert_yuv)")
        s = _yuv_struct(f)
        d = _view_struct(frame_view(out, order))
        st, _ = _stream_of(out, stream)
        self._chk(lib.rtp_convert_yuv_device(self.h, C.byref(s), C.byref(d), st))

    def decode_jpeg_device(self, data, out=None, stream=None, order="bgr"):
        """rtp_decode_jpeg_device: the pixels decode_image makes of the JPEG file `data`, decoded on the GPU into the u8 device
        frame `out` (see frame_view; None: a new (H, W, 3) torch tensor on the engine's device, torch must be imported), after the
        work queued on `stream`.  Returns (out, path) with path = JPEG_ENTROPY_DEVICE or JPEG_ENTROPY_HOST: where the Huffman
        decoding ran."""
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        if out is None:
            torch = sys.modules.get("torch")
            if torch is None:
                raise TypeError("decode_jpeg_device(out=None) allocates a torch tensor: import torch first, or pass a device frame")
            w, h = C.c_int(), C.c_int()
            rc = lib.rtp_decode_image(buf, len(data), None, 0, C.byref(w), C.byref(h))
            if rc:
                raise RtpError(rc, lib.rtp_codec_last_error().decode())
            out = torch.empty((h.value, w.value, 3), dtype=torch.uint8, device=f"cuda:{self.cfg.c.device_id}")
        v = _view_struct(frame_view(out, order))
        st, _ = _stream_of(out, stream)
        path = C.c_int(-1)
        self._chk(lib.rtp_decode_jpeg_device(self.h, buf, len(data), C.byref(v), st, C.byref(path)))
        return out, path.value

    def submit_frame_jpeg(self, data, tag=0):
        """rtp_submit_frame_jpeg: submit_frame of decode_image's pixels of the JPEG file `data`; the file's scan crosses PCIe and is
        decoded on the GPU.  Returns Frame::scale."""
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        fs = C.c_float()
        self._chk(lib.rtp_submit_frame_jpeg(self.h, buf, len(data), tag, C.byref(fs), None, None))
        return fs.value

    def debug_preprocess(self, img_u8):
        img = np.ascontiguousarray(img_u8, np.uint8)
        x = np.empty((self.N, 3, self.net_h, self.net_w), np.float32)
        disp = np.empty((self.cfg.c.disp_h, self.cfg.c.disp_w, 3), np.uint8)
        fs = C.c_float()
        self._chk(lib.rtp_debug_preprocess(self.h, img.ctypes.data_as(C.POINTER(C.c_ubyte)), img.shape[1], img.shape[0], _f(x),
                                           disp.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(fs)))
        return x, disp, fs.value

    def profile_steps(self, iters=20):
        ms = (C.c_float * 256)()
        gf = (C.c_double * 256)()
        n = lib.rtp_profile_steps(self.h, iters, ms, gf, 256)
        if n < 0:
            self._chk(n)
        return list(ms)[:n], list(gf)[:n]

    def post_from_lowres(self, lowres, peaks_in=None):
        lowres = np.ascontiguousarray(lowres, np.float32)
        peaks = np.zeros((self.num_parts, self.max_peaks + 1, 3), np.float32) if peaks_in is None else np.ascontiguousarray(peaks_in, np.float32).copy()
        joints = np.zeros((MAX_PEOPLE, self.num_parts, 3), np.float32)
        n = C.c_int()
        self._chk(lib.rtp_post_from_lowres(self.h, _f(lowres), _f(peaks), _f(joints), C.byref(n)))
        return peaks, joints[: n.value].copy(), n.value

    def render(self, display_bgr, joints, num_people, part_to_show=0, googly=0, resized=None):
        """render() of rtpose.cpp:270-299 on caller data: pose overlay (part_to_show 0) or a heat-map / PAF view of `resized`."""
        img = np.ascontiguousarray(display_bgr, np.uint8)
        assert img.shape == (self.cfg.c.disp_h, self.cfg.c.disp_w, 3), img.shape
        j = np.ascontiguousarray(joints, np.float32).reshape(-1)
        if j.size == 0:
            j = np.zeros(3, np.float32)
        res = None if resized is None else np.ascontiguousarray(resized, np.float32)
        out = np.empty_like(img)
        self._chk(lib.rtp_render(self.h, _u8(img), _f(j), int(num_people), int(part_to_show), int(googly), _f(res) if res is not None else None, _u8(out)))
        return out

    def collect_rendered(self):
        tag = C.c_uint64()
        n = C.c_int()
        joints = np.zeros((MAX_PEOPLE, self.num_parts, 3), np.float32)
        img = np.empty((self.cfg.c.disp_h, self.cfg.c.disp_w, 3), np.uint8)
        self._chk(lib.rtp_collect_rendered(self.h, C.byref(tag), _f(joints), C.byref(n), _u8(img)))
        return tag.value, n.value, joints[: n.value].copy(), img

    def collect_rendered_device(self, out, stream=None, order="bgr"):
        """rtp_collect_rendered_device: the rendered display image written into `out` (u8 device memory of disp_w x disp_h, see
        frame_view); work queued on `stream` afterwards sees it.  Returns (tag, num_people, joints)."""
        v = _view_struct(frame_view(out, order))
        st, _ = _stream_of(out, stream)
        tag = C.c_uint64()
        n = C.c_int()
        joints = np.zeros((MAX_PEOPLE, self.num_parts, 3), np.float32)
        self._chk(lib.rtp_collect_rendered_device(self.h, C.byref(tag), _f(joints), C.byref(n), C.byref(v), st))
        return tag.value, n.value, joints[: n.value].copy()

    def set_render_jpeg(self, quality):
        """rtp_set_render_jpeg: 0 off, 1..100 = every rendered frame is encoded on the GPU; collect it with collect_rendered_jpeg."""
        self._chk(lib.rtp_set_render_jpeg(self.h, int(quality)))

    def collect_rendered_jpeg(self):
        """rtp_collect_rendered_jpeg: (tag, num_people, joints, JPEG file as bytes) of the oldest frame."""
        tag = C.c_uint64()
        n = C.c_int()
        joints = np.zeros((MAX_PEOPLE, self.num_parts, 3), np.float32)
        out = np.empty(jpeg_max_bytes(self.cfg.c.disp_w, self.cfg.c.disp_h), np.uint8)
        nb = C.c_size_t()
        self._chk(lib.rtp_collect_rendered_jpeg(self.h, C.byref(tag), _f(joints), C.byref(n), _u8(out), out.size, C.byref(nb)))
        return tag.value, n.value, joints[: n.value].copy(), out[: nb.value].tobytes()

    def convert_to_yuv_device(self, frame, y, u, v=None, stream=None, order="bgr", *, interleaved_order="uv"):
        """rtp_convert_to_yuv_device: the u8 device frame `frame` (see frame_view) -> the device planes (see yuv_view; v = None:
        interleaved or luma only) of the same size, the bytes of convert_bgr_to_yuv, on the GPU in order with `stream`."""
        f = yuv_view(y, u, v, interleaved_order=interleaved_order)
        if not f["device"]:
            raise TypeError("convert_to_yuv_device takes device planes (host arrays: convert_bgr_to_yuv)")
        d = _yuv_struct(f)
        s = _view_struct(frame_view(frame, order))
        st, _ = _stream_of(frame, stream)
        self._chk(lib.rtp_convert_to_yuv_device(self.h, C.byref(s), C.byref(d), st))

    def set_render_yuv(self, chroma):
        """rtp_set_render_yuv: 0 off, 420 = every rendered frame leaves as planar 4:2:0 planes; collect with collect_rendered_yuv."""
        self._chk(lib.rtp_set_render_yuv(self.h, int(chroma)))

    def collect_rendered_yuv(self):
        """rtp_collect_rendered_yuv: (tag, joints, y, u, v) of the oldest frame: joints of the people found, and the rendered
        frame's planes (views of one buffer laid out as a Y4M FRAME payload)."""
        tag = C.c_uint64()
        n = C.c_int()
        joints = np.zeros((MAX_PEOPLE, self.num_parts, 3), np.float32)
        w, h = self.cfg.c.disp_w, self.cfg.c.disp_h
        cw, ch = (w + 1) // 2, (h + 1) // 2
        buf = np.empty(yuv_bytes(w, h, 420), np.uint8)
        self._chk(lib.rtp_collect_rendered_yuv(self.h, C.byref(tag), _f(joints), C.byref(n), _u8(buf), buf.size))
        y = buf[: w * h].reshape(h, w)
        u = buf[w * h: w * h + cw * ch].reshape(ch, cw)
        v = buf[w * h + cw * ch:].reshape(ch, cw)
        return tag.value, joints[: n.value].copy(), y, u, v

    def collect_rendered_yuv_device(self, y, u, v=None, stream=None, *, interleaved_order="uv"):
        """rtp_collect_rendered_yuv_device: the rendered display image converted into the caller's device planes (disp_w x disp_h,
        see yuv_view: e.g. a pitched NV12 surface); work queued on `stream` afterwards sees them.  Returns (tag, num_people, joints)."""
        f = yuv_view(y, u, v, interleaved_order=interleaved_order)
        if not f["device"]:
            raise TypeError("collect_rendered_yuv_device takes device planes (host planes: collect_rendered_yuv)")
        s = _yuv_struct(f)
        st, _ = _stream_of(y, stream)
        tag = C.c_uint64()
        n = C.c_int()
        joints = np.zeros((MAX_PEOPLE, self.num_parts, 3), np.float32)
        self._chk(lib.rtp_collect_rendered_yuv_device(self.h, C.byref(tag), _f(joints), C.byref(n), C.byref(s), st))
        return tag.value, n.value, joints[: n.value].copy()

    # ---- maps mode
    def set_maps_output(self, grid="net", fmt="u8", channels=None):
        """rtp_set_maps_output: every frame's chosen maps leave the engine (peek_maps / peek_maps_device in front of the frame's
        collect).  grid "net" ([nch][net_h][net_w], the values of resize()) or "lowres" ([N][nch][low_h][low_w], the values of
        forward_heatmaps()); fmt "f32", "f16" or "u8"; channels: indices into the heat channels in output order (None = all).
        grid=None switches the mode off.  Arguments are checked here, before the library is called."""
        if grid is None:
            self._chk(lib.rtp_set_maps_output(self.h, None))
            return
        if grid not in MAPS_GRIDS:
            raise ValueError(f"grid {grid!r}: 'net' or 'lowres'")
        if fmt not in MAPS_FORMATS:
            raise ValueError(f"fmt {fmt!r}: 'f32', 'f16' or 'u8'")
        cfg = rtp_maps_config()
        cfg.struct_size = C.sizeof(rtp_maps_config)
        cfg.grid, cfg.format = MAPS_GRIDS[grid], MAPS_FORMATS[fmt]
        if channels is not None:
            ch = [int(c) for c in channels]
            if not 1 <= len(ch) <= MAX_NUM_PARTS:
                raise ValueError(f"{len(ch)} channels: 1 .. {MAX_NUM_PARTS}")
            bad = [c for c in ch if not 0 <= c < self.heat_channels]
            if bad:
                raise ValueError(f"channels {bad} outside [0, {self.heat_channels})")
            arr = (C.c_int * len(ch))(*ch)
            cfg.channels, cfg.num_channels = arr, len(ch)
        self._chk(lib.rtp_set_maps_output(self.h, C.byref(cfg)))

    def maps_info(self):
        """rtp_maps_info: (shape of one frame's maps as 4 ints, numpy dtype, bytes)."""
        shape = (C.c_int * 4)()
        fmt = C.c_int()
        nb = C.c_size_t()
        rc = lib.rtp_maps_info(self.h, shape, C.byref(fmt), C.byref(nb))
        if rc:
            raise RtpError(rc, "maps mode is off (set_maps_output)")
        return tuple(shape), np.dtype(_MAPS_DTYPES[fmt.value]), nb.value

    def peek_maps(self, out=None):
        """rtp_peek_maps: (tag, maps) of the oldest frame in flight, which stays in flight: collect it afterwards.  out: a
        C-contiguous array of the shape and dtype of maps_info to fill (a loop that reuses one spares a fresh allocation per frame)."""
        shape, dt, nb = self.maps_info()
        if out is None:
            out = np.empty(shape, dt)
        elif not (isinstance(out, np.ndarray) and out.shape == shape and out.dtype == dt and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]):
            raise ValueError(f"out must be a writeable C-contiguous {dt} array of shape {shape}")
        tag = C.c_uint64()
        self._chk(lib.rtp_peek_maps(self.h, C.byref(tag), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return tag.value, out

    def peek_maps_device(self, out, stream=None):
        """rtp_peek_maps_device: the oldest frame's maps written into `out` (a device array of the shape and dtype of maps_info,
        leading 1s optional, any pitches: see maps_view); work queued on `stream` afterwards sees them.  Returns the tag."""
        shape, dt, _ = self.maps_info()
        f = maps_view(out, shape, dt)
        v = rtp_maps_view()
        v.struct_size = C.sizeof(rtp_maps_view)
        v.data, v.channel_stride, v.row_stride = f["data"], f["channel_stride"], f["row_stride"]
        st, _ = _stream_of(out, stream)
        tag = C.c_uint64()
        self._chk(lib.rtp_peek_maps_device(self.h, C.byref(tag), C.byref(v), st))
        return tag.value

    def maps_from_lowres(self, lowres):
        """rtp_maps_from_lowres: the maps of the current mode for the given low-res maps (parity tap, idle engine)."""
        lowres = np.ascontiguousarray(lowres, np.float32)
        assert lowres.shape == (self.N, self.heat_channels, self.low_h, self.low_w), lowres.shape
        shape, dt, _ = self.maps_info()
        out = np.empty(shape, dt)
        self._chk(lib.rtp_maps_from_lowres(self.h, _f(lowres), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    # ---- crops mode
    def set_crops_output(self, crop_w=None, crop_h=None, max_crops=16, parts=None, min_score=0.0, min_parts=1, margin=0.0, layout="hwc_bgr"):
        """rtp_set_crops_output: every frame's per-person boxes and fixed-size crops of the display image leave the engine
        (peek_crops / peek_crops_device in front of the frame's collect).  parts: the part indices that span a box (None = all,
        crops_head_parts(model) = the head); a part counts when its score > min_score; fewer than min_parts counting parts: no
        box; margin: every side moves out by margin * max(width, height).  crop_w=None switches the mode off."""
        if crop_w is None:
            self._chk(lib.rtp_set_crops_output(self.h, None))
            return
        cfg, keep = _crops_config(crop_w, crop_h, max_crops, parts, min_score, min_parts, margin, layout)
        self._chk(lib.rtp_set_crops_output(self.h, C.byref(cfg)))

    def crops_info(self):
        """rtp_crops_info: dict(crop_w, crop_h, max_crops, layout, crop_bytes, shape of one crop)."""
        w, h, m, lay = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        nb = C.c_size_t()
        rc = lib.rtp_crops_info(self.h, C.byref(w), C.byref(h), C.byref(m), C.byref(lay), C.byref(nb))
        if rc:
            raise RtpError(rc, "crops mode is off (set_crops_output)")
        return dict(crop_w=w.value, crop_h=h.value, max_crops=m.value, layout=lay.value, crop_bytes=nb.value,
                    shape=_crops_shape(w.value, h.value, lay.value))

    def peek_crops(self, pixels=True):
        """rtp_peek_crops: (tag, boxes [n][6], crops [n] + shape, or None for a frame without a display image or pixels=False) of
        the oldest frame in flight, which stays in flight: collect it afterwards."""
        info = self.crops_info()
        cap = info["max_crops"]
        boxes = np.zeros((cap, CROP_BOX_FLOATS), np.float32)
        crops = np.zeros((cap,) + info["shape"], np.uint8) if pixels else None
        tag = C.c_uint64()
        n, has = C.c_int(), C.c_int()
        self._chk(lib.rtp_peek_crops(self.h, C.byref(tag), _f(boxes), C.byref(n), _u8(crops) if pixels else None, cap, C.byref(has)))
        return tag.value, boxes[: n.value].copy(), (crops[: n.value].copy() if pixels and has.value else None)

    def peek_crops_device(self, out, stream=None):
        """rtp_peek_crops_device: the oldest frame's crops written into `out`, a u8 device array ([max_crops] + the crop's shape, the
        crops evenly spaced, each one dense: a window of a larger tensor keeps its stride); work queued on `stream` afterwards
        sees them.  Returns (tag, boxes [n][6])."""
        info = self.crops_info()
        cai = getattr(out, "__cuda_array_interface__", None)
        if cai is None:
            raise TypeError(f"{type(out).__name__} has no __cuda_array_interface__: device arrays only (host arrays: peek_crops)")
        want = (info["max_crops"],) + info["shape"]
        if np.dtype(cai["typestr"]) != np.uint8 or tuple(int(d) for d in cai["shape"]) != want:
            raise ValueError(f"{cai['typestr']} {tuple(cai['shape'])}: the crops are uint8 {want}")
        strides = cai.get("strides")
        dense = tuple(int(np.prod(want[i + 1:])) for i in range(4))
        strides = dense if strides is None else tuple(int(x) for x in strides)
        if strides[1:] != dense[1:]:
            raise ValueError(f"strides {strides}: every crop must be dense ({dense[1:]})")
        v = rtp_crops_view()
        v.struct_size = C.sizeof(rtp_crops_view)
        v.data, v.crop_stride = int(cai["data"][0]), strides[0]
        st, _ = _stream_of(out, stream)
        boxes = np.zeros((info["max_crops"], CROP_BOX_FLOATS), np.float32)
        tag = C.c_uint64()
        n = C.c_int()
        self._chk(lib.rtp_peek_crops_device(self.h, C.byref(tag), _f(boxes), C.byref(n), info["max_crops"], C.byref(v), st))
        return tag.value, boxes[: n.value].copy()

    # ---- tracking mode
    def set_tracking(self, cfg=True, **kw):
        """rtp_set_tracking: every submitted frame's people are associated with the engine's track table; peek_tracks in front of the
        frame's collect gives the records.  cfg: a track_config(), True (= track_config(**kw)) or None / False (off: the state is
        discarded).  Off -> on starts from an empty state; a new cfg while the mode is on keeps it."""
        if cfg is None or cfg is False:
            self._chk(lib.rtp_set_tracking(self.h, None))
            return
        if cfg is True:
            cfg = track_config(**kw)
        self._chk(lib.rtp_set_tracking(self.h, C.byref(cfg)))

    def track_reset(self):
        """rtp_track_reset: an empty table (next_id 1); idle engine."""
        self._chk(lib.rtp_track_reset(self.h))

    def track_state(self):
        """rtp_track_get_state: the engine's table as a TrackState; idle engine."""
        st = TrackState(self.num_parts)
        self._chk(lib.rtp_track_get_state(self.h, C.byref(st.c)))
        return st

    def set_track_state(self, state):
        """rtp_track_set_state: the engine's table becomes a copy of `state` (a TrackState of the engine's num_parts); idle engine."""
        self._chk(lib.rtp_track_set_state(self.h, C.byref(state.c)))

    def peek_tracks(self, capacity=MAX_PEOPLE):
        """rtp_peek_tracks: (tag, records [n][4] int32 {id, slot, hits, cost bits}) of the oldest frame in flight, which stays in
        flight (follow with a collect)."""
        recs = np.zeros((max(int(capacity), 1), TRACK_REC_INTS), np.int32)
        tag, n = C.c_uint64(0), C.c_int(0)
        self._chk(lib.rtp_peek_tracks(self.h, C.byref(tag), recs.ctypes.data_as(ip), C.byref(n), int(capacity)))
        return tag.value, recs[: n.value].copy()

    def track_from_joints(self, joints, num_people=None):
        """rtp_track_from_joints: the async path's kernel on joints [people][num_parts][3] (idle engine); the engine's table advances
        by one frame.  num_people: what the device is told where it is not the array's count (above 96 or negative, which the kernel
        clamps).  Returns the records [n][4]."""
        j = np.ascontiguousarray(joints, np.float32).reshape(-1, self.num_parts, 3)
        people = j.shape[0] if num_people is None else int(num_people)
        cap = min(max(people, 0), MAX_PEOPLE)
        if cap > j.shape[0]:
            raise ValueError(f"num_people {people}: the array holds {j.shape[0]} people")
        recs = np.zeros((max(cap, 1), TRACK_REC_INTS), np.int32)
        n = C.c_int(0)
        self._chk(lib.rtp_track_from_joints(self.h, _f(j) if j.size else None, people, recs.ctypes.data_as(ip), C.byref(n), cap))
        return recs[: n.value].copy()

    # ---- appearance-aided tracking
    def set_track_appearance(self, cfg=True, **kw):
        """rtp_set_track_appearance (tracking mode must be on): every submitted frame's people get a colour descriptor from the frame's
        display image, the track kernel's cost gains the appearance term, and peek_appearance in front of the frame's collect gives the
        descriptors.  cfg: an appearance_config(), True (= appearance_config(**kw)) or None / False (off: the descriptor table is
        discarded).  Off -> on starts from an empty descriptor table; a new cfg while the mode is on keeps it."""
        if cfg is None or cfg is False:
            self._chk(lib.rtp_set_track_appearance(self.h, None))
            return
        if cfg is True:
            cfg = appearance_config(**kw)
        self._chk(lib.rtp_set_track_appearance(self.h, C.byref(cfg)))

    def appearance_reset(self):
        """rtp_appearance_reset: an empty descriptor table; idle engine."""
        self._chk(lib.rtp_appearance_reset(self.h))

    def appearance_state(self):
        """rtp_appearance_get_state: the engine's descriptor table as an AppearanceState; idle engine."""
        st = AppearanceState()
        self._chk(lib.rtp_appearance_get_state(self.h, C.byref(st.c)))
        return st

    def set_appearance_state(self, state):
        """rtp_appearance_set_state: the engine's descriptor table becomes a copy of `state` (an AppearanceState); idle engine."""
        self._chk(lib.rtp_appearance_set_state(self.h, C.byref(state.c)))

    def peek_appearance(self, capacity=MAX_PEOPLE):
        """rtp_peek_appearance: (tag, bins [n][128] uint16, valid [n] uint8) of the oldest frame in flight, which stays in flight."""
        bins = np.zeros((max(int(capacity), 1), APPEARANCE_BINS), np.uint16)
        valid = np.zeros(max(int(capacity), 1), np.uint8)
        tag, n = C.c_uint64(0), C.c_int(0)
        self._chk(lib.rtp_peek_appearance(self.h, C.byref(tag), _u16(bins), _u8(valid), C.byref(n), int(capacity)))
        return tag.value, bins[: n.value].copy(), valid[: n.value].copy()

    def _appearance_tap_args(self, display_bgr, joints, num_people):
        img = None
        if display_bgr is not None:
            img = np.ascontiguousarray(display_bgr, np.uint8)
            if img.shape != (self.cfg.c.disp_h, self.cfg.c.disp_w, 3):
                raise ValueError(f"display image {img.shape}: the engine's display is {(self.cfg.c.disp_h, self.cfg.c.disp_w, 3)}")
        j = np.ascontiguousarray(joints, np.float32).reshape(-1, self.num_parts, 3)
        people = j.shape[0] if num_people is None else int(num_people)
        cap = min(max(people, 0), MAX_PEOPLE)
        if cap > j.shape[0]:
            raise ValueError(f"num_people {people}: the array holds {j.shape[0]} people")
        return img, j, people, cap

    def appearance_from_joints(self, display_bgr, joints, num_people=None):
        """rtp_appearance_from_joints: the async path's describe kernel on the display image [disp_h][disp_w][3] (None: a frame without
        one) and joints [people][num_parts][3] (idle engine); no table is touched.  Returns (bins [n][128], valid [n])."""
        img, j, people, cap = self._appearance_tap_args(display_bgr, joints, num_people)
        bins, valid = np.zeros((max(cap, 1), APPEARANCE_BINS), np.uint16), np.zeros(max(cap, 1), np.uint8)
        n = C.c_int(0)
        self._chk(lib.rtp_appearance_from_joints(self.h, _u8(img) if img is not None else None, _f(j) if j.size else None, people, _u16(bins), _u8(valid), C.byref(n), cap))
        return bins[: n.value].copy(), valid[: n.value].copy()

    def track_from_frame(self, display_bgr, joints, num_people=None):
        """rtp_track_from_frame: the async path's describe and track kernels on the display image (None: a frame without one) and joints
        (idle engine); both of the engine's tables advance by one frame.  Returns (records [n][4], bins [n][128], valid [n])."""
        img, j, people, cap = self._appearance_tap_args(display_bgr, joints, num_people)
        recs = np.zeros((max(cap, 1), TRACK_REC_INTS), np.int32)
        bins, valid = np.zeros((max(cap, 1), APPEARANCE_BINS), np.uint16), np.zeros(max(cap, 1), np.uint8)
        n = C.c_int(0)
        self._chk(lib.rtp_track_from_frame(self.h, _u8(img) if img is not None else None, _f(j) if j.size else None, people, recs.ctypes.data_as(ip), _u16(bins),
                                           _u8(valid), C.byref(n), cap))
        return recs[: n.value].copy(), bins[: n.value].copy(), valid[: n.value].copy()

    # ---- smoothing mode
    def set_smoothing(self, cfg=True, **kw):
        """rtp_set_smoothing (tracking mode must be on): every submitted frame's tracked people go through the engine's filter table;
        peek_smoothed in front of the frame's collect gives the result.  cfg: a smooth_config(), True (= smooth_config(**kw)) or None /
        False (off: the state is discarded).  Off -> on starts from an empty state; a new cfg while the mode is on keeps it."""
        if cfg is None or cfg is False:
            self._chk(lib.rtp_set_smoothing(self.h, None))
            return
        if cfg is True:
            cfg = smooth_config(**kw)
        self._chk(lib.rtp_set_smoothing(self.h, C.byref(cfg)))

    def smooth_reset(self):
        """rtp_smooth_reset: an empty filter table; idle engine."""
        self._chk(lib.rtp_smooth_reset(self.h))

    def smooth_state(self):
        """rtp_smooth_get_state: the engine's filter table as a SmoothState; idle engine."""
        st = SmoothState(self.num_parts)
        self._chk(lib.rtp_smooth_get_state(self.h, C.byref(st.c)))
        return st

    def set_smooth_state(self, state):
        """rtp_smooth_set_state: the engine's filter table becomes a copy of `state` (a SmoothState of the engine's num_parts); idle engine."""
        self._chk(lib.rtp_smooth_set_state(self.h, C.byref(state.c)))

    def peek_smoothed(self, capacity=MAX_PEOPLE):
        """rtp_peek_smoothed: (tag, joints_s [n][P][3], vel [n][P][2], flags [n][P] uint8) of the oldest frame in flight, which stays in
        flight (follow with a collect)."""
        P, cap = self.num_parts, max(int(capacity), 1)
        js, vel, flags = np.zeros((cap, P, 3), np.float32), np.zeros((cap, P, 2), np.float32), np.zeros((cap, P), np.uint8)
        tag, n = C.c_uint64(0), C.c_int(0)
        self._chk(lib.rtp_peek_smoothed(self.h, C.byref(tag), _f(js), _f(vel), flags.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(n), int(capacity)))
        return tag.value, js[: n.value].copy(), vel[: n.value].copy(), flags[: n.value].copy()

    def smooth_from_joints(self, joints, num_people=None):
        """rtp_smooth_from_joints: the async path's track and smooth kernels on joints [people][num_parts][3] (idle engine); both of the
        engine's tables advance by one frame.  num_people: what the device is told where it is not the array's count.  Returns
        (records [n][4], joints_s, vel, flags)."""
        P = self.num_parts
        j = np.ascontiguousarray(joints, np.float32).reshape(-1, P, 3)
        people = j.shape[0] if num_people is None else int(num_people)
        cap = min(max(people, 0), MAX_PEOPLE)
        if cap > j.shape[0]:
            raise ValueError(f"num_people {people}: the array holds {j.shape[0]} people")
        m = max(cap, 1)
        recs = np.zeros((m, TRACK_REC_INTS), np.int32)
        js, vel, flags = np.zeros((m, P, 3), np.float32), np.zeros((m, P, 2), np.float32), np.zeros((m, P), np.uint8)
        n = C.c_int(0)
        self._chk(lib.rtp_smooth_from_joints(self.h, _f(j) if j.size else None, people, recs.ctypes.data_as(ip), _f(js), _f(vel),
                                             flags.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(n), cap))
        return recs[: n.value].copy(), js[: n.value].copy(), vel[: n.value].copy(), flags[: n.value].copy()

    # ---- overlay mode
    def set_track_overlay(self, cfg=True, **kw):
        """rtp_set_track_overlay (tracking mode must be on, Config.render >= 1): every submitted frame's rendered image gets a box, an id
        label and a fading trail per tracked person before it is exported; peek_overlay_items in front of the frame's collect gives the
        draw list.  cfg: an overlay_config(), True (= overlay_config(**kw)) or None / False (off: the trail table is discarded).  Off -> on
        starts from an empty table; a new cfg while the mode is on keeps it."""
        if cfg is None or cfg is False:
            self._chk(lib.rtp_set_track_overlay(self.h, None))
            return
        if cfg is True:
            cfg = overlay_config(**kw)
        self._chk(lib.rtp_set_track_overlay(self.h, C.byref(cfg)))

    def overlay_reset(self):
        """rtp_overlay_reset: an empty trail table; idle engine."""
        self._chk(lib.rtp_overlay_reset(self.h))

    def overlay_state(self):
        """rtp_overlay_get_state: the engine's trail table as a TrailState; idle engine."""
        st = TrailState(self.num_parts)
        self._chk(lib.rtp_overlay_get_state(self.h, C.byref(st.c)))
        return st

    def set_overlay_state(self, state):
        """rtp_overlay_set_state: the engine's trail table becomes a copy of `state` (a TrailState of the engine's num_parts); idle engine."""
        self._chk(lib.rtp_overlay_set_state(self.h, C.byref(state.c)))

    def peek_overlay_items(self, capacity=OVERLAY_MAX_ITEMS):
        """rtp_peek_overlay_items: (tag, items [m][9] int32) of the oldest frame in flight, which stays in flight (follow with a collect)."""
        items = np.zeros((max(int(capacity), 1), OVERLAY_ITEM_INTS), np.int32)
        tag, m = C.c_uint64(0), C.c_int(0)
        self._chk(lib.rtp_peek_overlay_items(self.h, C.byref(tag), items.ctypes.data_as(ip), C.byref(m), int(capacity)))
        return tag.value, items[: m.value].copy()

    def overlay_from_joints(self, joints, num_people=None, image=None, capacity=OVERLAY_MAX_ITEMS):
        """rtp_overlay_from_joints: the async path's track, overlay_update and overlay_draw kernels on joints [people][num_parts][3] (idle
        engine); the track table and the trail table advance by one frame.  image: a uint8 array [h][w][3] up to the display size, or
        None (no drawing).  Returns (records [n][4], items [m][9], the image with the drawing or None)."""
        P = self.num_parts
        j = np.ascontiguousarray(joints, np.float32).reshape(-1, P, 3)
        people = j.shape[0] if num_people is None else int(num_people)
        n = min(max(people, 0), MAX_PEOPLE)
        if n > j.shape[0]:
            raise ValueError(f"num_people {people}: the array holds {j.shape[0]} people")
        recs = np.zeros((max(n, 1), TRACK_REC_INTS), np.int32)
        items = np.zeros((max(int(capacity), 1), OVERLAY_ITEM_INTS), np.int32)
        img = None if image is None else np.ascontiguousarray(image, np.uint8).copy()
        h, w = (0, 0) if img is None else img.shape[:2]
        m = C.c_int(0)
        self._chk(lib.rtp_overlay_from_joints(self.h, _f(j) if j.size else None, people, None if img is None else img.ctypes.data_as(C.POINTER(C.c_ubyte)), w, h,
                                              recs.ctypes.data_as(ip), items.ctypes.data_as(ip), C.byref(m), int(capacity)))
        return recs[:n].copy(), items[: m.value].copy(), img

    # ---- redaction mode
    def set_redaction(self, cfg=True, **kw):
        """rtp_set_redaction (Config.render >= 1; tracking mode is not needed): every submitted frame's rendered image has a region around
        each person's listed parts (the head's by default) mosaicked, blurred or filled before it is exported; peek_redactions in front of
        the frame's collect gives the records.  cfg: a redact_config(), True (= redact_config(**kw)) or None / False (off).  Crops mode and
        maps mode keep handing out un-redacted data."""
        if cfg is None or cfg is False:
            self._chk(lib.rtp_set_redaction(self.h, None))
            return
        if cfg is True:
            cfg = redact_config(**kw)
        self._chk(lib.rtp_set_redaction(self.h, C.byref(cfg)))

    def redaction_info(self):
        """rtp_redaction_info: the current configuration as a dict of rtp_redact_config's fields, parts = the list."""
        cfg = rtp_redact_config()
        parts = (C.c_int * 70)()
        rc = lib.rtp_redaction_info(self.h, C.byref(cfg), parts)
        if rc:
            raise RtpError(rc, "redaction mode is off (set_redaction)")
        d = {name: getattr(cfg, name) for name, _ in rtp_redact_config._fields_ if name not in ("struct_size", "parts", "num_parts")}
        d["parts"] = list(parts)[: cfg.num_parts]
        return d

    def peek_redactions(self, capacity=MAX_PEOPLE):
        """rtp_peek_redactions: (tag, records [n][6] int32) of the oldest frame in flight, which stays in flight (follow with a collect)."""
        regions = np.zeros((max(int(capacity), 1), REDACT_REGION_INTS), np.int32)
        tag, n = C.c_uint64(0), C.c_int(0)
        self._chk(lib.rtp_peek_redactions(self.h, C.byref(tag), regions.ctypes.data_as(ip), C.byref(n), int(capacity)))
        return tag.value, regions[: n.value].copy()

    def redact_from_joints(self, joints, num_people=None, image=None, capacity=MAX_PEOPLE):
        """rtp_redact_from_joints: the async path's redact_regions and redact_apply kernels on joints [people][num_parts][3] (idle engine,
        mode on).  image: a uint8 array [h][w][3] up to the display size, or None (regions only).  Returns (records [n][6], the redacted
        image or None)."""
        P = self.num_parts
        j = np.ascontiguousarray(joints, np.float32).reshape(-1, P, 3)
        people = j.shape[0] if num_people is None else int(num_people)
        n = min(max(people, 0), MAX_PEOPLE)
        if n > j.shape[0]:
            raise ValueError(f"num_people {people}: the array holds {j.shape[0]} people")
        regions = np.zeros((max(int(capacity), 1), REDACT_REGION_INTS), np.int32)
        img = None if image is None else np.ascontiguousarray(image, np.uint8).copy()
        h, w = (0, 0) if img is None else img.shape[:2]
        m = C.c_int(0)
        self._chk(lib.rtp_redact_from_joints(self.h, _f(j) if j.size else None, people, None if img is None else img.ctypes.data_as(C.POINTER(C.c_ubyte)), w, h,
                                             regions.ctypes.data_as(ip), C.byref(m), int(capacity)))
        return regions[: m.value].copy(), img

    def crops_from_joints(self, display_bgr, joints, pixels=True):
        """rtp_crops_from_joints: (boxes, crops) of the current mode for the given display image and joints [people][num_parts][3]
        through the kernel of the async path (parity tap, idle engine)."""
        info = self.crops_info()
        img = np.ascontiguousarray(display_bgr, np.uint8)
        assert img.shape == (self.cfg.c.disp_h, self.cfg.c.disp_w, 3), img.shape
        j = np.ascontiguousarray(joints, np.float32).reshape(-1, self.num_parts, 3)
        people = j.shape[0]
        cap = info["max_crops"]
        boxes = np.zeros((cap, CROP_BOX_FLOATS), np.float32)
        crops = np.zeros((cap,) + info["shape"], np.uint8) if pixels else None
        n = C.c_int()
        jj = j if people else np.zeros((1, self.num_parts, 3), np.float32)
        self._chk(lib.rtp_crops_from_joints(self.h, _u8(img), _f(jj), people, _f(boxes), C.byref(n), _u8(crops) if pixels else None, cap))
        return boxes[: n.value].copy(), (crops[: n.value].copy() if pixels else None)

    def encode_jpeg_device(self, obj, quality=98, stream=None, order="bgr"):
        """rtp_encode_jpeg_device: encode_jpeg of a u8 frame in device memory (see frame_view), on the GPU after the work queued on
        `stream` (see _stream_of) -> bytes."""
        f = frame_view(obj, order)
        v = _view_struct(f)
        st, _ = _stream_of(obj, stream)
        out = np.empty(jpeg_max_bytes(f["width"], f["height"]), np.uint8)
        nb = C.c_size_t()
        self._chk(lib.rtp_encode_jpeg_device(self.h, C.byref(v), int(quality), st, _u8(out), out.size, C.byref(nb)))
        return out[: nb.value].tobytes()

    def flush(self):
        self._chk(lib.rtp_flush(self.h))

    def collect(self):
        tag = C.c_uint64()
        n = C.c_int()
        joints = np.zeros((MAX_PEOPLE, self.num_parts, 3), np.float32)
        self._chk(lib.rtp_collect(self.h, C.byref(tag), _f(joints), C.byref(n)))
        return tag.value, n.value, joints[: n.value].copy()

    def in_flight(self):
        return lib.rtp_in_flight(self.h)

    # ---- thresholds / scales
    def set_thresholds(self, nms_threshold, inter_threshold, inter_min_above, min_subset_cnt, min_subset_score):
        self._chk(lib.rtp_set_thresholds(self.h, nms_threshold, inter_threshold, inter_min_above, min_subset_cnt, min_subset_score))

    def get_thresholds(self):
        a, b, e = C.c_float(), C.c_float(), C.c_float()
        c, d = C.c_int(), C.c_int()
        self._chk(lib.rtp_get_thresholds(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)))
        return dict(nms_threshold=a.value, inter_threshold=b.value, inter_min_above=c.value, min_subset_cnt=d.value,
                    min_subset_score=e.value)

    def set_scales(self, start_scale, scale_gap):
        self._chk(lib.rtp_set_scales(self.h, start_scale, scale_gap))

    # ---- parity taps
    def forward_heatmaps(self, x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty((self.N, self.heat_channels, self.low_h, self.low_w), np.float32)
        self._chk(lib.rtp_forward_heatmaps(self.h, _f(x), _f(out)))
        return out

    def resize(self, lowres):
        lowres = np.ascontiguousarray(lowres, np.float32)
        assert lowres.shape == (self.N, self.heat_channels, self.low_h, self.low_w)
        out = np.empty((self.heat_channels, self.net_h, self.net_w), np.float32)
        self._chk(lib.rtp_resize(self.h, _f(lowres), _f(out)))
        return out

    def nms(self, resized, peaks_init=None):
        resized = np.ascontiguousarray(resized, np.float32).reshape(self.heat_channels, self.net_h, self.net_w)
        peaks = np.zeros((self.num_parts, self.max_peaks + 1, 3), np.float32) if peaks_init is None else np.ascontiguousarray(peaks_init, np.float32).copy()
        self._chk(lib.rtp_nms(self.h, _f(resized), _f(peaks)))
        return peaks

    def connect(self, resized, peaks):
        resized = np.ascontiguousarray(resized, np.float32).reshape(self.heat_channels, self.net_h, self.net_w)
        peaks = np.ascontiguousarray(peaks, np.float32)
        joints = np.zeros((MAX_PEOPLE, self.num_parts, 3), np.float32)
        n = C.c_int()
        self._chk(lib.rtp_connect(self.h, _f(resized), _f(peaks), _f(joints), C.byref(n)))
        return n.value, joints

    def forward_debug(self, x):
        x = np.ascontiguousarray(x, np.float32)
        lowres = np.empty((self.N, self.heat_channels, self.low_h, self.low_w), np.float32)
        resized = np.empty((self.heat_channels, self.net_h, self.net_w), np.float32)
        peaks = np.empty((self.num_parts, self.max_peaks + 1, 3), np.float32)
        joints = np.zeros((MAX_PEOPLE, self.num_parts, 3), np.float32)
        n = C.c_int()
        self._chk(lib.rtp_forward_debug(self.h, _f(x), _f(lowres), _f(resized), _f(peaks), _f(joints), C.byref(n)))
        return dict(lowres=lowres, resized=resized, peaks=peaks, joints=joints, num_people=n.value)

    def get_blob(self, name):
        shape = (C.c_int * 4)()
        self._chk(lib.rtp_get_blob(self.h, name.encode(), None, 0, shape))
        out = np.empty(tuple(shape), np.float32)
        self._chk(lib.rtp_get_blob(self.h, name.encode(), _f(out), out.size, shape))
        return out

    def get_batch_blob(self, ctx, name):
        """rtp_get_batch_blob: (blob [nframes * N][C][H][W], tags of the frames in slot order) of the last batch that ran on batch context `ctx`."""
        shape = (C.c_int * 4)()
        tags = (C.c_uint64 * max(int(self.cfg.c.batch_frames), 1))()
        nf = C.c_int()
        self._chk(lib.rtp_get_batch_blob(self.h, int(ctx), name.encode(), None, 0, shape, tags, C.byref(nf)))
        out = np.empty(tuple(shape), np.float32)
        self._chk(lib.rtp_get_batch_blob(self.h, int(ctx), name.encode(), _f(out), out.size, shape, None, None))
        return out, list(tags)[: nf.value]

    def connect_stats(self):
        nl = 19 if self.num_parts == 18 else 14
        a = (C.c_int * nl)()
        b = (C.c_int * nl)()
        self._chk(lib.rtp_debug_connect_stats(self.h, a, b))
        return [v & ((1 << 30) - 1) for v in a], list(b), [v >> 30 for v in a]

    # ---- weights
    def conv_layers(self):
        res = []
        name = C.create_string_buffer(64)
        cin, cout, k = C.c_int(), C.c_int(), C.c_int()
        for i in range(lib.rtp_num_conv_layers(self.h)):
            lib.rtp_conv_layer_info(self.h, i, name, 64, C.byref(cin), C.byref(cout), C.byref(k))
            res.append((name.value.decode(), cin.value, cout.value, k.value))
        return res

    def get_conv_weights(self, i):
        _, cin, cout, k = self.conv_layers()[i]
        w = np.empty((cout, cin, k, k), np.float32)
        b = np.empty((cout,), np.float32)
        self._chk(lib.rtp_get_conv_weights(self.h, i, _f(w), _f(b)))
        return w, b

    def set_conv_weights(self, i, w, b):
        w = np.ascontiguousarray(w, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        self._chk(lib.rtp_set_conv_weights(self.h, i, _f(w), _f(b)))

    def save_caffemodel(self, path):
        self._chk(lib.rtp_save_caffemodel(self.h, str(path).encode()))

    def save_prototxt(self, path):
        self._chk(lib.rtp_save_prototxt(self.h, str(path).encode()))

    # ---- load-time precision calibration
    def calibrate_precision(self, frames=None, nframes=2, target=0.7e-3):
        """rtp_calibrate_precision: returns (rules, err_before, err_after); frames = [n][N][3][H][W] float32 or None (synthetic)."""
        buf = C.create_string_buffer(4096)
        a, b = C.c_float(), C.c_float()
        if frames is not None:
            frames = np.ascontiguousarray(frames, np.float32)
            nframes = frames.size // (self.N * 3 * self.net_h * self.net_w)
        self._chk(lib.rtp_calibrate_precision(self.h, _f(frames) if frames is not None else None, int(nframes), float(target), buf, len(buf), C.byref(a), C.byref(b)))
        return buf.value.decode(), a.value, b.value

    def calibration_report(self):
        return lib.rtp_calibration_report(self.h).decode()

    def split_layers(self):
        buf = C.create_string_buffer(1 << 16)   # (rtp_get_split_layers returns RTP_ERANGE instead of truncating)
        p = C.c_int()
        self._chk(lib.rtp_get_split_layers(self.h, buf, len(buf), C.byref(p)))
        return buf.value.decode(), p.value

    # ---- caller-owned device buffers (the engine's HIP runtime; bench.py keeps torch out of the data path)
    def device_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(lib.rtp_device_alloc(self.h, int(nbytes), C.byref(p)))
        return p.value

    def device_free(self, dptr):
        self._chk(lib.rtp_device_free(self.h, C.c_void_p(dptr)))

    def device_upload(self, dptr, arr):
        a = np.ascontiguousarray(arr)
        self._chk(lib.rtp_device_upload(self.h, C.c_void_p(dptr), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def device_frame(self, x):
        """A net input resident in HBM (for submit_device): allocates on the engine's device and uploads x."""
        x = np.ascontiguousarray(x, np.float32)
        p = self.device_alloc(x.nbytes)
        self.device_upload(p, x)
        return p

    def synchronize(self):
        self._chk(lib.rtp_device_synchronize(self.h))

    # ---- one-time weight distribution between replicas
    def weight_blob_bytes(self):
        """Length of this plan's weight blob without exporting one (no D2H copy of the arena)."""
        n = lib.rtp_weight_blob_bytes(self.h)
        if n < 0:
            raise RtpError(n, "rtp_weight_blob_bytes")
        return int(n)

    def weight_blob(self):
        n = lib.rtp_weight_blob_bytes(self.h)
        buf = np.empty(n, np.uint8)
        self._chk(lib.rtp_weight_blob_export(self.h, buf.ctypes.data_as(C.c_void_p), n))
        return buf

    def load_weight_blob(self, buf):
        b = np.ascontiguousarray(buf, np.uint8)
        self._chk(lib.rtp_weight_blob_import(self.h, b.ctypes.data_as(C.c_void_p), b.nbytes))

    def copy_weights_from(self, other):
        self._chk(lib.rtp_copy_weights_from(self.h, other.h))

    # ---- diagnostics
    def last_stage_ms(self):
        ms = (C.c_float * 5)()
        lib.rtp_last_stage_ms(self.h, ms)
        return dict(conv=ms[0], resize=ms[1], nms=ms[2], connect=ms[3], total=ms[4])

    def kernel_timing(self, enable=-1):
        tot, fl = C.c_double(), C.c_double()
        n = C.c_long()
        self._chk(lib.rtp_kernel_timing(self.h, enable, C.byref(tot), C.byref(n), C.byref(fl)))
        return tot.value, n.value, fl.value

    def kernel_timing_by_passes(self):
        ms = (C.c_double * 4)()
        n = (C.c_long * 4)()
        self._chk(lib.rtp_kernel_timing_by_passes(self.h, ms, n))
        return {p: (ms[p], n[p]) for p in (1, 2, 3) if n[p]}

    def kernel_timing_steps(self):
        """[(ms, launches)] per plan step of a timing pass switched on with kernel_timing(3) (harvest with kernel_timing(-1) first)."""
        cap = 512
        ms = (C.c_double * cap)()
        n = (C.c_long * cap)()
        k = lib.rtp_kernel_timing_steps(self.h, ms, n, cap)
        if k < 0:
            raise RtpError(k, "rtp_kernel_timing_steps")
        return [(ms[i], n[i]) for i in range(min(k, cap))]

    def busy_probe(self, enable=-1):
        """rtp_busy_probe: returns the spans recorded so far as an [n][3] float32 array {kind, start_ms, end_ms}."""
        n = lib.rtp_busy_probe(self.h, enable, None, 0)
        if n < 0:
            raise RtpError(n, lib.rtp_last_error(self.h).decode())
        out = np.zeros((n, 3), np.float32)
        if n:
            lib.rtp_busy_probe(self.h, -1, _f(out), n)
        return out

    def probe_dropped(self):
        """rtp_probe_dropped: {timing_pairs, busy_spans, busy_graph_frames} the probes could not record since creation."""
        out = (C.c_long * 3)()
        self._chk(lib.rtp_probe_dropped(self.h, out))
        return {"timing_pairs": out[0], "busy_spans": out[1], "busy_graph_frames": out[2]}

    def stamp_probe(self, enable=-1):
        """rtp_stamp_probe: kernel residency spans as an [n][3] float32 array {slot, start_us, end_us} (device-side wall-clock stamps)."""
        n = lib.rtp_stamp_probe(self.h, enable, None, 0)
        if n < 0:
            raise RtpError(n, lib.rtp_last_error(self.h).decode())
        out = np.zeros((n, 3), np.float32)
        if n:
            lib.rtp_stamp_probe(self.h, -1, _f(out), n)
        return out

    def stream_queues(self, reps=5):
        """rtp_debug_stream_queues: (owner [(context, frame)] per stream with (-1, 0) = the legacy stream, ratio [n][n] float32 or None when reps = 0, opens per context).
        ratio[a][b] = median pair time / single wait: ~1 = the two streams run side by side, ~2 = they share a hardware queue."""
        nctx = 64
        opens = (C.c_long * nctx)(*([-1] * nctx))
        n = lib.rtp_debug_stream_queues(self.h, 0, None, None, 0, opens, nctx)
        if n < 0:
            raise RtpError(n, lib.rtp_last_error(self.h).decode())
        owner = (C.c_int * max(n, 1))()
        ratio = np.zeros((n, n), np.float32)
        k = lib.rtp_debug_stream_queues(self.h, reps, owner, _f(ratio) if reps else None, n, None, 0)
        if k < 0:
            raise RtpError(k, lib.rtp_last_error(self.h).decode())
        return [(owner[i] // 256, owner[i] % 256) if owner[i] >= 0 else (-1, 0) for i in range(n)], (ratio if reps else None), [o for o in opens if o >= 0]

    def bench_dominant_conv(self, iters=50):
        ms = C.c_float()
        fl = C.c_double()
        self._chk(lib.rtp_bench_dominant_conv(self.h, iters, C.byref(ms), C.byref(fl)))
        return ms.value, fl.value

"""YUV frames without a GPU: the ABI surface, rtp_convert_yuv against the formula restated in numpy (all 2^24 triples, every sampling,
odd sizes, pitches, NV12 / NV21), the Y4M plane reader against rtp_video_read, the field checks with a NULL engine, the Python view
builder, and a stand-alone address/undefined-sanitizer run of rtp_convert_yuv on exactly-sized heap planes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import caffe_rtpose_amd as r
from caffe_rtpose_amd import _lib
from caffe_rtpose_amd.engine import _yuv_struct

import _yuvcases as yc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rtp_convert_yuv", "rtp_video_chroma", "rtp_video_read_yuv", "rtp_submit_frame_yuv", "rtp_submit_frame_yuv_device", "rtp_convert_yuv_device")


class _Dev:
    """Stands in for a device tensor: only __cuda_array_interface__ (nothing here is ever dereferenced)."""

    def __init__(self, shape, strides=None, typestr="|u1", ptr=1 << 20):
        self.__cuda_array_interface__ = dict(typestr=typestr, shape=shape, strides=strides, data=(ptr, False), version=2)


def test_new_symbols_are_exported():
    for name in NEW:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    assert C.sizeof(_lib.rtp_yuv_view) == 72   # 4 + 4 + 3 x 8 + 4 x 4 + 3 x 8 on LP64
    for name in ("yuv_view", "convert_yuv", "video_chroma", "video_read_yuv"):
        assert hasattr(r, name), name
    for name in ("submit_frame_yuv", "submit_frame_yuv_device", "convert_yuv_device"):
        assert hasattr(r.Engine, name), name


def test_convert_yuv_all_triples():
    y, u, v = yc.exhaustive()
    got = r.convert_yuv(y, u, v)
    want = yc.ref_bgr(y, u, v, "444")
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} of 2^24 triples differ"


@pytest.mark.parametrize("fmt", ["420", "422", "444", "mono"])
def test_convert_yuv_samplings_and_odd_sizes(fmt):
    for w, h in yc.ODD_SIZES:
        y, u, v = yc.planes(w, h, fmt)
        assert np.array_equal(r.convert_yuv(y, u, v), yc.ref_bgr(y, u, v, fmt)), (fmt, w, h)


def _padded(a, extra, fill=0xEE):
    """`a` as a window of a wider array (the pitch of a decoder surface)."""
    big = np.full((a.shape[0], a.shape[1] + extra) + a.shape[2:], fill, np.uint8)
    big[:, :a.shape[1]] = a
    return big[:, :a.shape[1]]


def test_convert_yuv_padded_pitches_and_interleaved_chroma():
    for w, h in ((5, 4), (16, 8), (67, 45)):
        y, u, v = yc.planes(w, h, "420", seed=3)
        want = yc.ref_bgr(y, u, v, "420")
        assert np.array_equal(r.convert_yuv(_padded(y, 13), _padded(u, 7), _padded(v, 7)), want), (w, h)
        assert np.array_equal(r.convert_yuv(y, yc.interleave(u, v, "uv")), want), ("nv12", w, h)
        assert np.array_equal(r.convert_yuv(y, yc.interleave(u, v, "vu"), interleaved_order="vu"), want), ("nv21", w, h)
        assert np.array_equal(r.convert_yuv(_padded(y, 3), _padded(yc.interleave(u, v), 5)), want), ("nv12 pitch", w, h)
    y, u, v = yc.planes(16, 8, "422", seed=4)
    assert np.array_equal(r.convert_yuv(_padded(y, 1), _padded(u, 3), _padded(v, 3)), yc.ref_bgr(y, u, v, "422"))


@pytest.mark.parametrize("fmt,w,h", [("420", 67, 45), ("420", 64, 48), ("422", 67, 45), ("444", 67, 45), ("mono", 67, 45)])
def test_y4m_planes_equal_the_bgr_reader(tmp_path, fmt, w, h):
    p = tmp_path / "clip.y4m"
    frames = yc.write_y4m(p, w, h, fmt, 3)
    a, b = r.Video(p), r.Video(p)
    assert r.video_chroma(a) == (400 if fmt == "mono" else int(fmt))
    for y, u, v in frames:
        got = r.video_read_yuv(a)
        assert np.array_equal(got[0], y) and (u is None and got[1] is None and got[2] is None or np.array_equal(got[1], u) and np.array_equal(got[2], v))
        bgr = b.read()
        assert np.array_equal(r.convert_yuv(*got), bgr)
        assert np.array_equal(bgr, yc.ref_bgr(y, u, v, fmt))
    assert r.video_read_yuv(a) is None and b.read() is None
    a.close()
    b.close()


def test_mjpeg_streams_have_no_planes(tmp_path):
    gold = os.path.join(ROOT, "tests", "golden", "codecs")
    jpg = open(os.path.join(gold, "j420_q75.jpg"), "rb").read()
    m = tmp_path / "clip.mjpeg"
    m.write_bytes(jpg + jpg)
    vid = r.Video(m)
    assert r.video_chroma(vid) == 0
    with pytest.raises(r.RtpError) as ex:
        r.video_read_yuv(vid)
    assert ex.value.code == r.RTP_EINVAL and "Y4M" in str(ex.value)
    assert np.array_equal(vid.read(), np.load(os.path.join(gold, "j420_q75.npy")))   # nothing was consumed
    vid.close()


def _view(w=64, h=48):
    return _yuv_struct(r.yuv_view(_Dev((h, w)), _Dev((h // 2, w // 2)), _Dev((h // 2, w // 2), ptr=1 << 21)))


@pytest.mark.parametrize("entry", ["rtp_submit_frame_yuv_device", "rtp_submit_frame_yuv", "rtp_convert_yuv_device"])
def test_refusals_without_a_gpu(entry):
    lib = _lib.lib

    def call(view):
        ref = None if view is None else C.byref(view)
        if entry == "rtp_submit_frame_yuv_device":
            return lib.rtp_submit_frame_yuv_device(None, ref, None, 0, None)
        if entry == "rtp_submit_frame_yuv":
            return lib.rtp_submit_frame_yuv(None, ref, 0, None)
        return lib.rtp_convert_yuv_device(None, ref, None, None)

    def refused(view, word):
        assert call(view) == r.RTP_EINVAL, word
        msg = lib.rtp_last_error(None)
        assert word.encode() in msg and entry.encode() in msg, (word, msg)

    refused(None, "NULL yuv view")
    for field, bad, word in (("struct_size", 64, "struct_size"), ("matrix", 1, "matrix"), ("width", 0, "view size"), ("chroma_shift_x", 2, "chroma shifts"),
                             ("chroma_shift_y", 2, "chroma shifts"), ("y_stride", -1, "y_stride"), ("uv_stride", -2, "uv_stride"),
                             ("uv_pixel_stride", 3, "uv_pixel_stride"), ("u", None, "exactly one"), ("v", None, "exactly one")):
        v = _view()
        setattr(v, field, bad)
        refused(v, word)
    v = _view()
    v.chroma_shift_x, v.chroma_shift_y = 0, 1
    refused(v, "chroma shifts")
    v = _view()
    v.height, v.y_stride = 1 << 20, (1 << 62)
    v.width = 1024
    refused(v, "overflows")
    if entry != "rtp_convert_yuv_device":   # a well-formed view with no engine: refused as such
        refused(_view(), "NULL engine")
    else:
        refused(_view(), "NULL frame view")


def test_convert_yuv_refuses_bad_views():
    v = _view()
    v.matrix = 1
    out = np.empty((48, 64, 3), np.uint8)
    assert _lib.lib.rtp_convert_yuv(C.byref(v), out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.size) == r.RTP_EINVAL
    assert b"matrix" in _lib.lib.rtp_codec_last_error()
    y, u, vv = yc.planes(16, 8, "420")
    s = _yuv_struct(r.yuv_view(y, u, vv))
    assert _lib.lib.rtp_convert_yuv(C.byref(s), out.ctypes.data_as(C.POINTER(C.c_ubyte)), 16 * 8 * 3 - 1) == r.RTP_EINVAL
    assert b"too small" in _lib.lib.rtp_codec_last_error()


def test_yuv_view_nv12_i420_and_crop():
    base = 1 << 24
    # NV12 surface of a decoder: pitch 1536 for a 1280-wide frame, chroma right behind 720 luma rows
    f = r.yuv_view(_Dev((720, 1280), strides=(1536, 1), ptr=base), _Dev((360, 640, 2), strides=(1536, 2, 1), ptr=base + 720 * 1536))
    assert f == dict(y=base, u=base + 720 * 1536, v=base + 720 * 1536 + 1, width=1280, height=720, chroma_shift_x=1, chroma_shift_y=1,
                     y_stride=1536, uv_stride=1536, uv_pixel_stride=2, device=True)
    g = r.yuv_view(_Dev((720, 1280), strides=(1536, 1), ptr=base), _Dev((360, 640, 2), strides=(1536, 2, 1), ptr=base + 720 * 1536), interleaved_order="vu")
    assert (g["u"], g["v"]) == (f["v"], f["u"])
    # I420, contiguous
    f = r.yuv_view(_Dev((45, 67), ptr=base), _Dev((23, 34), ptr=base + 4096), _Dev((23, 34), ptr=base + 8192))
    assert (f["width"], f["height"], f["chroma_shift_x"], f["chroma_shift_y"], f["y_stride"], f["uv_stride"], f["uv_pixel_stride"]) == (67, 45, 1, 1, 67, 34, 1)
    assert (f["y"], f["u"], f["v"]) == (base, base + 4096, base + 8192)
    # a crop keeps its parent's pitches: y[100:580, 200:840] of 1080p I420 and the matching chroma windows
    f = r.yuv_view(_Dev((480, 640), strides=(1920, 1), ptr=base + 100 * 1920 + 200), _Dev((240, 320), strides=(960, 1), ptr=base + (1 << 22) + 50 * 960 + 100),
                   _Dev((240, 320), strides=(960, 1), ptr=base + (1 << 23) + 50 * 960 + 100))
    assert (f["y_stride"], f["uv_stride"], f["chroma_shift_x"], f["chroma_shift_y"]) == (1920, 960, 1, 1)
    # 4:2:2, 4:4:4, luma only, host arrays
    assert (r.yuv_view(_Dev((8, 16)), _Dev((8, 8)), _Dev((8, 8)))["chroma_shift_x"], r.yuv_view(_Dev((8, 16)), _Dev((8, 8)), _Dev((8, 8)))["chroma_shift_y"]) == (1, 0)
    assert r.yuv_view(_Dev((8, 16)), _Dev((8, 16)), _Dev((8, 16)))["chroma_shift_x"] == 0
    assert r.yuv_view(_Dev((8, 16)), None)["u"] is None
    y, u, v = yc.planes(5, 3, "420")
    f = r.yuv_view(y, u, v)
    assert not f["device"] and (f["y"], f["chroma_shift_x"], f["chroma_shift_y"]) == (y.ctypes.data, 1, 1)


def test_yuv_view_refusals():
    with pytest.raises(ValueError, match="u8"):
        r.yuv_view(_Dev((48, 64), typestr="<f4"), None)
    with pytest.raises(ValueError, match="u8"):
        r.yuv_view(_Dev((48, 64)), _Dev((24, 32), typestr="<u2"), _Dev((24, 32)))
    with pytest.raises(ValueError, match="shape"):
        r.yuv_view(_Dev((48, 64, 1)), None)
    with pytest.raises(ValueError, match="shape"):
        r.yuv_view(_Dev((48, 64)), _Dev((24, 32, 2)), _Dev((24, 32, 2)))
    with pytest.raises(ValueError, match="interleaved"):
        r.yuv_view(_Dev((48, 64)), _Dev((24, 32, 3)))
    with pytest.raises(ValueError, match="sampling"):
        r.yuv_view(_Dev((48, 64)), _Dev((24, 64)), _Dev((24, 64)))       # shifts (0, 1)
    with pytest.raises(ValueError, match="sampling"):
        r.yuv_view(_Dev((48, 64)), _Dev((12, 16)), _Dev((12, 16)))       # 4:1:0
    with pytest.raises(ValueError, match="differ"):
        r.yuv_view(_Dev((48, 64)), _Dev((24, 32)), _Dev((48, 32)))
    with pytest.raises(ValueError, match="contiguous"):
        r.yuv_view(_Dev((48, 64), strides=(128, 2)), None)
    with pytest.raises(ValueError, match="order"):
        r.yuv_view(_Dev((48, 64)), _Dev((24, 32, 2)), interleaved_order="nv12")
    with pytest.raises(ValueError, match="mixed"):
        r.yuv_view(np.zeros((48, 64), np.uint8), _Dev((24, 32)), _Dev((24, 32)))
    with pytest.raises(TypeError):
        r.yuv_view([[1, 2]], None)
    with pytest.raises(TypeError, match="host"):
        r.convert_yuv(_Dev((48, 64)), None)


def test_every_triple_appears_once_in_the_420_cube():
    y, u, v = yc.exhaustive_420()
    up = np.repeat(np.repeat(u, 2, 0), 2, 1).astype(np.uint32)
    vp = np.repeat(np.repeat(v, 2, 0), 2, 1).astype(np.uint32)
    seen = np.bincount((y.astype(np.uint32) | (up << 8) | (vp << 16)).ravel(), minlength=1 << 24)
    assert seen.min() == 1 and seen.max() == 1
    assert np.array_equal(r.convert_yuv(y, u, v), yc.ref_bgr(y, u, v, "420"))


def test_host_planes_with_a_column_stride_of_two():
    """u and v as every second column of two separate arrays: uv_pixel_stride 2 without a neighbouring partner plane"""
    y, u, v = yc.planes(16, 8, "420", seed=5)
    wide_u, wide_v = np.full((4, 16), 7, np.uint8), np.full((4, 16), 9, np.uint8)
    wide_u[:, ::2], wide_v[:, ::2] = u, v
    f = r.yuv_view(y, wide_u[:, ::2], wide_v[:, ::2])
    assert f["uv_pixel_stride"] == 2 and abs(f["u"] - f["v"]) != 1
    assert np.array_equal(r.convert_yuv(y, wide_u[:, ::2], wide_v[:, ::2]), yc.ref_bgr(y, u, v, "420"))


def test_layout_choice():
    """yuv_layout through its host-side tap: 4:2:0 with w % 4 == 0, h % 2 == 0, a packed-BGR destination and every access aligned
    takes the 4 x 2 kernel; anything else the generic one."""
    base = 1 << 24
    out = _Dev((48, 64, 3), ptr=base + (1 << 20))
    y, u, v = _Dev((48, 64), ptr=base), _Dev((24, 32), ptr=base + 4096), _Dev((24, 32), ptr=base + 8192)
    uv = _Dev((24, 32, 2), ptr=base + 4096)
    assert yc.layout(y, u, v, out) == yc.LAYOUT_420_PLANAR
    assert yc.layout(y, uv, None, out) == yc.LAYOUT_420_NV12
    assert yc.layout(y, uv, None, out, interleaved_order="vu") == yc.LAYOUT_420_NV21
    assert yc.layout(_Dev((2, 4), ptr=base), _Dev((1, 2), ptr=base + 64), _Dev((1, 2), ptr=base + 66), _Dev((2, 4, 3), ptr=base + 128)) == yc.LAYOUT_420_PLANAR
    # the planes as rtp_submit_frame_yuv stages them: Y at a 256-byte boundary, U and V right behind
    assert yc.layout(_Dev((48, 64), ptr=base + 9216), _Dev((24, 32), ptr=base + 9216 + 3072), _Dev((24, 32), ptr=base + 9216 + 3840), _Dev((48, 64, 3), ptr=base)) == yc.LAYOUT_420_PLANAR
    # a window with aligned pitches
    assert yc.layout(_Dev((6, 20), strides=(32, 1), ptr=base + 8), _Dev((3, 10), strides=(16, 1), ptr=base + 4100), _Dev((3, 10), strides=(16, 1), ptr=base + 8196),
                     _Dev((6, 20, 3), strides=(96, 3, 1), ptr=base + (1 << 20) + 48)) == yc.LAYOUT_420_PLANAR
    generic = [
        (_Dev((45, 67), ptr=base), _Dev((23, 34), ptr=base + 4096), _Dev((23, 34), ptr=base + 8192), _Dev((45, 67, 3), ptr=base + (1 << 20)), {}),   # odd size
        (_Dev((48, 66), ptr=base), _Dev((24, 33), ptr=base + 4096), _Dev((24, 33), ptr=base + 8192), _Dev((48, 66, 3), ptr=base + (1 << 20)), {}),   # w % 4 == 2
        (_Dev((6, 20), strides=(27, 1), ptr=base), _Dev((3, 10), ptr=base + 4096), _Dev((3, 10), ptr=base + 8192), _Dev((6, 20, 3), ptr=base + (1 << 20)), {}),      # odd luma pitch
        (_Dev((6, 20), ptr=base + 3), _Dev((3, 10), ptr=base + 4096), _Dev((3, 10), ptr=base + 8192), _Dev((6, 20, 3), ptr=base + (1 << 20)), {}),                   # odd luma start
        (_Dev((6, 20), ptr=base), _Dev((3, 10), ptr=base + 4097), _Dev((3, 10), ptr=base + 8192), _Dev((6, 20, 3), ptr=base + (1 << 20)), {}),                       # odd u start
        (_Dev((6, 20), ptr=base), _Dev((3, 10), strides=(15, 1), ptr=base + 4096), _Dev((3, 10), strides=(15, 1), ptr=base + 8192), _Dev((6, 20, 3), ptr=base + (1 << 20)), {}),   # odd chroma pitch
        (_Dev((6, 20), ptr=base), _Dev((3, 10, 2), ptr=base + 4098), None, _Dev((6, 20, 3), ptr=base + (1 << 20)), {}),                                              # pairs not on a dword
        (_Dev((6, 20), ptr=base), _Dev((3, 10, 2), strides=(22, 2, 1), ptr=base + 4096), None, _Dev((6, 20, 3), ptr=base + (1 << 20)), {}),                          # pair pitch % 4 == 2
        (_Dev((6, 20), ptr=base), _Dev((3, 10), ptr=base + 4096), _Dev((3, 10), ptr=base + 8192), _Dev((6, 20, 3), ptr=base + (1 << 20) + 2), {}),                   # destination start
        (_Dev((6, 20), ptr=base), _Dev((3, 10), ptr=base + 4096), _Dev((3, 10), ptr=base + 8192), _Dev((6, 20, 3), strides=(62, 3, 1), ptr=base + (1 << 20)), {}),  # destination pitch
        (_Dev((6, 20), ptr=base), _Dev((3, 10), ptr=base + 4096), _Dev((3, 10), ptr=base + 8192), _Dev((6, 20, 3), ptr=base + (1 << 20)), dict(order="rgb")),
        (_Dev((6, 20), ptr=base), _Dev((3, 10), ptr=base + 4096), _Dev((3, 10), ptr=base + 8192), _Dev((6, 20, 3), strides=(80, 4, 1), ptr=base + (1 << 20)), {}),  # BGRA
        (_Dev((6, 20), ptr=base), _Dev((6, 10), ptr=base + 4096), _Dev((6, 10), ptr=base + 8192), _Dev((6, 20, 3), ptr=base + (1 << 20)), {}),                       # 4:2:2
        (_Dev((6, 20), ptr=base), _Dev((6, 20), ptr=base + 4096), _Dev((6, 20), ptr=base + 8192), _Dev((6, 20, 3), ptr=base + (1 << 20)), {}),                       # 4:4:4
        (_Dev((6, 20), ptr=base), None, None, _Dev((6, 20, 3), ptr=base + (1 << 20)), {}),                                                                            # luma only
        (_Dev((6, 20), ptr=base), _Dev((3, 10), strides=(32, 2), ptr=base + 4096), _Dev((3, 10), strides=(32, 2), ptr=base + 8192), _Dev((6, 20, 3), ptr=base + (1 << 20)), {}),   # stride 2, no partner
    ]
    for i, (a, b, c, o, kw) in enumerate(generic):
        assert yc.layout(a, b, c, o, **kw) == yc.LAYOUT_GENERIC, i


def test_package_import_does_not_import_torch():
    import sys
    code = "import sys; import caffe_rtpose_amd as r; r.yuv_view; assert 'torch' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_convert_yuv_is_clean_under_sanitizers(tmp_path):
    """tests/helpers/yuv_check.cpp (its own main) calls rtp_convert_yuv on exactly-sized heap planes of the odd shapes: a byte read or
    written outside a plane is an AddressSanitizer report.  Built with the host-only sources; nothing is loaded into python."""
    csrc = os.path.join(ROOT, "caffe_rtpose_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "helpers", "yuv_check.cpp")] + [os.path.join(csrc, f) for f in ("codecs.cpp", "preprocess.cpp", "host_util.cpp")]
    exe = str(tmp_path / "yuv_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-o", exe] + src + ["-lpthread", "-lz"],
                       capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and ("cannot find" in p.stderr or "unrecognized" in p.stderr):
        pytest.skip(f"this toolchain has no address / undefined sanitizer: {p.stderr[-200:]}")
    assert p.returncode == 0, p.stderr[-3000:]
    q = subprocess.run([exe], capture_output=True, text=True, timeout=300, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert q.returncode == 0, q.stdout[-2000:] + q.stderr[-3000:]
    assert not [ln for ln in q.stderr.splitlines() if "Sanitizer" in ln or "runtime error:" in ln], q.stderr[-3000:]
    assert "yuv_check OK" in q.stdout

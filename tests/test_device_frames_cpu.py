"""Frames in GPU memory (rtp_submit_frame_device / rtp_collect_rendered_device): the ABI surface and the Python view builder, without a GPU."""
import ctypes as C

import pytest

import caffe_rtpose_amd as r
from caffe_rtpose_amd import _lib
from caffe_rtpose_amd.engine import _view_struct


class _Dev:
    """Stands in for a device tensor: only __cuda_array_interface__ (nothing here is ever dereferenced)."""

    def __init__(self, shape, strides=None, typestr="|u1", ptr=1 << 20):
        self.__cuda_array_interface__ = dict(typestr=typestr, shape=shape, strides=strides, data=(ptr, False), version=2)


def test_new_symbols_are_exported():
    for name in ("rtp_submit_frame_device", "rtp_collect_rendered_device"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert C.sizeof(_lib.rtp_frame_view) == 64   # unsigned + pad, pointer, 2 ints, 5 longs


def test_refusals_without_a_gpu():
    lib = _lib.lib
    assert lib.rtp_submit_frame_device(None, None, None, 0, None) == r.RTP_EINVAL
    assert b"NULL frame view" in lib.rtp_last_error(None)
    assert lib.rtp_collect_rendered_device(None, None, None, None, None, None) == r.RTP_EINVAL
    v = _view_struct(r.frame_view(_Dev((48, 64, 3))))
    v.struct_size = C.sizeof(_lib.rtp_frame_view) - 8
    assert lib.rtp_submit_frame_device(None, C.byref(v), None, 0, None) == r.RTP_EINVAL
    assert b"struct_size" in lib.rtp_last_error(None)
    assert lib.rtp_collect_rendered_device(None, None, None, None, C.byref(v), None) == r.RTP_EINVAL
    assert b"struct_size" in lib.rtp_last_error(None)
    v.struct_size = C.sizeof(_lib.rtp_frame_view)
    for field, bad in (("width", 0), ("height", -1), ("row_stride", -3), ("pixel_stride", 0)):
        w = _view_struct(r.frame_view(_Dev((48, 64, 3))))
        setattr(w, field, bad)
        assert lib.rtp_submit_frame_device(None, C.byref(w), None, 0, None) == r.RTP_EINVAL, field
    w = _view_struct(r.frame_view(_Dev((48, 64, 3))))
    w.channel_offset[1] = -1
    assert lib.rtp_submit_frame_device(None, C.byref(w), None, 0, None) == r.RTP_EINVAL
    assert b"channel_offset" in lib.rtp_last_error(None)
    # a well-formed view with no engine: refused as such
    assert lib.rtp_submit_frame_device(None, C.byref(v), None, 0, None) == r.RTP_EINVAL
    assert b"NULL engine" in lib.rtp_last_error(None)


@pytest.mark.parametrize("C_,order,offs", [(3, "bgr", (0, 1, 2)), (3, "rgb", (2, 1, 0)), (4, "bgr", (0, 1, 2)), (4, "rgb", (2, 1, 0))])
def test_frame_view_hwc(C_, order, offs):
    f = r.frame_view(_Dev((720, 1280, C_), ptr=4096), order)
    assert f == dict(data=4096, width=1280, height=720, row_stride=1280 * C_, pixel_stride=C_, channel_offset=offs)
    assert r.frame_view(_Dev((720, 1280, C_), strides=(1280 * C_, C_, 1), ptr=4096), order) == f


def test_frame_view_crop_keeps_the_row_pitch():
    # x[100:580, 200:840] of a (1080, 1920, 3) tensor: the crop starts at its first pixel, rows keep the parent's pitch
    base = 1 << 24
    ptr = base + 100 * 1920 * 3 + 200 * 3
    f = r.frame_view(_Dev((480, 640, 3), strides=(1920 * 3, 3, 1), ptr=ptr))
    assert f == dict(data=ptr, width=640, height=480, row_stride=5760, pixel_stride=3, channel_offset=(0, 1, 2))
    # channels [..., :3] of an RGBA image
    f = r.frame_view(_Dev((480, 640, 3), strides=(2560, 4, 1), ptr=base), "rgb")
    assert (f["row_stride"], f["pixel_stride"], f["channel_offset"]) == (2560, 4, (2, 1, 0))


def test_frame_view_planar_chw():
    plane = 720 * 1280
    f = r.frame_view(_Dev((3, 720, 1280), ptr=8192), "rgb")
    assert f == dict(data=8192, width=1280, height=720, row_stride=1280, pixel_stride=1, channel_offset=(2 * plane, plane, 0))
    f = r.frame_view(_Dev((3, 480, 640), strides=(plane, 1280, 1), ptr=8192), "bgr")
    assert (f["width"], f["height"], f["row_stride"], f["pixel_stride"], f["channel_offset"]) == (640, 480, 1280, 1, (0, plane, 2 * plane))


def test_frame_view_refusals():
    with pytest.raises(ValueError, match="u8"):
        r.frame_view(_Dev((48, 64, 3), typestr="<f4"))
    with pytest.raises(ValueError, match="u8"):
        r.frame_view(_Dev((48, 64, 3), typestr="<u2"))
    for shape in ((48, 64), (1, 48, 64, 3), (48 * 64 * 3,)):
        with pytest.raises(ValueError, match="shape"):
            r.frame_view(_Dev(shape))
    for shape in ((48, 64, 2), (48, 64, 1), (4, 48, 64), (48, 64, 5)):
        with pytest.raises(ValueError, match="channels"):
            r.frame_view(_Dev(shape))
    with pytest.raises(ValueError, match="order"):
        r.frame_view(_Dev((48, 64, 3)), "bgra")
    with pytest.raises(TypeError, match="__cuda_array_interface__"):
        import numpy as np
        r.frame_view(np.zeros((48, 64, 3), np.uint8))


def test_package_import_does_not_import_torch():
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; import caffe_rtpose_amd; assert 'torch' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", code], cwd=root)

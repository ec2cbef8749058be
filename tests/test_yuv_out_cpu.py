"""YUV output, host side (no GPU): rtp_convert_bgr_to_yuv against its formulas restated in numpy (_yuvoutcases.ref_planes) for every
view kind and the odd sizes, with guard bytes around every plane; the whole BGR cube (ranges without a clamp, and the round trip through
rtp_convert_yuv); every refusal of the host function and, with a NULL engine, of the device entries; the Y4M / MJPEG stream writers
read back through the project's own reader; the stand-alone sanitizer program; rtpose.bin --write_video under --dry_engine.
Everything is integer arithmetic: no tolerances except the round trip's, which the arithmetic itself fixes (see the test)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _yuvoutcases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
SIZES = [(1, 1), (3, 5), (17, 9), (64, 48)]   # (w, h)
# (fmt, layout, pitch padding, first column, padding of the source rows in bytes)
VIEWS = {"420_planar": ("420", "planar", 0, 0, 0), "nv12": ("420", "nv12", 0, 0, 0), "nv21": ("420", "nv21", 0, 0, 0),
         "422": ("422", "planar", 0, 0, 0), "444": ("444", "planar", 0, 0, 0), "luma_only": ("mono", "mono", 0, 0, 0),
         "pitched_planes": ("420", "planar", 5, 3, 0), "pitched_nv12": ("420", "nv12", 3, 1, 0), "pitched_422": ("422", "planar", 7, 2, 0),
         "source_row_stride": ("420", "planar", 0, 0, 7)}


def _source(w, h, pad, seed):
    """the test image as rows `pad` bytes longer than 3 w (guard bytes in the padding)"""
    img = oc.image(w, h, seed)
    if not pad:
        return img, img
    big = np.full((h, 3 * w + pad), oc.GUARD, np.uint8)
    win = np.lib.stride_tricks.as_strided(big, (h, w, 3), (3 * w + pad, 3, 1))
    win[...] = img
    return win, img


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_host_definition_equals_the_numpy_restatement(size, view):
    import caffe_rtpose_amd as r
    w, h = size
    fmt, layout, extra, dx, spad = VIEWS[view]
    src, img = _source(w, h, spad, seed=3)
    dst = oc.HostPlanes(w, h, fmt, layout, extra, dx)
    r.convert_bgr_to_yuv(src, out=dst.out, interleaved_order=dst.order)
    for name, got, want in zip("yuv", dst.planes(), oc.ref_planes(img, fmt)):
        assert (got is None) == (want is None)
        if want is not None:
            assert np.array_equal(got, want), f"{view} {w}x{h}: plane {name} differs in {int((got != want).sum())} samples"
    assert dst.guards_intact(), f"{view} {w}x{h}: a byte outside the planes (guard rows or pitch padding) was written"
    assert np.array_equal(src, img)


def test_new_planes_by_chroma_name():
    import caffe_rtpose_amd as r
    img = oc.image(17, 9, seed=5)
    for chroma, fmt in ((420, "420"), (422, "422"), (444, "444"), (400, "mono")):
        got = r.convert_bgr_to_yuv(img, chroma)
        for a, b in zip(got, oc.ref_planes(img, fmt)):
            assert (a is None and b is None) or np.array_equal(a, b), chroma
    with pytest.raises(ValueError):
        r.convert_bgr_to_yuv(img, 411)


def test_whole_cube_at_444():
    """All 2^24 triples: the ranges hold without a clamp, and rtp_convert_yuv of the planes returns every channel within 3 (the two
    8-bit roundings and the limited range's 219 / 224 steps; measured exhaustively: R 2, G 2, B 3)."""
    import caffe_rtpose_amd as r
    img = oc.cube()
    y, u, v = oc.cube_planes("444")
    assert (int(y.min()), int(y.max())) == (16, 235)
    assert int(u.min()) >= 16 and int(u.max()) <= 240 and int(v.min()) >= 16 and int(v.max()) <= 240
    assert (int(u.min()), int(u.max()), int(v.min()), int(v.max())) == (16, 240, 16, 240)
    back = r.convert_yuv(y, u, v)
    err = np.abs(back.astype(np.int16) - img.astype(np.int16)).reshape(-1, 3).max(0)
    print("round trip, max |error| of B, G, R:", err.tolist())
    assert (err <= 3).all(), err.tolist()
    # rows of the cube against the restatement (the whole cube in numpy would take a minute)
    for row in (0, 1, 255, 256, 2048, 4095):
        for a, b in zip((y, u, v), oc.ref_planes(img[row:row + 1], "444")):
            assert np.array_equal(a[row:row + 1], b), row


def _view(w=4, h=4, **kw):
    from caffe_rtpose_amd import _lib
    buf = np.zeros(64, np.uint8)
    v = _lib.rtp_yuv_view()
    v.struct_size = C.sizeof(_lib.rtp_yuv_view)
    v.matrix = 0
    v.y, v.u, v.v = buf.ctypes.data, buf.ctypes.data + 16, buf.ctypes.data + 20
    v.width, v.height = w, h
    v.chroma_shift_x = v.chroma_shift_y = 1
    v.y_stride, v.uv_stride, v.uv_pixel_stride = w, (w + 1) // 2, 1
    for k, val in kw.items():
        setattr(v, k, val)
    v._keep = buf
    return v


BAD_FIELDS = {
    "struct_size": dict(struct_size=8), "matrix": dict(matrix=1), "width": dict(width=0), "height": dict(height=-1),
    "pixels": dict(width=1 << 16, height=1 << 15), "shift_x": dict(chroma_shift_x=2), "shift_y": dict(chroma_shift_y=-1),
    "shifts_0_1": dict(chroma_shift_x=0, chroma_shift_y=1), "y_stride": dict(y_stride=-1), "uv_stride": dict(uv_stride=-4),
    "uv_pixel_stride": dict(uv_pixel_stride=3), "y_null": dict(y=None), "u_null": dict(u=None), "v_null": dict(v=None),
}


def _frame_struct(w=4, h=4):
    from caffe_rtpose_amd import _lib
    f = _lib.rtp_frame_view()
    f.struct_size = C.sizeof(_lib.rtp_frame_view)
    f.data, f.width, f.height, f.row_stride, f.pixel_stride = 0x1000, w, h, 3 * w, 3
    f.channel_offset[0], f.channel_offset[1], f.channel_offset[2] = 0, 1, 2
    return f


@pytest.mark.parametrize("field", sorted(BAD_FIELDS))
def test_view_field_refusals(field):
    """Every field check of the view, with the validator and the message of rtp_convert_yuv, for the host function and — NULL engine,
    so nothing touches a GPU — the device entries that take a view."""
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd._lib import lib
    bad = _view(**BAD_FIELDS[field])
    out = np.zeros(48, np.uint8)
    assert lib.rtp_convert_yuv(C.byref(bad), out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.size) == r.RTP_EINVAL
    want = lib.rtp_codec_last_error().decode().split(": ", 1)[1]
    img = np.zeros((4, 4, 3), np.uint8)
    assert lib.rtp_convert_bgr_to_yuv(img.ctypes.data_as(C.POINTER(C.c_ubyte)), 4, 4, 12, C.byref(bad)) == r.RTP_EINVAL
    assert lib.rtp_codec_last_error().decode() == "rtp_convert_bgr_to_yuv: " + want
    fv = _frame_struct()
    assert lib.rtp_convert_to_yuv_device(None, C.byref(fv), C.byref(bad), None) == r.RTP_EINVAL
    assert lib.rtp_last_error(None).decode() == "rtp_convert_to_yuv_device: " + want
    assert lib.rtp_collect_rendered_yuv_device(None, None, None, None, C.byref(bad), None) == r.RTP_EINVAL
    assert lib.rtp_last_error(None).decode() == "rtp_collect_rendered_yuv_device: " + want


def test_null_and_size_refusals():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd._lib import lib
    ok = _view()
    img = np.zeros((4, 4, 3), np.uint8)
    p = img.ctypes.data_as(C.POINTER(C.c_ubyte))
    assert lib.rtp_convert_bgr_to_yuv(p, 4, 4, 12, C.byref(ok)) == r.RTP_OK
    assert lib.rtp_convert_bgr_to_yuv(None, 4, 4, 12, C.byref(ok)) == r.RTP_EINVAL
    assert lib.rtp_convert_bgr_to_yuv(p, 4, 4, 12, None) == r.RTP_EINVAL and "NULL yuv view" in lib.rtp_codec_last_error().decode()
    assert lib.rtp_convert_bgr_to_yuv(p, 2, 4, 12, C.byref(ok)) == r.RTP_EINVAL and "2 x 4" in lib.rtp_codec_last_error().decode()
    assert lib.rtp_convert_bgr_to_yuv(p, 4, 4, 11, C.byref(ok)) == r.RTP_EINVAL and "row_stride" in lib.rtp_codec_last_error().decode()
    fv = _frame_struct()
    # NULL engine behind valid views; NULL views; a frame of another size
    assert lib.rtp_convert_to_yuv_device(None, C.byref(fv), C.byref(ok), None) == r.RTP_EINVAL and "NULL engine" in lib.rtp_last_error(None).decode()
    assert lib.rtp_convert_to_yuv_device(None, C.byref(fv), None, None) == r.RTP_EINVAL and "NULL yuv view" in lib.rtp_last_error(None).decode()
    assert lib.rtp_convert_to_yuv_device(None, None, C.byref(ok), None) == r.RTP_EINVAL
    fv2 = _frame_struct(8, 4)
    assert lib.rtp_convert_to_yuv_device(None, C.byref(fv2), C.byref(ok), None) == r.RTP_EINVAL and "8 x 4" in lib.rtp_last_error(None).decode()
    assert lib.rtp_collect_rendered_yuv_device(None, None, None, None, C.byref(ok), None) == r.RTP_EINVAL and "NULL engine" in lib.rtp_last_error(None).decode()
    assert lib.rtp_collect_rendered_yuv_device(None, None, None, None, None, None) == r.RTP_EINVAL
    buf = np.zeros(64, np.uint8)
    assert lib.rtp_collect_rendered_yuv(None, None, None, None, buf.ctypes.data_as(C.POINTER(C.c_ubyte)), buf.size) == r.RTP_EINVAL
    assert "NULL engine" in lib.rtp_last_error(None).decode()
    assert lib.rtp_set_render_yuv(None, 420) == r.RTP_EINVAL


def test_yuv_bytes():
    import caffe_rtpose_amd as r
    assert r.yuv_bytes(1280, 720) == 1280 * 720 * 3 // 2
    assert r.yuv_bytes(1, 1, 420) == 3 and r.yuv_bytes(3, 5, 420) == 15 + 2 * 2 * 3 and r.yuv_bytes(17, 9, 420) == 153 + 2 * 9 * 5
    assert r.yuv_bytes(17, 9, 422) == 153 + 2 * 9 * 9 and r.yuv_bytes(17, 9, 444) == 3 * 153 and r.yuv_bytes(17, 9, 400) == 153
    for w, h, c in ((0, 4, 420), (4, 0, 420), (-1, 4, 420), (4, 4, 0), (4, 4, 411), (4, 4, 421)):
        assert r.yuv_bytes(w, h, c) == 0, (w, h, c)
    assert r.yuv_bytes(65536, 65536, 444) == 3 * (1 << 32)   # size_t, not int


def test_y4m_writer_round_trip(tmp_path):
    """3 frames of 18 x 10 (odd chroma width), from planar, pitched and NV12 planes: the project's reader returns the size, the count and
    the plane bytes; the header's chroma tag is one the reader takes as 4:2:0."""
    import caffe_rtpose_amd as r
    w, h, path = 18, 10, tmp_path / "clip.y4m"
    frames = []
    wr = r.VideoWriter(path, w, h, fps=(30000, 1001))
    for i, (layout, extra) in enumerate((("planar", 0), ("planar", 6), ("nv12", 3))):
        dst = oc.HostPlanes(w, h, "420", layout, extra, dx=1 if extra else 0)
        r.convert_bgr_to_yuv(oc.image(w, h, seed=20 + i), out=dst.out, interleaved_order=dst.order)
        wr.write_yuv(*dst.out, interleaved_order=dst.order)
        frames.append(dst.planes())
    wr.close()
    data = open(path, "rb").read()
    assert data.startswith(b"YUV4MPEG2 W18 H10 F30000:1001 ") and b" C420jpeg" in data[:data.index(b"\n")]
    assert len(data) == data.index(b"\n") + 1 + 3 * (6 + r.yuv_bytes(w, h))
    vid = r.Video(path)
    assert (vid.w, vid.h_, vid.nframes, vid.chroma()) == (w, h, 3, 420)
    for i, want in enumerate(frames):
        got = vid.read_yuv()
        assert got is not None and all(np.array_equal(a, b) for a, b in zip(got, want)), i
    assert vid.read_yuv() is None
    vid.close()
    assert [f[0].tobytes() for f in oc.parse_y4m(data)[3]] == [f[0].tobytes() for f in frames]


def test_mjpeg_writer_round_trip(tmp_path):
    import caffe_rtpose_amd as r
    w, h, path = 18, 10, tmp_path / "clip.mjpg"
    files = [r.encode_jpeg(oc.image(w, h, seed=30 + i), 90) for i in range(3)]
    with r.VideoWriter(path, w, h) as wr:
        assert wr.kind == r.VIDEO_MJPEG
        for f in files:
            wr.write_jpeg(f)
    assert open(path, "rb").read() == b"".join(files)
    vid = r.Video(path)
    assert (vid.w, vid.h_, vid.nframes, vid.chroma()) == (w, h, 3, 0)
    assert [vid.read_jpeg() for _ in range(3)] == files and vid.read_jpeg() is None
    vid.close()


def test_writer_refusals(tmp_path):
    import caffe_rtpose_amd as r
    w, h = 18, 10
    y, u, v = r.convert_bgr_to_yuv(oc.image(w, h, seed=1))
    jpg = r.encode_jpeg(oc.image(w, h, seed=1), 90)
    y4m, mj = r.VideoWriter(tmp_path / "a.y4m", w, h), r.VideoWriter(tmp_path / "a.mjpeg", w, h)

    def refused(call, word):
        with pytest.raises(r.RtpError) as ex:
            call()
        assert ex.value.code == r.RTP_EINVAL and word in str(ex.value), ex.value

    refused(lambda: y4m.write_jpeg(jpg), "rtp_video_write_yuv")           # wrong kind, both ways: the message names the right entry
    refused(lambda: mj.write_yuv(y, u, v), "rtp_video_write_jpeg")
    refused(lambda: y4m.write_yuv(*r.convert_bgr_to_yuv(oc.image(16, 10, seed=1))), "18 x 10")   # wrong size
    refused(lambda: y4m.write_yuv(*r.convert_bgr_to_yuv(oc.image(w, h, seed=1), 444)), "4:2:0")  # wrong chroma
    refused(lambda: y4m.write_yuv(y, None), "4:2:0")
    refused(lambda: mj.write_jpeg(b"not a jpeg file"), "SOI")
    y4m.write_yuv(y, u, v)
    mj.write_jpeg(jpg)
    y4m.close()
    mj.close()
    assert r.Video(tmp_path / "a.y4m").nframes == 1 and open(tmp_path / "a.mjpeg", "rb").read() == jpg   # the refused writes left nothing
    for bad in (dict(w=0), dict(h=0), dict(fps=0), dict(kind=3)):
        kw = dict(dict(w=w, h=h, fps=30, kind=r.VIDEO_Y4M), **bad)
        refused(lambda: r.VideoWriter(tmp_path / "b.y4m", kw["w"], kw["h"], kw["kind"], kw["fps"]), "rtp_video_create")
    with pytest.raises(ValueError):
        r.VideoWriter(tmp_path / "b.avi", w, h)
    with pytest.raises(r.RtpError) as ex:
        r.VideoWriter(tmp_path / "missing" / "b.y4m", w, h)
    assert ex.value.code == r.RTP_EIO


def test_writer_never_seeks(tmp_path):
    """The path may be a FIFO feeding an encoder: the stream arrives whole through a pipe.  The reading end is a child process that is
    ended on every way out of the test, so that nothing stays blocked on the FIFO when the writer cannot be made."""
    import sys
    import caffe_rtpose_amd as r
    w, h, fifo = 18, 10, str(tmp_path / "pipe.y4m")
    os.mkfifo(fifo)
    reader = subprocess.Popen([sys.executable, "-c", "import sys; sys.stdout.buffer.write(open(sys.argv[1], 'rb').read())", fifo], stdout=subprocess.PIPE)
    try:
        imgs = [oc.image(w, h, seed=40 + i) for i in range(2)]
        with r.VideoWriter(fifo, w, h) as wr:
            for img in imgs:
                wr.write_bgr(img)
        data = reader.communicate(timeout=60)[0]
    finally:
        if reader.poll() is None:
            reader.kill()
            reader.wait()
    assert reader.returncode == 0 and len(data) > 0
    frames = oc.parse_y4m(data)[3]
    assert len(frames) == 2
    for f, img in zip(frames, imgs):
        assert all(np.array_equal(a, b) for a, b in zip(f, oc.ref_planes(img, "420")))


def test_convert_and_writers_are_clean_under_sanitizers(tmp_path):
    """tests/helpers/yuv_out_check.cpp (its own main) calls rtp_convert_bgr_to_yuv on exactly-sized heap images and planes of the odd
    shapes, and both writers: a byte read or written outside a block is an AddressSanitizer report.  Built with the host-only sources;
    nothing is loaded into python."""
    csrc = os.path.join(ROOT, "caffe_rtpose_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "helpers", "yuv_out_check.cpp")] + [os.path.join(csrc, f) for f in ("codecs.cpp", "preprocess.cpp", "host_util.cpp")]
    exe = str(tmp_path / "yuv_out_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-o", exe] + src + ["-lpthread", "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    out = tmp_path / "streams"
    out.mkdir()
    q = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=300, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert q.returncode == 0, q.stdout[-2000:] + q.stderr[-3000:]
    assert not [ln for ln in q.stderr.splitlines() if "Sanitizer" in ln or "runtime error:" in ln], q.stderr[-3000:]
    assert "yuv_out_check OK" in q.stdout


DRY = ["--video", "synthetic:64x48:6", "--dry_engine", "400", "--model", "coco", "--resolution", "64x48", "--net_resolution", "64x48", "--no_display", "--no_frame_drops"]


def _dry_frame(i, w=64, h=48):
    """what a --dry_engine worker hands the writers in place of the i-th frame's rendered image (Frame::index counts from 1)"""
    return np.full((h, w, 3), 40 + ((i + 1) * 7) % 160, np.uint8)


def test_cli_dry_writes_y4m(tmp_path):
    import caffe_rtpose_amd as r
    out = tmp_path / "out.y4m"
    p = subprocess.run([BIN] + DRY + ["--write_video", str(out), "--video_fps", "25"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    w, h, tags, frames = oc.parse_y4m(open(out, "rb").read())
    assert (w, h) == (64, 48) and b"F25:1" in tags and len(frames) == 6
    for i, f in enumerate(frames):
        want = r.convert_bgr_to_yuv(_dry_frame(i))
        assert all(np.array_equal(a, b) for a, b in zip(f, want)), i
    vid = r.Video(out)
    assert (vid.w, vid.h_, vid.nframes) == (64, 48, 6)
    vid.close()
    # --host_video is what --dry_engine does anyway: the same bytes
    p = subprocess.run([BIN] + DRY + ["--write_video", str(tmp_path / "host.y4m"), "--video_fps", "25", "--host_video"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert open(tmp_path / "host.y4m", "rb").read() == open(out, "rb").read()


def test_cli_dry_writes_mjpeg_next_to_the_frames(tmp_path):
    import caffe_rtpose_amd as r
    out, frames = tmp_path / "out.mjpeg", tmp_path / "frames"
    p = subprocess.run([BIN] + DRY + ["--write_video", str(out), "--write_frames", str(frames)], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    files = [open(frames / f, "rb").read() for f in sorted(os.listdir(frames))]
    assert len(files) == 6 and open(out, "rb").read() == b"".join(files)
    assert files == [r.encode_jpeg(_dry_frame(i), 98) for i in range(6)]


def test_cli_refusals(tmp_path):
    p = subprocess.run([BIN] + DRY + ["--write_video", str(tmp_path / "out.y4m"), "--write_frames", str(tmp_path / "frames")], capture_output=True, timeout=300)
    assert p.returncode != 0 and b"--write_frames" in p.stderr and b"one renderer mode" in p.stderr
    assert not os.path.exists(tmp_path / "out.y4m")
    p = subprocess.run([BIN] + DRY + ["--write_video", str(tmp_path / "out.avi")], capture_output=True, timeout=300)
    assert p.returncode != 0 and b".y4m" in p.stderr
    p = subprocess.run([BIN] + DRY + ["--write_video", str(tmp_path / "missing" / "out.y4m")], capture_output=True, timeout=300)
    assert p.returncode != 0 and b"cannot create" in p.stderr
    help_ = subprocess.run([BIN, "--help"], capture_output=True, timeout=60)
    assert b"--write_video" in help_.stdout and b"--host_video" in help_.stdout and b"--video_fps" in help_.stdout
    assert b"frames that were processed" in help_.stdout   # what frame drops mean for the stream

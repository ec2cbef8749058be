"""YUV frames on the GPU.  rtp_convert_yuv_device against rtp_convert_yuv byte for byte (all 2^24 triples; the 4 x 2 kernel and the
generic one at every size and layout at which the choice or the addressing changes; planes that end with their allocations), and
rtp_submit_frame_yuv / rtp_submit_frame_yuv_device against rtp_submit_frame of rtp_convert_yuv's pixels: frame_scale, num_people,
joints, rendered frames and GPU-JPEG files bit for bit.  Everything is integer arithmetic: no tolerances."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _yuvcases as yc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
NET_W, NET_H = 320, 176
DISP_W, DISP_H = 1280, 720


def _torch():
    import torch   # (tests/conftest.py imported it before the engine library: one HIP runtime for both)
    return torch


def _engine(**kw):
    import caffe_rtpose_amd as r
    kw = dict(dict(net_w=NET_W, net_h=NET_H, disp_w=DISP_W, disp_h=DISP_H, frames_in_flight=2), **kw)
    e = r.Engine(r.Config(**kw))
    t = r.default_thresholds(e.cfg.c.model)
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], 2, 0.05)   # keep more "people" of the noise maps
    return e


@pytest.fixture(scope="module")
def engine():
    e = _engine(render=1)
    yield e
    e.close()


def _dev(a):
    return None if a is None else _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _window(a, extra, dx=0, fill=0xEE):
    """`a` on the device as a window of a wider tensor: pitch = width + extra, first column dx."""
    torch = _torch()
    big = torch.full((a.shape[0], a.shape[1] + extra) + tuple(a.shape[2:]), fill, dtype=torch.uint8, device="cuda")
    win = big[:, dx:dx + a.shape[1]]
    win.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return win


def _convert(e, y, u, v, out=None, order="bgr", **kw):
    """convert_yuv_device of device planes into a fresh (or the given) device tensor -> host array"""
    torch = _torch()
    if out is None:
        out = torch.full((y.shape[0], y.shape[1], 3), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e.convert_yuv_device(y, u, v, out, order=order, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


BLOCK = {"planar": yc.LAYOUT_420_PLANAR, "nv12": yc.LAYOUT_420_NV12, "nv21": yc.LAYOUT_420_NV21}


def _convert_checked(e, kernel, y, u, v, **kw):
    """_convert into a fresh BGR tensor, after asserting that the library picks `kernel` for exactly these tensors"""
    torch = _torch()
    out = torch.full((y.shape[0], y.shape[1], 3), 0x5A, dtype=torch.uint8, device="cuda")
    assert yc.layout(y, u, v, out, **kw) == kernel, f"kernel choice for {tuple(y.shape)}: wanted layout {kernel}"
    return _convert(e, y, u, v, out=out, **kw)


def _check(e, w, h, fmt, layout="planar", what="", block=False):
    """block: the frame must take the 4 x 2 kernel of its layout; otherwise it must take the generic kernel"""
    import caffe_rtpose_amd as r
    y, u, v = yc.planes(w, h, fmt, seed=11)
    want = r.convert_yuv(y, u, v)
    kernel = BLOCK[layout] if block else yc.LAYOUT_GENERIC
    if layout == "planar":
        got = _convert_checked(e, kernel, _dev(y), _dev(u), _dev(v))
    else:
        order = "uv" if layout == "nv12" else "vu"
        got = _convert_checked(e, kernel, _dev(y), _dev(yc.interleave(u, v, order)), None, interleaved_order=order)
    assert np.array_equal(got, want), f"{what} {fmt} {layout} {w}x{h}: {int((got != want).any(-1).sum())} pixels differ"


def test_convert_all_triples(engine):
    import caffe_rtpose_amd as r
    y, u, v = yc.exhaustive()
    want = r.convert_yuv(y, u, v)
    got = _convert_checked(engine, yc.LAYOUT_GENERIC, _dev(y), _dev(u), _dev(v))
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} of 2^24 triples differ"


def test_convert_420_block_kernel(engine):
    """w % 4 == 0, h % 2 == 0, aligned planes (torch allocations are 256-byte aligned, the pitches multiples of 4): the 4 x 2 kernel"""
    for w, h in ((4, 2), (16, 8), (64, 48)):
        for layout in ("planar", "nv12", "nv21"):
            _check(engine, w, h, "420", layout, "block kernel", block=True)


def test_block_kernel_all_triples(engine):
    """Every (Y, U, V) triple through the 4 x 2 kernel's own packing (a 4096 x 4096 4:2:0 image), planar and interleaved"""
    import caffe_rtpose_amd as r
    y, u, v = yc.exhaustive_420()
    want = r.convert_yuv(y, u, v)
    dy = _dev(y)
    got = _convert_checked(engine, yc.LAYOUT_420_PLANAR, dy, _dev(u), _dev(v))
    assert np.array_equal(got, want), f"planar: {int((got != want).any(-1).sum())} of 2^24 triples differ"
    got = _convert_checked(engine, yc.LAYOUT_420_NV12, dy, _dev(yc.interleave(u, v)), None)
    assert np.array_equal(got, want), f"nv12: {int((got != want).any(-1).sum())} of 2^24 triples differ"
    got = _convert_checked(engine, yc.LAYOUT_420_NV21, dy, _dev(yc.interleave(u, v, "vu")), None, interleaved_order="vu")
    assert np.array_equal(got, want), f"nv21: {int((got != want).any(-1).sum())} of 2^24 triples differ"


def test_convert_generic_kernel(engine):
    import caffe_rtpose_amd as r
    e = engine
    _check(e, 5, 4, "420", "nv21", "odd width")
    for w, h in ((1, 1), (3, 3), (5, 4), (67, 45)):
        for layout in ("planar", "nv12"):
            _check(e, w, h, "420", layout, "odd size")
    for fmt in ("422", "444", "mono"):
        for w, h in ((1, 1), (5, 4), (16, 8), (67, 45)):
            _check(e, w, h, fmt, "planar")
    # w % 4 == 0 and h % 2 == 0, but an odd pitch and an odd start: the alignment test of the layout choice must fail
    for w, h in ((67, 45), (20, 6)):
        y, u, v = yc.planes(w, h, "420", seed=13)
        want = r.convert_yuv(y, u, v)
        got = _convert_checked(e, yc.LAYOUT_GENERIC, _window(y, 7, dx=3), _window(u, 5, dx=1), _window(v, 5, dx=1))
        assert np.array_equal(got, want), (w, h, "odd pitch, planar")
        got = _convert_checked(e, yc.LAYOUT_GENERIC, _window(y, 7, dx=3), _window(yc.interleave(u, v), 3, dx=1), None)
        assert np.array_equal(got, want), (w, h, "odd pitch, nv12")
    # an aligned pitch: the block kernel on a window
    y, u, v = yc.planes(20, 6, "420", seed=14)
    got = _convert_checked(e, yc.LAYOUT_420_PLANAR, _window(y, 12, dx=8), _window(u, 6, dx=4), _window(v, 6, dx=4))
    assert np.array_equal(got, r.convert_yuv(y, u, v))


def test_convert_destination_views(engine):
    import caffe_rtpose_amd as r
    torch = _torch()
    e = engine
    for w, h in ((64, 48), (67, 45)):
        y, u, v = yc.planes(w, h, "420", seed=17)
        want = r.convert_yuv(y, u, v)
        dy, du, dv = _dev(y), _dev(u), _dev(v)
        assert np.array_equal(_convert(e, dy, du, dv), want)
        assert np.array_equal(_convert(e, dy, du, dv, order="rgb"), want[..., ::-1])
        for order in ("bgr", "rgb"):
            out = torch.full((h, w, 4), 201, dtype=torch.uint8, device="cuda")
            got = _convert(e, dy, du, dv, out=out[..., :3], order=order)
            full = out.cpu().numpy()
            assert (full[..., 3] == 201).all(), "the 4th byte of the destination was written"
            assert np.array_equal(full[..., :3], want if order == "bgr" else want[..., ::-1])
        for dx, dyy, extra in ((16, 8, 64), (7, 11, 71)):   # a window of a larger image: aligned pitch / odd pitch and start
            big = torch.full((h + 2 * dyy, w + extra, 3), 5, dtype=torch.uint8, device="cuda")
            _convert(e, dy, du, dv, out=big[dyy:dyy + h, dx:dx + w])
            full = big.cpu().numpy()
            assert np.array_equal(full[dyy:dyy + h, dx:dx + w], want)
            full[dyy:dyy + h, dx:dx + w] = 5
            assert (full == 5).all(), "bytes outside the destination window were written"
        planar = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda")   # CHW RGB
        torch.cuda.synchronize()
        e.convert_yuv_device(dy, du, dv, planar, order="rgb")
        torch.cuda.synchronize()
        assert np.array_equal(planar.cpu().numpy().transpose(1, 2, 0)[..., ::-1], want)
    with pytest.raises(r.RtpError) as ex:
        e.convert_yuv_device(dy, du, dv, torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda"))
    assert ex.value.code == r.RTP_EINVAL and "64 x 48" in str(ex.value)


class _Fake:
    def __init__(self, ptr, shape, strides=None):
        self.__cuda_array_interface__ = dict(typestr="|u1", shape=shape, strides=strides, data=(ptr, False), version=2)
        self.shape = shape


def _exact(e, a, pool):
    """`a` in a device allocation of exactly its bytes (rtp_device_alloc: one hipMalloc each): the plane ends with its allocation"""
    a = np.ascontiguousarray(a)
    p = e.device_alloc(a.nbytes)
    pool.append(p)
    e.device_upload(p, a)
    return _Fake(p, a.shape)


def test_planes_that_end_with_their_allocations(engine):
    """Every plane is the whole of its own allocation: a kernel (or a host check) that looks one element past the last chroma sample
    shows as a wrong refusal here; the host check itself is tested with a plane one byte short."""
    import caffe_rtpose_amd as r
    e = engine
    pool = []
    try:
        for w, h, layout in ((64, 48, "planar"), (64, 48, "nv12"), (4, 2, "nv12"), (67, 45, "planar"), (67, 45, "nv12"), (5, 4, "nv21"), (1, 1, "planar"), (3, 3, "planar")):
            y, u, v = yc.planes(w, h, "420", seed=19)
            want = r.convert_yuv(y, u, v)
            if layout == "planar":
                got = _convert(e, _exact(e, y, pool), _exact(e, u, pool), _exact(e, v, pool))
            else:
                order = "uv" if layout == "nv12" else "vu"
                got = _convert(e, _exact(e, y, pool), _exact(e, yc.interleave(u, v, order), pool), None, interleaved_order=order)
            assert np.array_equal(got, want), (w, h, layout)
        for fmt in ("422", "444", "mono"):
            y, u, v = yc.planes(67, 45, fmt, seed=23)
            got = _convert(e, _exact(e, y, pool), None if u is None else _exact(e, u, pool), None if v is None else _exact(e, v, pool))
            assert np.array_equal(got, r.convert_yuv(y, u, v)), fmt
    finally:
        e.synchronize()
        for p in pool:
            e.device_free(p)


def _frame(w, h, i, seed):
    """(planes, the BGR pixels the library makes of them) of a synthetic frame"""
    import caffe_rtpose_amd as r
    y, u, v = yc.from_bgr(r.synth_frame(w, h, i, seed=seed))
    return (y, u, v), r.convert_yuv(y, u, v)


def _host_bgr(e, bgr, tag, jpeg):
    fs = e.submit_frame(bgr, tag=tag)
    t, n, j, img = e.collect_rendered_jpeg() if jpeg else e.collect_rendered()
    assert t == tag
    return fs, n, j, img


def _submit(e, how, planes, tag, keep):
    """Submit the planes as host I420, device I420 or device NV12; device tensors go to `keep` (they must outlive the collect)."""
    y, u, v = planes
    if how == "host_i420":
        return e.submit_frame_yuv(y, u, v, tag=tag)
    torch = _torch()
    dev = [_dev(y), _dev(u), _dev(v)] if how == "dev_i420" else [_dev(y), _dev(yc.interleave(u, v))]
    keep.extend(dev)
    torch.cuda.synchronize()
    return e.submit_frame_yuv_device(*dev, tag=tag)


def _same(a, b, what):
    assert a[0] == b[0], f"{what}: frame_scale {a[0]} != {b[0]}"
    assert a[1] == b[1], f"{what}: num_people {a[1]} != {b[1]}"
    assert np.array_equal(a[2], b[2]), f"{what}: joints differ"
    if isinstance(a[3], bytes):
        assert a[3] == b[3], f"{what}: JPEG files differ ({len(a[3])} and {len(b[3])} bytes)"
    else:
        assert np.array_equal(a[3], b[3]), f"{what}: rendered frames differ in {int((a[3] != b[3]).any(-1).sum())} pixels"


@pytest.mark.parametrize("size", [(1280, 720), (640, 480), (67, 45)], ids=["display_size", "warp", "odd_enlarging_warp"])
def test_submitted_yuv_frames_equal_bgr_frames(engine, size):
    e = engine
    w, h = size
    torch = _torch()
    people = 0
    try:
        for jpeg in (False, True):
            e.set_render_jpeg(98 if jpeg else 0)
            for i, how in enumerate(("host_i420", "dev_nv12", "dev_i420")):
                planes, bgr = _frame(w, h, i, seed=41)
                want = _host_bgr(e, bgr, 2 * i, jpeg)
                keep = []
                fs = _submit(e, how, planes, 2 * i + 1, keep)
                t, n, j, img = e.collect_rendered_jpeg() if jpeg else e.collect_rendered()
                assert t == 2 * i + 1
                _same((fs, n, j, img), want, f"{w}x{h} {how} jpeg={jpeg}")
                people += n
    finally:
        e.set_render_jpeg(0)
    assert people > 0 or w < 100, "the test frames produced no people: nothing was drawn"


def test_host_planes_with_a_column_stride_of_two(engine):
    """u and v as every second column of two separate host arrays (uv_pixel_stride 2 without a neighbouring partner plane): staged as
    two planes, same result as the BGR path; at the display size and through the warp"""
    e = engine
    for k, (w, h) in enumerate(((1280, 720), (640, 480), (67, 45))):
        (y, u, v), bgr = _frame(w, h, k, seed=43)
        wide_u, wide_v = np.full((u.shape[0], 2 * u.shape[1]), 7, np.uint8), np.full((u.shape[0], 2 * u.shape[1]), 9, np.uint8)
        wide_u[:, ::2], wide_v[:, ::2] = u, v
        want = _host_bgr(e, bgr, 2 * k, False)
        fs = e.submit_frame_yuv(y, wide_u[:, ::2], wide_v[:, ::2], tag=2 * k + 1)
        t, n, j, img = e.collect_rendered()
        assert t == 2 * k + 1
        _same((fs, n, j, img), want, f"{w}x{h} column stride 2")


def _mixed_run(e, mixed, nframes=9):
    """Alternating YUV and BGR frames in one FIFO (sizes alternate as well); returns [(tag, n, joints)] and the frame scales."""
    sizes = [(1280, 720), (640, 480), (67, 45)]
    out, scales = [], []
    for i in range(nframes):
        planes, bgr = _frame(*sizes[i % 3], i, seed=47)
        scales.append(e.submit_frame_yuv(*planes, tag=100 + i) if mixed and i % 2 == 0 else e.submit_frame(bgr, tag=100 + i))
        while e.in_flight() >= 4:
            out.append(e.collect())
    while e.in_flight():
        out.append(e.collect())
    return out, scales


def _digest(results):
    h = hashlib.sha256()
    for t, n, j in results:
        h.update(np.int64([t, n]).tobytes() + j.tobytes())
    return h.hexdigest()


def _mixed_digest():
    e = _engine(batch_frames=2, frames_in_flight=4)
    out, _ = _mixed_run(e, True)
    e.close()
    return _digest(out)


def test_yuv_and_bgr_frames_share_one_fifo():
    e = _engine(batch_frames=2, frames_in_flight=4)
    host, hs = _mixed_run(e, False)
    mixed, ms = _mixed_run(e, True)
    e.close()
    assert [t for t, _, _ in mixed] == [100 + i for i in range(9)]
    assert hs == ms
    for (ta, na, ja), (tb, nb, jb) in zip(host, mixed):
        assert ta == tb and na == nb and np.array_equal(ja, jb), ta
    assert sum(n for _, n, _ in host) > 0


def test_deferred_preprocessing_knows_the_slot_holds_yuv():
    """The experiments build's RTP_PREP_DEFER=1 launches a host frame's kernels once its copy is done: the slot carries the format."""
    import caffe_rtpose_amd as r
    exp = os.path.join(ROOT, "caffe_rtpose_amd", "librtpose_mi355x_exp.so")
    want = _mixed_digest()
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTP_")}
    env.update(RTP_LIB=exp, RTP_PREP_DEFER="1")
    code = ("import sys; sys.path[:0] = [%r, %r]; import torch; import test_yuv_frames as t; print('digest', t._mixed_digest())") % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert [l for l in out.stdout.splitlines() if l.startswith("digest")][-1].split()[1] == want


def test_submit_is_ordered_on_the_callers_stream(engine):
    """The planes are written on a busy side stream and zeroed right after the submit on the same stream, without a host wait: the
    engine reads them after the write and before the zeroing."""
    torch = _torch()
    e = engine
    for k, (w, h) in enumerate(((1920, 1080), (1280, 720))):
        (y, u, v), bgr = _frame(w, h, 3, seed=53)
        want = _host_bgr(e, bgr, 1, False)
        src = [_dev(y), _dev(yc.interleave(u, v))]
        dst = [torch.empty_like(t) for t in src]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            torch.cuda._sleep(50_000_000)
            for a, b in zip(dst, src):
                a.copy_(b)
            fs = e.submit_frame_yuv_device(dst[0], dst[1], tag=2, stream=s)
            for a in dst:
                a.zero_()
        t, n, j, img = e.collect_rendered()
        assert t == 2
        _same((fs, n, j, img), want, f"stream-ordered submit {w}x{h}")
        torch.cuda.synchronize()
        assert all(bool((a == 0).all()) for a in dst)


def _still_usable(e, tag):
    (y, u, v), _ = _frame(640, 480, 1, seed=61)
    torch = _torch()
    planes = (_dev(y), _dev(u), _dev(v))
    torch.cuda.synchronize()
    e.submit_frame_yuv_device(*planes, tag=tag)
    assert e.collect()[0] == tag


def test_refusals_leave_the_engine_usable(engine):
    import caffe_rtpose_amd as r
    torch = _torch()
    e = engine
    (y, u, v), _ = _frame(640, 480, 0, seed=67)

    def refused(call, *words):
        with pytest.raises(r.RtpError) as ex:
            call()
        assert ex.value.code == r.RTP_EINVAL, ex.value
        for w in words:
            assert w in str(ex.value), ex.value

    # host arrays: refused by the Python layer; pinned host memory behind a forged interface: by the library's pointer check, per plane
    with pytest.raises(TypeError):
        e.submit_frame_yuv_device(y, u, v)
    dy, du, dv = _dev(y), _dev(u), _dev(v)
    torch.cuda.synchronize()
    pin = torch.from_numpy(u).pin_memory()
    refused(lambda: e.submit_frame_yuv_device(dy, _Fake(pin.data_ptr(), u.shape), dv, stream=0), "host", " u ")
    piny = torch.from_numpy(y).pin_memory()
    refused(lambda: e.submit_frame_yuv_device(_Fake(piny.data_ptr(), y.shape), du, dv, stream=0), "host", " y ")
    out = torch.zeros((480, 640, 3), dtype=torch.uint8, device="cuda")
    refused(lambda: e.convert_yuv_device(dy, du, _Fake(pin.data_ptr(), u.shape), out, stream=0), "host", " v ")
    _still_usable(e, 10)
    # a u plane one byte too short for its allocation (y and v are fine)
    pool = []
    try:
        short = e.device_alloc(u.nbytes - 1)
        pool.append(short)
        refused(lambda: e.submit_frame_yuv_device(dy, _Fake(short, u.shape), dv, stream=0), "allocation", "past u")
        refused(lambda: e.convert_yuv_device(dy, _Fake(short, u.shape), dv, out, stream=0), "allocation", "past u")
        exact = _exact(e, u, pool)
        e.submit_frame_yuv_device(dy, exact, dv, tag=11, stream=0)
        assert e.collect()[0] == 11
    finally:
        e.synchronize()
        for p in pool:
            e.device_free(p)
    _still_usable(e, 12)
    # a capturing stream (the capture is opened and closed, never replayed)
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    with torch.cuda.graph(g):
        x.add_(1)
        refused(lambda: e.submit_frame_yuv_device(dy, du, dv, tag=14, stream=torch.cuda.current_stream()), "capturing")
        refused(lambda: e.convert_yuv_device(dy, du, dv, out, stream=torch.cuda.current_stream()), "capturing")
    del g
    _still_usable(e, 15)
    assert e.in_flight() == 0


def test_cli_reads_y4m_planes(tmp_path):
    """rtpose.bin --video clip.y4m: the planes go to rtp_submit_frame_yuv; --host_yuv converts on the producer thread.  Same files."""
    import caffe_rtpose_amd as r
    clip = tmp_path / "clip.y4m"
    with open(clip, "wb") as f:
        f.write(b"YUV4MPEG2 W320 H180 F25:1 Ip A1:1 C420jpeg\n")
        for i in range(8):
            y, u, v = yc.from_bgr(r.synth_frame(320, 180, i, seed=5))
            f.write(b"FRAME\n" + y.tobytes() + u.tobytes() + v.tobytes())
    files = {}
    for mode in ("gpu", "host"):
        out = {k: tmp_path / f"{mode}_{k}" for k in ("json", "frames")}
        p = subprocess.run([BIN, "--video", str(clip), "--model", "coco", "--net_resolution", "160x96", "--resolution", "320x180", "--write_json", str(out["json"]),
                            "--write_frames", str(out["frames"]), "--no_frame_drops", "--no_display", "--num_gpu", "1"] + (["--host_yuv"] if mode == "host" else []),
                           capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        files[mode] = {(k, f): open(d / f, "rb").read() for k, d in out.items() for f in sorted(os.listdir(d))}
    assert len(files["gpu"]) == 16, sorted(files["gpu"])
    assert files["gpu"] == files["host"]
    help_ = subprocess.run([BIN, "--help"], capture_output=True, timeout=60)
    assert b"--host_yuv" in help_.stdout

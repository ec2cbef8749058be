"""YUV output on the GPU.  rtp_convert_to_yuv_device against rtp_convert_bgr_to_yuv byte for byte (the whole BGR cube through both
kernels; the 4 x 2 kernel and the generic one at every size, layout and alignment at which the choice or the addressing changes, with
guard bytes around every plane), the YUV mode of the renderer and rtp_collect_rendered_yuv_device against the raw rendered frames of the
same engine, the mode's refusals, and rtpose.bin --write_video with and without --host_video.  Integer arithmetic: no tolerances."""
import os
import subprocess

import numpy as np
import pytest

import _yuvoutcases as oc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
NET_W, NET_H = 160, 96
DISP_W, DISP_H = 320, 180
BLOCK = {"planar": oc.LAYOUT_420_PLANAR, "nv12": oc.LAYOUT_420_NV12, "nv21": oc.LAYOUT_420_NV21}


def _torch():
    import torch   # (tests/conftest.py imported it before the engine library: one HIP runtime for both)
    return torch


def _engine(**kw):
    import caffe_rtpose_amd as r
    kw = dict(dict(net_w=NET_W, net_h=NET_H, disp_w=DISP_W, disp_h=DISP_H, frames_in_flight=4, batch_frames=2, render=1), **kw)
    e = r.Engine(r.Config(**kw))
    t = r.default_thresholds(e.cfg.c.model)
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], 2, 0.05)   # keep more "people" of the noise maps
    return e


@pytest.fixture(scope="module")
def engine():
    e = _engine()
    yield e
    e.close()


class DevPlanes(oc.HostPlanes):
    """HostPlanes whose guard arrays live on the device while a kernel writes them: .dev = the windows as torch tensors (what
    convert_to_yuv_device takes), fetch() copies the arrays back so that planes() / guards_intact() judge what the GPU wrote."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        torch = _torch()
        self.tbig = [torch.from_numpy(b).cuda() for b in self.big]
        win = [self.tbig[0][2:2 + self.h, self.dx:self.dx + self.w]] + [t[2:2 + self.ch, self.dx:self.dx + self.cw] for t in self.tbig[1:]]
        self.dev = (tuple(win) + (None, None))[:3]

    def fetch(self):
        for b, t in zip(self.big, self.tbig):
            b[...] = t.cpu().numpy()
        return self


def _export(e, src_dev, img, fmt, layout="planar", extra=0, dx=0, order="bgr", kernel=None, what=""):
    """convert_to_yuv_device of the device frame `src_dev` (whose pixels are `img`, BGR) into guarded planes; everything is checked"""
    import caffe_rtpose_amd as r
    torch = _torch()
    h, w = img.shape[:2]
    dst = DevPlanes(w, h, fmt, layout, extra, dx)
    if kernel is not None:
        assert oc.layout(src_dev, *dst.dev, order=order, interleaved_order=dst.order) == kernel, f"{what}: kernel choice, wanted layout {kernel}"
    before = src_dev.clone()
    torch.cuda.synchronize()
    e.convert_to_yuv_device(src_dev, *dst.dev, order=order, interleaved_order=dst.order)
    torch.cuda.synchronize()
    dst.fetch()
    want = r.convert_bgr_to_yuv(img, {"420": 420, "422": 422, "444": 444, "mono": 400}[fmt])
    for name, got, ref in zip("yuv", dst.planes(), want):
        assert (got is None) == (ref is None)
        if ref is not None:
            assert np.array_equal(got, ref), f"{what} {fmt} {layout} {w}x{h}: plane {name} differs in {int((got != ref).sum())} samples"
    assert dst.guards_intact(), f"{what} {fmt} {layout} {w}x{h}: a byte outside the planes (guard rows or pitch padding) was written"
    assert bool((src_dev == before).all()), f"{what}: the source was written"


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("layout", ["planar", "nv12", "nv21"])
def test_block_kernel(engine, layout):
    """w % 4 == 0, h % 2 == 0, packed BGR, aligned planes: the 4 x 2 kernel.  260 x 2: 65 blocks, a grid tail inside a workgroup."""
    for w, h in ((64, 48), (260, 2), (4, 2)):
        img = oc.image(w, h, seed=3)
        _export(engine, _dev(img), img, "420", layout, kernel=BLOCK[layout], what="block kernel")
    img = oc.image(64, 48, seed=4)
    _export(engine, _dev(img), img, "420", layout, extra=12, kernel=BLOCK[layout], what="pitched destination")
    _export(engine, _dev(img), img, "420", layout, extra=12, dx=8, kernel=BLOCK[layout], what="destination window")
    # the source as a crop of a larger image (its first pixel and its pitch are 4-byte aligned)
    torch = _torch()
    big = torch.full((48 + 10, 64 + 20, 3), 0x33, dtype=torch.uint8, device="cuda")
    big[4:4 + 48, 8:8 + 64] = _dev(img)
    _export(engine, big[4:4 + 48, 8:8 + 64], img, "420", layout, kernel=BLOCK[layout], what="cropped source")
    full = big.cpu().numpy()
    full[4:4 + 48, 8:8 + 64] = 0x33
    assert (full == 0x33).all()


def test_generic_kernel_sizes_and_samplings(engine):
    for w, h in ((1, 1), (3, 5), (17, 9)):
        img = oc.image(w, h, seed=5)
        for layout in ("planar", "nv12", "nv21"):
            _export(engine, _dev(img), img, "420", layout, kernel=oc.LAYOUT_GENERIC, what="odd size")
    for w, h in ((1, 1), (3, 5), (17, 9), (64, 48)):
        img = oc.image(w, h, seed=6)
        for fmt, layout in (("422", "planar"), ("444", "planar"), ("mono", "mono"), ("422", "nv12"), ("444", "nv21")):
            _export(engine, _dev(img), img, fmt, layout, extra=3 if w > 1 else 0, kernel=oc.LAYOUT_GENERIC, what="sampling")


def test_generic_kernel_sources_and_misalignment(engine):
    torch = _torch()
    for w, h in ((64, 48), (17, 9)):
        img = oc.image(w, h, seed=7)
        bgra = torch.full((h, w, 4), 0x44, dtype=torch.uint8, device="cuda")
        bgra[..., :3] = _dev(img)
        _export(engine, bgra[..., :3], img, "420", "planar", kernel=oc.LAYOUT_GENERIC, what="BGRA source")
        assert bool((bgra[..., 3] == 0x44).all())
        rgba = torch.full((h, w, 4), 0x44, dtype=torch.uint8, device="cuda")
        rgba[..., :3] = _dev(img[..., ::-1])
        _export(engine, rgba[..., :3], img, "420", "nv12", order="rgb", kernel=oc.LAYOUT_GENERIC, what="RGBA source")
        chw = _dev(img[..., ::-1].transpose(2, 0, 1))   # planar RGB
        _export(engine, chw, img, "420", "planar", order="rgb", kernel=oc.LAYOUT_GENERIC, what="planar RGB source")
        _export(engine, chw, img, "444", "planar", order="rgb", kernel=oc.LAYOUT_GENERIC, what="planar RGB source")
    # w % 4 == 0 and h % 2 == 0 and packed BGR, but planes at odd addresses with odd pitches, or a source at an odd address: the fall-back
    img = oc.image(64, 48, seed=8)
    for layout in ("planar", "nv12", "nv21"):
        _export(engine, _dev(img), img, "420", layout, extra=3, dx=1, kernel=oc.LAYOUT_GENERIC, what="misaligned planes")
    big = torch.full((48, 64 + 3, 3), 0x33, dtype=torch.uint8, device="cuda")
    big[:, 1:65] = _dev(img)
    _export(engine, big[:, 1:65], img, "420", "planar", kernel=oc.LAYOUT_GENERIC, what="misaligned source")
    # aligned luma, chroma planes at an odd address only
    dst = DevPlanes(64, 48, "420", "planar", 0, 0)
    odd = [torch.full((48 // 2 + 4, 32 + 1), oc.GUARD, dtype=torch.uint8, device="cuda") for _ in range(2)]
    assert oc.layout(_dev(img), dst.dev[0], odd[0][2:26, 1:33], odd[1][2:26, 1:33]) == oc.LAYOUT_GENERIC


def test_whole_cube_through_both_kernels(engine):
    """Every BGR triple through the 4 x 2 kernel's own unpacking and packing (4:2:0, planar and NV12) and through the generic kernel
    (4:4:4): the guard against the compiler pairing shifts into packed instructions with other semantics."""
    torch = _torch()
    src = _torch().from_numpy(oc.cube().copy()).cuda()   # (the cached cube is read-only)
    for fmt, layout, kernel in (("420", "planar", oc.LAYOUT_420_PLANAR), ("420", "nv12", oc.LAYOUT_420_NV12), ("444", "planar", oc.LAYOUT_GENERIC)):
        want = oc.cube_planes(fmt)
        ch, cw = want[1].shape
        y = torch.zeros((4096, 4096), dtype=torch.uint8, device="cuda")
        if layout == "planar":
            planes = (y, torch.zeros((ch, cw), dtype=torch.uint8, device="cuda"), torch.zeros((ch, cw), dtype=torch.uint8, device="cuda"))
        else:
            planes = (y, torch.zeros((ch, cw, 2), dtype=torch.uint8, device="cuda"), None)
        assert oc.layout(src, *planes) == kernel
        torch.cuda.synchronize()
        engine.convert_to_yuv_device(src, *planes)
        torch.cuda.synchronize()
        got = [p.cpu().numpy() for p in planes if p is not None]
        if layout == "nv12":
            got = [got[0], got[1][..., 0], got[1][..., 1]]
        for name, a, b in zip("yuv", got, want):
            assert np.array_equal(a, b), f"{fmt} {layout}: plane {name} differs in {int((a != b).sum())} of {b.size} samples"


def _frames(n=3, seed=21):
    import caffe_rtpose_amd as r
    sizes = [(DISP_W, DISP_H), (640, 360), (DISP_W, DISP_H)]   # at the display size, and through the warp
    return [r.synth_frame(*sizes[i % 3], i, seed=seed) for i in range(n)]


def _raw_and_yuv(e, frames):
    """The frames through `e` in raw mode and then in YUV mode (a batch of 2 and a flushed batch of 1): planes = rtp_convert_bgr_to_yuv
    of the raw rendered frames, joints identical.  Returns the raw results."""
    import caffe_rtpose_amd as r
    raw, yuv = [], []
    try:
        for mode, out, collect in ((0, raw, e.collect_rendered), (420, yuv, e.collect_rendered_yuv)):
            e.set_render_yuv(mode)
            for i, f in enumerate(frames):
                e.submit_frame(f, tag=10 + i)
            while e.in_flight():
                out.append(collect())
    finally:
        e.set_render_yuv(0)
    assert len(raw) == len(yuv) == len(frames)
    for i, ((t0, n0, j0, img), (t1, j1, y, u, v)) in enumerate(zip(raw, yuv)):
        assert t0 == t1 == 10 + i
        assert n0 == len(j1) and np.array_equal(j0, j1), f"frame {i}: joints differ between raw and YUV mode"
        for name, got, want in zip("yuv", (y, u, v), r.convert_bgr_to_yuv(img)):
            assert np.array_equal(got, want), f"frame {i}: plane {name} differs in {int((got != want).sum())} samples"
    return raw


def test_renderer_mode_graph_replay(engine):
    raw = _raw_and_yuv(engine, _frames())
    assert sum(n for _, n, _, _ in raw) > 0, "the test frames produced no people: nothing was drawn"


def test_renderer_mode_eager():
    import caffe_rtpose_amd as r
    e = _engine(exec_mode=r.EXEC_EAGER)
    try:
        _raw_and_yuv(e, _frames())
    finally:
        e.close()


def test_renderer_mode_part_to_show_view():
    e = _engine(render=2)   # part_to_show 1: a heat-map view
    try:
        raw = _raw_and_yuv(e, _frames(2))
        assert not np.array_equal(raw[0][3], _frames(2)[0]), "the view equals the input frame: nothing was rendered"
    finally:
        e.close()


def test_collect_into_a_pitched_nv12_surface(engine):
    """rtp_collect_rendered_yuv_device on a caller's stream, in raw mode and in YUV mode: the planes of the same rendered frame"""
    import caffe_rtpose_amd as r
    torch = _torch()
    e = engine
    frame = _frames(1, seed=23)[0]
    e.submit_frame(frame, tag=1)
    _, n0, j0, img = e.collect_rendered()
    want = r.convert_bgr_to_yuv(img)
    try:
        for mode in (0, 420):
            e.set_render_yuv(mode)
            ybig = torch.full((DISP_H, DISP_W + 64), oc.GUARD, dtype=torch.uint8, device="cuda")
            cbig = torch.full((DISP_H // 2, DISP_W // 2 + 32, 2), oc.GUARD, dtype=torch.uint8, device="cuda")
            y, uv = ybig[:, :DISP_W], cbig[:, :DISP_W // 2]
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            e.submit_frame(frame, tag=2)
            t, n, j = e.collect_rendered_yuv_device(y, uv, stream=s)
            s.synchronize()
            assert (t, n) == (2, n0) and np.array_equal(j, j0)
            yh, ch = ybig.cpu().numpy(), cbig.cpu().numpy()
            assert np.array_equal(yh[:, :DISP_W], want[0]) and np.array_equal(ch[:, :DISP_W // 2, 0], want[1]) and np.array_equal(ch[:, :DISP_W // 2, 1], want[2]), mode
            assert (yh[:, DISP_W:] == oc.GUARD).all() and (ch[:, DISP_W // 2:] == oc.GUARD).all(), "pitch padding was written"
            # NULL stream: complete when the call returns; planar I420 this time
            planes = [torch.zeros(p.shape, dtype=torch.uint8, device="cuda") for p in want]
            torch.cuda.synchronize()
            e.submit_frame(frame, tag=3)
            assert e.collect_rendered_yuv_device(*planes, stream=0)[0] == 3
            assert all(np.array_equal(p.cpu().numpy(), q) for p, q in zip(planes, want)), mode
        # a view of another size is refused before the frame leaves the FIFO
        e.submit_frame(frame, tag=4)
        small = [torch.zeros((90, 160), dtype=torch.uint8, device="cuda"), torch.zeros((45, 80, 2), dtype=torch.uint8, device="cuda")]
        with pytest.raises(r.RtpError) as ex:
            e.collect_rendered_yuv_device(*small, stream=0)
        assert ex.value.code == r.RTP_EINVAL and "320 x 180" in str(ex.value) and e.in_flight() == 1
        assert e.collect_rendered_yuv()[0] == 4
    finally:
        e.set_render_yuv(0)


def test_mode_refusals(engine):
    import ctypes as C
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd._lib import lib
    e = engine
    frame = _frames(1, seed=25)[0]

    def refused(call, code, *words):
        with pytest.raises(r.RtpError) as ex:
            call()
        assert ex.value.code == code, ex.value
        for w in words:
            assert w in str(ex.value), ex.value

    try:
        refused(lambda: e.set_render_yuv(422), r.RTP_EINVAL, "422")
        refused(lambda: e.set_render_yuv(1), r.RTP_EINVAL)
        refused(e.collect_rendered_yuv, r.RTP_EINVAL, "rtp_set_render_yuv")            # mode off
        e.submit_frame(frame, tag=1)
        refused(lambda: e.set_render_yuv(420), r.RTP_EAGAIN, "in flight")              # frames in flight
        assert e.collect_rendered()[0] == 1
        e.set_render_jpeg(90)
        refused(lambda: e.set_render_yuv(420), r.RTP_EINVAL, "JPEG mode")              # the two modes exclude each other, both ways
        e.set_render_jpeg(0)
        e.set_render_yuv(420)
        refused(lambda: e.set_render_jpeg(90), r.RTP_EINVAL, "YUV mode")
        e.set_render_jpeg(0)                                                           # (switching JPEG mode off stays legal)
        e.submit_frame(frame, tag=2)
        refused(e.collect_rendered, r.RTP_EINVAL, "rtp_collect_rendered_yuv")          # the message names the right entry
        assert e.in_flight() == 1
        # a capacity that is too small leaves the frame collectable
        tag, n = C.c_uint64(), C.c_int()
        joints = np.zeros((r.MAX_PEOPLE, e.num_parts, 3), np.float32)
        need = r.yuv_bytes(DISP_W, DISP_H)
        buf = np.zeros(need, np.uint8)
        rc = lib.rtp_collect_rendered_yuv(e.h, C.byref(tag), joints.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n), buf.ctypes.data_as(C.POINTER(C.c_ubyte)), need - 1)
        assert rc == r.RTP_EINVAL and str(need) in lib.rtp_last_error(e.h).decode() and e.in_flight() == 1
        assert e.collect_rendered_yuv()[0] == 2
        # a frame submitted as a net input has no display image: refused, still collectable with collect()
        e.submit(np.zeros((1, 3, NET_H, NET_W), np.float32), tag=3)
        refused(e.collect_rendered_yuv, r.RTP_EINVAL, "no display image")
        assert e.in_flight() == 1 and e.collect()[0] == 3
        e.set_render_yuv(0)
        e.submit_frame(frame, tag=4)
        assert e.collect_rendered()[0] == 4                                             # raw mode works again
    finally:
        while e.in_flight():
            e.collect()
        e.set_render_jpeg(0)
        e.set_render_yuv(0)
    off = _engine(render=0)
    try:
        refused(lambda: off.set_render_yuv(420), r.RTP_EINVAL, "render")
        off.set_render_yuv(0)
    finally:
        off.close()


@pytest.mark.parametrize("suffix", ["y4m", "mjpeg"])
def test_cli_gpu_and_host_video_are_the_same_bytes(tmp_path, suffix):
    """rtpose.bin --write_video: converted / encoded on the GPU, and with --host_video on the host: byte-identical files"""
    import caffe_rtpose_amd as r
    files = {}
    for mode in ("gpu", "host"):
        out = tmp_path / f"{mode}.{suffix}"
        p = subprocess.run([BIN, "--video", "synthetic:320x180:6:5", "--model", "coco", "--net_resolution", "160x96", "--resolution", "320x180", "--write_video", str(out),
                            "--no_frame_drops", "--no_display", "--num_gpu", "1"] + (["--host_video"] if mode == "host" else []), capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        assert (b"on the GPU" in p.stderr) == (mode == "gpu"), p.stderr.decode()[-3000:]
        files[mode] = open(out, "rb").read()
    assert files["gpu"] == files["host"] and len(files["gpu"]) > 0
    vid = r.Video(tmp_path / f"gpu.{suffix}")
    assert (vid.w, vid.h_, vid.nframes) == (320, 180, 6)
    vid.close()

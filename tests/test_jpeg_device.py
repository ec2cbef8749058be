"""JPEG files encoded on the GPU (rtp_encode_jpeg_device, rtp_set_render_jpeg / rtp_collect_rendered_jpeg) against rtp_encode_jpeg on
the host: the bytes must be identical, for libjpeg-turbo's own fixtures, a grid of sizes, qualities and contents, every frame layout,
the engine's rendered frames (overlay and part_to_show views, COCO and MPI) and the CLI's --write_frames files."""
import glob
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
GOLDEN = os.path.join(ROOT, "tests", "golden", "codecs")
NET_W, NET_H = 320, 176
DISP_W, DISP_H = 640, 368


def _torch():
    import torch   # (tests/conftest.py imported it before the engine library: one HIP runtime for both)
    return torch


@pytest.fixture(scope="module")
def enc():
    import caffe_rtpose_amd as r
    e = r.Engine(r.Config(net_w=NET_W, net_h=NET_H, disp_w=DISP_W, disp_h=DISP_H, frames_in_flight=2))
    yield e
    e.close()


def _dev(img):
    return _torch().from_numpy(np.ascontiguousarray(img)).cuda()


def _content(kind, w, h, seed=0):
    import caffe_rtpose_amd as r
    rng = np.random.default_rng(seed + w * 7919 + h)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 3) % 256], -1).astype(np.uint8)
    if kind == "synth":   # (synth_frame has a minimum size: crop a larger one)
        return np.ascontiguousarray(r.synth_frame(max(w, 64), max(h, 64), 3, seed=11)[:h, :w])
    if kind == "zeros":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "ones":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "checker":   # 1-pixel black / white: long codes, many 0xFF bytes
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    raise ValueError(kind)


def test_golden_fixtures_byte_identical(enc):
    files = sorted(glob.glob(os.path.join(GOLDEN, "enc_*.npy")))
    assert files
    for f in files:
        q = int(os.path.basename(f).split("_q")[1].split(".")[0])
        img = np.load(f)
        want = open(f[:-4] + ".jpgref", "rb").read()
        assert enc.encode_jpeg_device(_dev(img), q) == want, os.path.basename(f)


SMALL = [(1, 1), (2, 1), (7, 5), (15, 16), (16, 16), (17, 17), (33, 31), (65, 9)]
LARGE = [(656, 368), (1280, 720), (1920, 1080)]
KINDS = ["noise", "gradient", "synth", "zeros", "ones", "checker"]


def test_grid_small_sizes_every_quality(enc):
    import caffe_rtpose_amd as r
    for w, h in SMALL:
        for kind in KINDS:
            img = _content(kind, w, h)
            d = _dev(img)
            for q in (1, 25, 50, 75, 95, 98, 100):
                assert enc.encode_jpeg_device(d, q) == r.encode_jpeg(img, q), (w, h, kind, q)


@pytest.mark.parametrize("size", LARGE, ids=[f"{w}x{h}" for w, h in LARGE])
def test_grid_large_sizes(enc, size):
    import caffe_rtpose_amd as r
    w, h = size
    for kind in KINDS:
        img = _content(kind, w, h)
        d = _dev(img)
        for q in (98, 100):
            assert enc.encode_jpeg_device(d, q) == r.encode_jpeg(img, q), (w, h, kind, q)


def test_quality_is_clamped_like_the_host_encoder(enc):
    import caffe_rtpose_amd as r
    img = _content("synth", 40, 24)
    assert enc.encode_jpeg_device(_dev(img), 0) == r.encode_jpeg(img, 1)
    assert enc.encode_jpeg_device(_dev(img), 250) == r.encode_jpeg(img, 100)


def test_layouts_give_the_bytes_of_the_bgr_image(enc):
    import caffe_rtpose_amd as r
    import test_device_frames as tdf
    for w, h in ((1280, 720), (37, 23)):
        img = r.synth_frame(w, h, 5, seed=13)
        want = r.encode_jpeg(img, 98)
        for layout in ("bgr", "rgb", "bgra", "chw", "crop_odd"):
            t, order = tdf._to_device(img, layout)
            _torch().cuda.synchronize()
            assert enc.encode_jpeg_device(t, 98, order=order) == want, (w, h, layout)


def test_encode_is_ordered_on_the_callers_stream(enc):
    """The frame is written by work still queued on a busy side stream: the file is that of the final content."""
    import caffe_rtpose_amd as r
    torch = _torch()
    img = r.synth_frame(1280, 720, 9, seed=17)
    src = torch.from_numpy(img).cuda()
    frame = torch.zeros_like(src)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(50_000_000)
        frame.copy_(src)
        data = enc.encode_jpeg_device(frame, 98, stream=s)
    assert data == r.encode_jpeg(img, 98)


def _render_engine(model, render, jpeg):
    import caffe_rtpose_amd as r
    e = r.Engine(r.Config(net_w=NET_W, net_h=NET_H, disp_w=DISP_W, disp_h=DISP_H, frames_in_flight=4, batch_frames=2, render=render,
                          model=model))
    t = r.default_thresholds(model)
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], 2, 0.05)   # keep more "people" of the noise maps
    if jpeg:
        e.set_render_jpeg(98)
    return e


@pytest.mark.parametrize("model,render", [(0, 1), (0, 1 + 19), (1, 1), (1, 1 + 3)], ids=["coco", "coco_view", "mpi", "mpi_view"])
def test_engine_jpeg_mode_equals_host_encoding(model, render):
    import caffe_rtpose_amd as r
    sizes = [(1280, 720), (640, 480), (1920, 1080)]
    imgs = [r.synth_frame(*sizes[i % 3], i, seed=61) for i in range(7)]

    def run(jpeg):
        e = _render_engine(model, render, jpeg)
        devs = [_dev(im) for im in imgs]
        _torch().cuda.synchronize()
        out = []
        for i, im in enumerate(imgs):
            if i % 2:
                e.submit_frame_device(devs[i], tag=10 + i)
            else:
                e.submit_frame(im, tag=10 + i)
            while e.in_flight() >= 4:
                out.append(e.collect_rendered_jpeg() if jpeg else e.collect_rendered())
        while e.in_flight():
            out.append(e.collect_rendered_jpeg() if jpeg else e.collect_rendered())
        e.close()
        return out

    got, want = run(True), run(False)
    assert [g[0] for g in got] == [10 + i for i in range(7)]
    for (tg, ng, jg, data), (tw, nw, jw, img) in zip(got, want):
        assert tg == tw and ng == nw and np.array_equal(jg, jw), tg
        assert data == r.encode_jpeg(img, 98), f"frame {tg}"


def test_refusals_leave_the_engine_usable():
    import caffe_rtpose_amd as r
    img = r.synth_frame(1280, 720, 2, seed=67)
    e = _render_engine(0, 1, False)
    e.submit_frame(img, tag=1)
    with pytest.raises(r.RtpError) as ex:           # JPEG mode off
        e.collect_rendered_jpeg()
    assert ex.value.code == r.RTP_EINVAL
    with pytest.raises(r.RtpError) as ex:           # frames in flight
        e.set_render_jpeg(98)
    assert ex.value.code == r.RTP_EAGAIN
    for bad in (101, -1):                            # out of range, with the frame in flight
        with pytest.raises(r.RtpError) as ex:
            e.set_render_jpeg(bad)
        assert ex.value.code == r.RTP_EINVAL and e.in_flight() == 1
    _, n_raw, j_raw, raw = e.collect_rendered()     # the frame stayed in the FIFO
    e.set_render_jpeg(98)
    e.submit_frame(img, tag=2)
    with pytest.raises(r.RtpError) as ex:           # raw frames are not copied in JPEG mode
        e.collect_rendered()
    assert ex.value.code == r.RTP_EINVAL and "JPEG" in str(ex.value)
    from caffe_rtpose_amd._lib import lib
    import ctypes as C
    small = np.empty(r.jpeg_max_bytes(DISP_W, DISP_H) - 1, np.uint8)
    tag, n, nb = C.c_uint64(), C.c_int(), C.c_size_t()
    joints = np.zeros((r.MAX_PEOPLE, e.num_parts, 3), np.float32)
    rc = lib.rtp_collect_rendered_jpeg(e.h, C.byref(tag), joints.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n),
                                       small.ctypes.data_as(C.POINTER(C.c_ubyte)), small.size, C.byref(nb))
    assert rc == r.RTP_EINVAL and e.in_flight() == 1  # capacity too small
    t, n, j, data = e.collect_rendered_jpeg()
    assert t == 2 and n == n_raw and np.array_equal(j, j_raw) and data == r.encode_jpeg(raw, 98)
    torch = _torch()                                 # rtp_collect_rendered_device still works in JPEG mode
    e.submit_frame(img, tag=4)
    out = torch.zeros((DISP_H, DISP_W, 3), dtype=torch.uint8, device="cuda")
    t, n, j = e.collect_rendered_device(out)
    assert t == 4 and n == n_raw and np.array_equal(j, j_raw) and np.array_equal(out.cpu().numpy(), raw)
    e.set_render_jpeg(0)                             # off again: raw frames as before
    e.submit_frame(img, tag=3)
    assert np.array_equal(e.collect_rendered()[3], raw)
    e.close()
    e = r.Engine(r.Config(net_w=NET_W, net_h=NET_H, disp_w=DISP_W, disp_h=DISP_H, frames_in_flight=2))   # render = 0
    with pytest.raises(r.RtpError) as ex:
        e.set_render_jpeg(98)
    assert ex.value.code == r.RTP_EINVAL
    e.close()


def test_cli_gpu_encoder_equals_host_jpeg(tmp_path):
    for view in ([], ["--part_to_show", "19"]):
        files = {}
        for mode in ("gpu", "host"):
            out = tmp_path / f"{mode}{len(view)}"
            p = subprocess.run([BIN, "--video", "synthetic:640x480:4:5", "--model", "coco", "--net_resolution", "160x96", "--resolution",
                                "320x240", "--write_frames", str(out), "--no_frame_drops", "--no_display", "--num_gpu", "1"]
                               + view + (["--host_jpeg"] if mode == "host" else []), capture_output=True, timeout=600)
            assert p.returncode == 0, p.stderr.decode()
            assert (b"JPEG files encoded on the GPU" if mode == "gpu" else b"JPEG files encoded on the host") in p.stderr
            files[mode] = {f: open(out / f, "rb").read() for f in sorted(os.listdir(out))}
        assert sorted(files["gpu"]) == [f"frame{i:06d}.jpg" for i in range(4)]
        assert files["gpu"] == files["host"], view

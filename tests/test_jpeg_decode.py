"""JPEG files decoded on the GPU (rtp_decode_jpeg_device, rtp_submit_frame_jpeg, rtpose.bin without --host_decode) against
rtp_decode_image on the host: the pixels must be identical, for every fixture (baseline files through the device's Huffman decoder,
progressive ones through the host's), a grid of generated files at the production subsequence size and at one that spreads small
files over several workgroups, every destination layout, the reconstruction kernels alone on full-range coefficients, and
submitted frames (joints, frame_scale, rendered frames).  Where the Huffman decoding ran is asserted every time.
The layout fixtures (tests/golden/codecs/layouts) are compared with libjpeg's committed pixels instead: the device side has no other
test of MCU shapes beyond 1, 3, 4 and 6 blocks, of the up-sampling ratios beyond 2, or of the colour model handed over by the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _jpegcases as jc
import _yuvcases as yc

pytestmark = pytest.mark.gpu

ROOT = jc.ROOT
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
NET_W, NET_H = 320, 176
DISP_W, DISP_H = 640, 368


def _torch():
    import torch   # (tests/conftest.py imported it before the engine library: one HIP runtime for both)
    return torch


def _engine(**kw):
    import caffe_rtpose_amd as r
    kw = dict(dict(net_w=NET_W, net_h=NET_H, disp_w=DISP_W, disp_h=DISP_H, frames_in_flight=2, render=1), **kw)
    e = r.Engine(r.Config(**kw))
    t = r.default_thresholds(e.cfg.c.model)
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], 2, 0.05)   # keep more "people" of the noise maps
    return e


@pytest.fixture(scope="module")
def engine():
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def decoded():
    """rtp_decode_image of every file the tests use, computed once"""
    import caffe_rtpose_amd as r
    cache = {}

    def get(data):
        if data not in cache:
            cache[data] = r.decode_image(data)
        return cache[data]
    return get


def _decode(e, data, sub_bits=0, group=0, force_host=0, out=None, order="bgr"):
    """(device tensor, path, rounds) of the internal entry behind rtp_decode_jpeg_device (S and subsequences per workgroup as given)"""
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd.engine import _view_struct, frame_view
    torch = _torch()
    if out is None:
        w, h = C.c_int(), C.c_int()
        buf0 = (C.c_ubyte * len(data)).from_buffer_copy(data)
        assert r.lib.rtp_decode_image(buf0, len(data), None, 0, C.byref(w), C.byref(h)) == 0
        out = torch.full((h.value, w.value, 3), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    v = _view_struct(frame_view(out, order))
    path = C.c_int(-1)
    rounds = (C.c_int * 2)()
    rc = r.lib.rtp_internal_jpeg_decode_device(e.h, data, C.c_size_t(len(data)), C.byref(v), None, sub_bits, group, force_host, C.byref(path), rounds)
    if rc:
        raise r.RtpError(rc, r.lib.rtp_last_error(e.h).decode())
    return out, path.value, list(rounds)


def test_every_fixture_equals_the_host_decoder(engine, decoded):
    import caffe_rtpose_amd as r
    names = jc.BASELINE + jc.progressive_names()
    assert len(names) >= 15
    for name in names:
        data = jc.fixture(name)
        want = np.load(os.path.join(jc.GOLD, name + ".npy"))
        assert np.array_equal(decoded(data), want), name
        out, path = engine.decode_jpeg_device(data)
        assert path == (r.engine.JPEG_ENTROPY_HOST if name.startswith("jprog") else r.engine.JPEG_ENTROPY_DEVICE), (name, path)
        assert np.array_equal(out.cpu().numpy(), want), name
    # the reconstruction kernels on the host decoder's coefficients of a baseline file
    data = jc.fixture("j422_q85")
    out, path, _ = _decode(engine, data, force_host=1)
    assert path == jc.HOST and np.array_equal(out.cpu().numpy(), decoded(data))


@pytest.mark.parametrize("name", sorted(jc.LAYOUTS))
def test_layout_fixtures_equal_libjpeg(engine, name):
    """tests/golden/codecs/layouts against the committed libjpeg pixels (not the host decoder): MCUs of up to 10 blocks in every block
    map, restart interval 1, tables under id 3, h1v2 / x3 / x4 / luma up-sampling, latched quantisers, the colour model.  The DEVICE
    ones again with subsequences so small that their boundaries fall inside these MCUs and restart segments."""
    data, want = jc.layout(name)
    assert want.shape[0] <= 40 and want.shape[1] <= 48
    out, path = engine.decode_jpeg_device(data)
    assert path == jc.LAYOUTS[name], (name, path)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (name, int((got != want).any(-1).sum()))
    if jc.LAYOUTS[name] == jc.DEVICE:
        for s, g in ((32, 4), (64, 64)):
            out, path, rounds = _decode(engine, data, sub_bits=s, group=g)
            got = out.cpu().numpy()
            assert path == jc.DEVICE and np.array_equal(got, want), (name, s, g, rounds, int((got != want).any(-1).sum()))


def test_generated_grid_at_the_production_subsequence_size(engine, decoded):
    for name, data in jc.grid():
        out, path = engine.decode_jpeg_device(data)
        assert path == jc.DEVICE, name
        assert np.array_equal(out.cpu().numpy(), decoded(data)), name


def test_generated_grid_over_several_workgroups(engine, decoded):
    """S = 64 bits, 64 subsequences per workgroup: 4096 bits per workgroup, so the larger files need states carried from launch to launch"""
    spans = {}
    for name, data in jc.grid():
        out, path, rounds = _decode(engine, data, sub_bits=64, group=64)
        assert path == jc.DEVICE, name
        assert np.array_equal(out.cpu().numpy(), decoded(data)), (name, rounds)
        assert 1 <= rounds[0] <= max(rounds[1], 1), (name, rounds)
        spans[name] = rounds[1]
    assert spans["noise_65x9_q100"] >= 2 and spans["noise_33x31_q100"] >= 2 and spans["noise_301x173_q100"] >= 8, spans
    # and the smallest subsequences with tiny workgroups: boundaries inside almost every block and inside extra-bit fields
    for name in ("noise_33x31_q100", "checker_17x17_q75", "flat_7x5_q25"):
        data = dict(jc.grid())[name]
        out, path, rounds = _decode(engine, data, sub_bits=32, group=4)
        assert path == jc.DEVICE and np.array_equal(out.cpu().numpy(), decoded(data)), (name, rounds)
    data = jc.fixture("j420_rst")   # restart segments: several anchored subsequences
    out, path, rounds = _decode(engine, data, sub_bits=32, group=4)
    assert path == jc.DEVICE and np.array_equal(out.cpu().numpy(), decoded(data)), rounds


RECON = [
    ("420_16x16_full_range", 16, 16, 3, (2, 2, 1, 1, 1, 1), 0, 65535),
    ("420_odd", 35, 19, 3, (2, 2, 1, 1, 1, 1), 0, 255),
    ("420_narrow", 4, 9, 3, (2, 2, 1, 1, 1, 1), 0, 255),
    ("422", 21, 10, 3, (2, 1, 1, 1, 1, 1), 0, 65535),
    ("422_narrow", 3, 9, 3, (2, 1, 1, 1, 1, 1), 0, 255),
    ("440_h1v2", 19, 21, 3, (1, 2, 1, 1, 1, 1), 0, 255),
    ("444_rgb", 9, 9, 3, (1, 1, 1, 1, 1, 1), 1, 255),
    ("411_replicated", 37, 9, 3, (4, 1, 1, 1, 1, 1), 0, 255),
    ("mixed_ratios", 33, 17, 3, (2, 2, 2, 1, 1, 2), 0, 255),
    ("grey", 13, 11, 1, (1, 1), 0, 65535),
]


@pytest.mark.parametrize("case", RECON, ids=[c[0] for c in RECON])
def test_reconstruction_alone_equals_the_host_counterpart(engine, case):
    """random full-range int16 coefficients and 16-bit quantisers: dequantise + IDCT (64-bit, & 1023 wrap) + up-sampling + colour"""
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd.engine import _view_struct, frame_view
    name, w, h, nc, hv, rgb, qmax = case
    rng = np.random.default_rng(len(name) * 131 + w)
    hmax, vmax = (max(hv[0::2]), max(hv[1::2])) if nc == 3 else (1, 1)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    blocks = sum(mcux * (hv[2 * c] if nc == 3 else 1) * mcuy * (hv[2 * c + 1] if nc == 3 else 1) for c in range(nc))
    qn = rng.integers(1, qmax + 1, (nc, 64)).astype(np.uint16)
    qn[:, 0] = qmax
    hvc = (C.c_int * len(hv))(*hv)
    torch = _torch()
    for kind in ("full", "sparse"):
        coef = rng.integers(-32768, 32768, blocks * 64).astype(np.int16)
        if kind == "sparse":   # mostly small values, as a real file has
            coef = (coef // 4096).astype(np.int16) * (rng.random(blocks * 64) < 0.2)
            coef = coef.astype(np.int16)
        coef[:4] = (-32768, 32767, -32768, 32767)
        want = np.zeros((h, w, 3), np.uint8)
        rc = r.lib.rtp_internal_jpeg_reconstruct_host(w, h, nc, hvc, qn.ctypes.data_as(C.c_void_p), rgb, coef.ctypes.data_as(C.c_void_p),
                                                      want.ctypes.data_as(C.c_void_p), C.c_size_t(want.size))
        assert rc == 0, jc.codec_error()
        out = torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        v = _view_struct(frame_view(out))
        rc = r.lib.rtp_internal_jpeg_reconstruct_device(engine.h, w, h, nc, hvc, qn.ctypes.data_as(C.c_void_p), rgb, coef.ctypes.data_as(C.c_void_p), C.byref(v), None)
        assert rc == 0, r.lib.rtp_last_error(engine.h).decode()
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (name, kind, int((got != want).any(-1).sum()))


def test_destination_layouts(engine, decoded):
    import test_device_frames as tdf
    torch = _torch()
    data = dict(jc.grid())["noise_33x31_q75"]
    want = decoded(data)
    # and a 4:4:0 file and an RGB-model one (no colour conversion: the channel order is the kernel's own) against libjpeg's pixels
    for data_, want_ in ((data, want), jc.layout("l440_37x29"), jc.layout("ladobe0_rgb")):
        for layout in ("bgr", "rgb", "bgra", "chw", "crop", "crop_odd"):
            t, order = tdf._to_device(np.zeros_like(want_), layout, fill=77)
            out, path, _ = _decode(engine, data_, out=t, order=order)
            assert path == jc.DEVICE
            assert np.array_equal(tdf._to_host_bgr(t, layout), want_), layout
            if layout == "bgra":
                assert (t[..., 3] == 77).all(), "the 4th channel was written"
    # a window of a larger allocation: nothing outside the window changes
    big = torch.full((31 + 10, 33 + 23, 3), 5, dtype=torch.uint8, device="cuda")
    win = big[4:4 + 31, 9:9 + 33]
    _decode(engine, data, out=win)
    host = big.cpu().numpy()
    assert np.array_equal(host[4:35, 9:42], want)
    host[4:35, 9:42] = 5
    assert (host == 5).all()
    # an aligned packed image takes the 16-byte store kernel: width a multiple of 16, and one that is not
    import caffe_rtpose_amd as r
    for w in (64, 72):
        d2 = r.encode_jpeg(jc.content("noise", w, 24), 90)
        out, path = engine.decode_jpeg_device(d2)
        assert path == jc.DEVICE and np.array_equal(out.cpu().numpy(), decoded(d2)), w


def test_sampling_shapes(engine, decoded):
    """4:4:4, 4:2:2, 4:2:0, grey; chroma planes of at most 2 columns (replication instead of fancy up-sampling); odd sizes whose last MCU
    is mostly padding"""
    cases = {n: jc.fixture(n) for n in ("j444_q90", "j422_q85", "j420_q75", "jgray_q88", "j422_w3", "j420_tiny", "jproggray_q85", "jprog422_q92")}
    g = dict(jc.grid())
    for n in ("noise_1x1_q75", "noise_17x17_q100", "checker_33x31_q25", "noise_65x9_q75"):
        cases[n] = g[n]
    import caffe_rtpose_amd as r
    for w in (2, 3, 4):   # 4:2:0 with 1 or 2 chroma columns
        cases[f"w{w}"] = r.encode_jpeg(jc.content("noise", w, 9), 90)
    assert decoded(cases["j422_w3"]).shape[1] == 3
    for name, data in cases.items():
        out, path = engine.decode_jpeg_device(data)
        assert path == (jc.HOST if name.startswith("jprog") else jc.DEVICE), name
        assert np.array_equal(out.cpu().numpy(), decoded(data)), name


def _collect(e):
    t, n, j, img = e.collect_rendered()
    return t, n, j, img


def test_submitted_jpeg_frames_equal_bgr_frames(decoded):
    """a display-size file, a smaller one that needs the warp and a progressive one, interleaved with BGR and YUV frames in batches of two"""
    import caffe_rtpose_amd as r
    e = _engine(batch_frames=2, frames_in_flight=4)
    try:
        big = r.encode_jpeg(r.synth_frame(DISP_W, DISP_H, 3, seed=41), 90)
        small = r.encode_jpeg(r.synth_frame(301, 173, 4, seed=41), 75)
        prog = jc.fixture("jprog420_q75")
        bgr = r.synth_frame(DISP_W, DISP_H, 5, seed=41)
        planes = yc.from_bgr(r.synth_frame(DISP_W, DISP_H, 6, seed=41))
        seq = [("jpeg", big), ("bgr", bgr), ("yuv", planes), ("jpeg", small), ("jpeg", prog), ("jpeg", big), ("bgr", bgr), ("jpeg", small)]

        def run(as_jpeg):
            out = []
            for i, (kind, x) in enumerate(seq):
                if kind == "bgr":
                    fs = e.submit_frame(x, tag=i)
                elif kind == "yuv":
                    fs = e.submit_frame_yuv(*x, tag=i) if as_jpeg else e.submit_frame(r.convert_yuv(*x), tag=i)
                else:
                    fs = e.submit_frame_jpeg(x, tag=i) if as_jpeg else e.submit_frame(decoded(x), tag=i)
                out.append([fs])
                while e.in_flight() >= 4:
                    t, n, j, img = _collect(e)
                    out[t] += [n, j, img]
            while e.in_flight():
                t, n, j, img = _collect(e)
                out[t] += [n, j, img]
            return out
        want, got = run(False), run(True)
        for i, (a, b) in enumerate(zip(want, got)):
            assert a[0] == b[0], (i, "frame_scale")
            assert a[1] == b[1] and np.array_equal(a[2], b[2]), (i, "joints")
            assert np.array_equal(a[3], b[3]), (i, "rendered frame", int((a[3] != b[3]).any(-1).sum()))
        assert sum(a[1] for a in want) > 0, "the test frames produced no people: nothing was drawn"
    finally:
        e.close()


def test_submitted_layout_files_equal_frames_of_libjpegs_pixels(engine):
    """a 4:4:0 file and an Adobe transform-0 (RGB) one through rtp_submit_frame_jpeg against rtp_submit_frame of the committed pixels"""
    e = engine
    assert e.in_flight() == 0
    for i, name in enumerate(("l440_37x29", "ladobe0_rgb")):
        data, pixels = jc.layout(name)
        fs_want = e.submit_frame(pixels, tag=20 + i)
        want = _collect(e)
        fs_got = e.submit_frame_jpeg(data, tag=20 + i)
        got = _collect(e)
        assert fs_got == fs_want, (name, "frame_scale")
        assert got[0] == want[0] == 20 + i, (name, "tag")
        assert got[1] == want[1] and np.array_equal(got[2], want[2]), (name, "joints")
        assert np.array_equal(got[3], want[3]), (name, "rendered frame", int((got[3] != want[3]).any(-1).sum()))


def _corrupt(data):
    """the file with one scan byte changed so that the host decoder meets a code its tables do not have"""
    start = jc.scan_start(data)
    for pos in range(start + 8, len(data) - 2, 7):
        d = bytearray(data)
        d[pos] = 0xFE if d[pos] != 0xFE else 0xFD
        rc, msg = jc.host_decode(bytes(d))
        if rc and "corrupt" in msg:
            return bytes(d), rc, msg
    raise AssertionError("no corrupting byte found")


def test_corrupted_scan_is_an_error_of_the_frame_not_of_the_engine(engine, decoded):
    """an error path of defined behaviour: the status word carries the host decoder's failure, the engine goes on"""
    import caffe_rtpose_amd as r
    e = engine
    good = dict(jc.grid())["noise_301x173_q75"]
    bad, hrc, hmsg = _corrupt(good)
    assert hrc == r.RTP_EIO
    with pytest.raises(r.RtpError) as ei:
        e.decode_jpeg_device(bad)
    assert ei.value.code == hrc and hmsg in str(ei.value), str(ei.value)
    out, path = e.decode_jpeg_device(good)
    assert path == jc.DEVICE and np.array_equal(out.cpu().numpy(), decoded(good))
    # header errors are the submit's own
    with pytest.raises(r.RtpError) as ei:
        e.submit_frame_jpeg(good[: good.index(b"\xff\xc0") + 7], tag=1)
    assert ei.value.code == r.RTP_EIO and e.in_flight() == 0
    fs0 = e.submit_frame(decoded(good), tag=10)
    want = e.collect_rendered()
    e.submit_frame_jpeg(bad, tag=11)
    fs2 = e.submit_frame_jpeg(good, tag=12)
    with pytest.raises(r.RtpError) as ei:
        e.collect_rendered()
    assert ei.value.code == r.RTP_EIO and "corrupt" in str(ei.value) and "11" in str(ei.value), str(ei.value)
    t, n, j, img = e.collect_rendered()
    assert (t, fs2) == (12, fs0) and n == want[1] and np.array_equal(j, want[2]) and np.array_equal(img, want[3])
    assert e.in_flight() == 0
    fs3 = e.submit_frame_jpeg(good, tag=13)
    t, n, j, img = e.collect_rendered()
    assert (t, fs3) == (13, fs0) and n == want[1] and np.array_equal(j, want[2]) and np.array_equal(img, want[3])


def test_cli_same_files_whichever_decoder(tmp_path):
    """--image_dir with small JPEG files (one of them with a corrupt scan) and --video with a 3-frame MJPEG stream: the same JSON files
    with --gpu_decode, with --host_decode and with neither (--video decodes on the GPU by default, --image_dir on the producer pool);
    the corrupt file is skipped by both decoders"""
    import shutil
    d = tmp_path / "imgs"
    d.mkdir()
    names = ["j420_q75", "j444_q90", "jprog422_q92"]
    for n in names:
        shutil.copy(os.path.join(jc.GOLD, n + ".jpg"), d / (n + ".jpg"))
    bad, _, _ = _corrupt(jc.fixture("j422_q85"))
    (d / "j422_bad.jpg").write_bytes(bad)
    clip = tmp_path / "clip.mjpeg"
    clip.write_bytes(jc.fixture("j420_q75") + jc.fixture("j422_q85") + jc.fixture("j444_q90"))   # (one size: a stream's frames may not change it)
    common = ["--model", "coco", "--net_resolution", "160x96", "--resolution", "320x240", "--no_frame_drops", "--no_display", "--num_gpu", "1"]
    outs = {}
    for src, key in ((["--image_dir", str(d)], "dir"), (["--video", str(clip)], "clip")):
        for flag in ("--gpu_decode", "--host_decode", ""):
            out = tmp_path / f"js_{key}_{flag.strip('-') or 'default'}"
            p = subprocess.run([BIN] + src + ["--write_json", str(out)] + common + ([flag] if flag else []), capture_output=True)
            assert p.returncode == 0, p.stderr.decode()
            outs[key, flag] = {f: open(out / f, "rb").read() for f in sorted(os.listdir(out))}
            if key == "dir":
                assert b"corrupt" in p.stderr, (flag, p.stderr.decode()[-500:])
    assert sorted(outs["dir", "--gpu_decode"]) == sorted(n + ".json" for n in names)
    assert sorted(outs["clip", "--gpu_decode"]) == [f"frame{i:06d}.json" for i in range(3)]
    for key in ("dir", "clip"):
        assert outs[key, "--gpu_decode"] == outs[key, "--host_decode"] == outs[key, ""], key

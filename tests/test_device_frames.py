"""Frames in GPU memory: rtp_submit_frame_device / rtp_collect_rendered_device against rtp_submit_frame / rtp_collect_rendered of the
same pixels as a host BGR array.  Joints, num_people and frame_scale must be bit-identical and rendered frames byte-identical (the device
path runs the same per-pixel arithmetic); ordering against the caller's stream is checked with a stream kept busy on purpose."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NET_W, NET_H = 320, 176
DISP_W, DISP_H = 1280, 720
LAYOUTS = ("bgr", "rgb", "bgra", "rgba", "chw", "crop", "crop_odd")


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


def _to_device(img, layout, fill=0):
    """The BGR host image `img` as a device tensor of `layout`; returns (tensor or view, order)."""
    torch = _torch()
    h, w, _ = img.shape
    rgb = np.ascontiguousarray(img[..., ::-1])
    alpha = np.full((h, w, 1), 77 if fill == 0 else fill, np.uint8)
    if layout == "bgr":
        return torch.from_numpy(img.copy()).cuda(), "bgr"
    if layout == "rgb":
        return torch.from_numpy(rgb).cuda(), "rgb"
    if layout == "bgra":
        return torch.from_numpy(np.concatenate([img, alpha], -1)).cuda(), "bgr"
    if layout == "rgba":
        return torch.from_numpy(np.concatenate([rgb, alpha], -1)).cuda(), "rgb"
    if layout == "chw":
        return torch.from_numpy(rgb).cuda().permute(2, 0, 1).contiguous(), "rgb"
    if layout in ("crop", "crop_odd"):   # a window of a larger tensor: aligned pitch (dword path) / odd pitch and start (byte gather)
        dx, dy, extra = (16, 8, 64) if layout == "crop" else (7, 11, 71)
        big = torch.full((h + 2 * dy, w + extra, 3), 5, dtype=torch.uint8, device="cuda")
        big[dy:dy + h, dx:dx + w] = torch.from_numpy(img).cuda()
        return big[dy:dy + h, dx:dx + w], "bgr"
    raise ValueError(layout)


def _to_host_bgr(t, layout):
    a = t.cpu().numpy()
    if layout == "chw":
        a = a.transpose(1, 2, 0)
    a = a[..., :3]
    return np.ascontiguousarray(a[..., ::-1] if layout in ("rgb", "rgba", "chw") else a)


def _host_result(e, img, tag):
    fs = e.submit_frame(img, tag=tag)
    t, n, j, rendered = e.collect_rendered()
    assert t == tag
    return fs, n, j, rendered


def _device_result(e, img, in_layout, out_layout, tag):
    torch = _torch()
    frame, order = _to_device(img, in_layout)
    torch.cuda.synchronize()
    fs = e.submit_frame_device(frame, tag=tag, order=order)
    ref = _to_device(np.zeros((DISP_H, DISP_W, 3), np.uint8), out_layout, fill=201)
    out, oorder = ref
    t, n, j = e.collect_rendered_device(out, order=oorder)
    assert t == tag
    if out_layout in ("bgra", "rgba"):
        assert bool((out[..., 3] == 201).all()), "the 4th channel of the output was written"
    return fs, n, j, _to_host_bgr(out, out_layout)


def _assert_same(a, b, what):
    assert a[0] == b[0], f"{what}: frame_scale {a[0]} != {b[0]}"
    assert a[1] == b[1], f"{what}: num_people {a[1]} != {b[1]}"
    assert np.array_equal(a[2], b[2]), f"{what}: joints differ"
    assert np.array_equal(a[3], b[3]), f"{what}: rendered frames differ in {int((a[3] != b[3]).any(-1).sum())} pixels"


@pytest.fixture(scope="module")
def render_engine():
    e = _engine(render=1)
    yield e
    e.close()


@pytest.mark.parametrize("size", [(1280, 720), (640, 480), (1920, 1080)], ids=["import", "warp_up", "warp_down"])
def test_device_frames_equal_host_frames(render_engine, size):
    import caffe_rtpose_amd as r
    e = render_engine
    w, h = size
    people = 0
    for i, layout in enumerate(LAYOUTS):
        img = r.synth_frame(w, h, i, seed=41)
        want = _host_result(e, img, 2 * i)
        got = _device_result(e, img, layout, LAYOUTS[(i + 3) % len(LAYOUTS)], 2 * i + 1)
        _assert_same(got, want, f"{w}x{h} in {layout} out {LAYOUTS[(i + 3) % len(LAYOUTS)]}")
        people += want[1]
    assert people > 0, "the test frames produced no people: nothing was drawn"


@pytest.mark.parametrize("kw", [dict(render=1 + 3), dict(render=1, num_scales=3, scale_gap=0.25), dict(render=1, model=1)],
                         ids=["heatmap_view", "three_scales", "mpi"])
def test_device_frames_other_configurations(kw):
    import caffe_rtpose_amd as r
    e = _engine(**kw)
    for i, (size, lin, lout) in enumerate((((1280, 720), "bgra", "rgb"), ((640, 480), "chw", "bgr"), ((1920, 1080), "crop_odd", "chw"))):
        img = r.synth_frame(size[0], size[1], i, seed=43)
        _assert_same(_device_result(e, img, lin, lout, 2 * i + 1), _host_result(e, img, 2 * i), f"{kw} {size}")
    e.close()


def _interleaved_digest(exec_mode):
    """batch_frames 2 / frames_in_flight 7 (bench.py's engine shape), 11 frames: host-only run, then every other frame from device
    memory in one of the layouts.  FIFO order and results must match; returns a digest of the run."""
    import caffe_rtpose_amd as r
    torch = _torch()
    e = _engine(batch_frames=2, frames_in_flight=7, exec_mode=exec_mode)
    sizes = [(1280, 720), (640, 480), (1920, 1080)]
    imgs = [r.synth_frame(*sizes[i % 3], i, seed=47) for i in range(11)]
    frames = [_to_device(im, LAYOUTS[i % len(LAYOUTS)]) for i, im in enumerate(imgs)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()

    def run(mixed):
        out, scales = [], []
        for i, im in enumerate(imgs):
            if mixed and i % 2:
                scales.append(e.submit_frame_device(frames[i][0], tag=100 + i, stream=side, order=frames[i][1]))
            else:
                scales.append(e.submit_frame(im, tag=100 + i))
            while e.in_flight() >= 7:
                out.append(e.collect())
        while e.in_flight():
            out.append(e.collect())
        return out, scales

    host, hs = run(False)
    mixed, ms = run(True)
    e.close()
    assert [t for t, _, _ in mixed] == [100 + i for i in range(11)]
    assert hs == ms
    for (ta, na, ja), (tb, nb, jb) in zip(host, mixed):
        assert ta == tb and na == nb and np.array_equal(ja, jb), ta
    assert sum(n for _, n, _ in host) > 0
    h = hashlib.sha256()
    for t, n, j in mixed:
        h.update(np.int64([t, n]).tobytes() + j.tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_interleaved_host_and_device_frames(mode):
    import caffe_rtpose_amd as r
    _interleaved_digest(r.EXEC_GRAPH if mode == "graph" else r.EXEC_EAGER)


def test_interleaved_with_deferred_preprocessing():
    """The experiments build's RTP_PREP_DEFER=1 (host frames' kernels wait for their copy): device frames have no copy to wait for and
    mix in unchanged."""
    import caffe_rtpose_amd as r
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = os.path.join(root, "caffe_rtpose_amd", "librtpose_mi355x_exp.so")
    want = _interleaved_digest(r.EXEC_GRAPH)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTP_")}
    env.update(RTP_LIB=exp, RTP_PREP_DEFER="1")
    code = ("import sys; sys.path[:0] = [%r, %r]; import torch; import caffe_rtpose_amd as r; import test_device_frames as t; "
            "print('digest', t._interleaved_digest(r.EXEC_GRAPH))") % (root, os.path.join(root, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert [l for l in out.stdout.splitlines() if l.startswith("digest")][-1].split()[1] == want


def test_submit_is_ordered_on_the_callers_stream(render_engine):
    """The frame is written on a busy side stream and zeroed right after the submit on the same stream, without a host wait: the
    engine reads it after the write and before the zeroing."""
    import caffe_rtpose_amd as r
    torch = _torch()
    e = render_engine
    img = r.synth_frame(1920, 1080, 3, seed=53)
    want = _host_result(e, img, 1)
    src = torch.from_numpy(img).cuda()
    frame = torch.empty_like(src)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(50_000_000)
        frame.copy_(src)
        fs = e.submit_frame_device(frame, tag=2, stream=s)
        frame.zero_()
    out = torch.zeros((DISP_H, DISP_W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t, n, j = e.collect_rendered_device(out)
    assert t == 2
    _assert_same((fs, n, j, out.cpu().numpy()), want, "stream-ordered submit")
    assert bool((frame == 0).all())


def test_collect_is_ordered_on_the_callers_stream(render_engine):
    import caffe_rtpose_amd as r
    torch = _torch()
    e = render_engine
    img = r.synth_frame(1280, 720, 4, seed=59)
    want = _host_result(e, img, 1)
    for layout in ("bgr", "bgra"):
        ch = 4 if layout == "bgra" else 3
        out = torch.full((DISP_H, DISP_W, ch), 231, dtype=torch.uint8, device="cuda")
        e.submit_frame(img, tag=2)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            torch.cuda._sleep(50_000_000)
            t, n, j = e.collect_rendered_device(out, stream=s)
            snap = out.clone()
        s.synchronize()
        assert t == 2 and n == want[1] and np.array_equal(j, want[2])
        a = snap.cpu().numpy()
        assert np.array_equal(a[..., :3], want[3]), layout
        if ch == 4:
            assert (a[..., 3] == 231).all()


class _Fake:
    def __init__(self, ptr, shape, strides):
        self.__cuda_array_interface__ = dict(typestr="|u1", shape=shape, strides=strides, data=(ptr, False), version=2)


def _still_usable(e, tag):
    import caffe_rtpose_amd as r
    torch = _torch()
    img = r.synth_frame(640, 480, 1, seed=61)
    frame = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    e.submit_frame_device(frame, tag=tag)
    got = e.collect()
    assert got[0] == tag


def test_refusals_leave_the_engine_usable(render_engine):
    import caffe_rtpose_amd as r
    torch = _torch()
    e = render_engine
    img = r.synth_frame(640, 480, 0, seed=67)

    def refused(call, *words):
        with pytest.raises(r.RtpError) as ex:
            call()
        assert ex.value.code == r.RTP_EINVAL, ex.value
        for w in words:
            assert w in str(ex.value), ex.value

    # host memory: refused by the Python layer (no device interface) and, behind a forged interface, by the library's pointer check
    with pytest.raises(TypeError):
        e.submit_frame_device(img)
    pinned = torch.from_numpy(img).pin_memory()
    with pytest.raises(TypeError):
        e.submit_frame_device(pinned)
    refused(lambda: e.submit_frame_device(_Fake(pinned.data_ptr(), (480, 640, 3), None), stream=0), "host")
    refused(lambda: e.submit_frame_device(_Fake(img.ctypes.data, (480, 640, 3), None), stream=0), "import torch BEFORE")
    _still_usable(e, 10)
    # rows that run past the allocation
    dev = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    refused(lambda: e.submit_frame_device(_Fake(dev.data_ptr(), (480, 640, 3), (1 << 26, 3, 1)), stream=0), "allocation")
    _still_usable(e, 11)
    # wrong output size: nothing is collected, the frame stays first in line
    e.submit_frame_device(dev, tag=12)
    small = torch.zeros((480, 640, 3), dtype=torch.uint8, device="cuda")
    refused(lambda: e.collect_rendered_device(small), "640 x 480")
    assert e.in_flight() == 1
    out = torch.zeros((DISP_H, DISP_W, 3), dtype=torch.uint8, device="cuda")
    assert e.collect_rendered_device(out)[0] == 12
    _still_usable(e, 13)
    # a capturing stream (the capture is opened and closed, never replayed)
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    with torch.cuda.graph(g):
        x.add_(1)
        refused(lambda: e.submit_frame_device(dev, tag=14, stream=torch.cuda.current_stream()), "capturing")
    del g
    _still_usable(e, 15)
    # render == 0
    e0 = _engine(render=0)
    e0.submit_frame_device(dev, tag=16)
    refused(lambda: e0.collect_rendered_device(out), "render")
    assert e0.collect()[0] == 16
    _still_usable(e0, 17)
    e0.close()


def test_refuses_another_devices_memory(render_engine):
    torch = _torch()
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    import caffe_rtpose_amd as r
    e = render_engine
    other = torch.zeros((480, 640, 3), dtype=torch.uint8, device="cuda:1")
    torch.cuda.synchronize(1)
    with pytest.raises(r.RtpError) as ex:
        e.submit_frame_device(other, stream=0)
    assert ex.value.code == r.RTP_EINVAL and "device 1" in str(ex.value)
    _still_usable(e, 20)


def test_stamp_probe_accounts_for_import_and_export():
    """Device frames stamp the pre-processing slots of host frames (200 + 2 j: import / warp, + 1: area / pad), the export of the
    rendered image slot 64 + 8 j + 5."""
    import caffe_rtpose_amd as r
    torch = _torch()
    e = _engine(render=1, exec_mode=r.EXEC_EAGER)
    e.stamp_probe(1)
    img = r.synth_frame(1280, 720, 0, seed=71)
    frame = torch.from_numpy(img).cuda()
    out = torch.zeros((DISP_H, DISP_W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for i in range(3):
        e.submit_frame_device(frame, tag=i)
        e.collect_rendered_device(out)
    spans = e.stamp_probe(-1)
    slots = set(int(s) for s in spans[:, 0])
    assert {200, 201, 69} <= slots, sorted(slots)
    e.stamp_probe(0)
    e.close()

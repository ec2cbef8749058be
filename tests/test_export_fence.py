"""A frame slot's next frame must not overwrite what a caller's stream is still reading.  Every device export (rtp_collect_rendered_device,
rtp_collect_rendered_yuv_device, rtp_peek_maps_device, rtp_peek_crops_device) is enqueued on a side stream that is held busy, and the
next frame is submitted and finished at once on the ONE context and slot the engine has: the export must still deliver the first frame."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NET_W, NET_H = 160, 96
DISP_W, DISP_H = 320, 180
GUARD = 0x5A
HOLD = 50_000_000   # cycles the side stream sleeps in front of the export (test_device_frames.py holds its streams the same way)


def _torch():
    import torch   # (tests/conftest.py imported it before the engine library: one HIP runtime for both)
    return torch


def _engine(**kw):
    import caffe_rtpose_amd as r
    e = r.Engine(r.Config(net_w=NET_W, net_h=NET_H, num_scales=1, disp_w=DISP_W, disp_h=DISP_H, frames_in_flight=1, batch_frames=1, **kw))
    t = e.get_thresholds()
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], 2, 0.05)   # keep more "people" of the noise maps
    return e


@pytest.fixture(scope="module")
def render_engine():
    e = _engine(render=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def plain_engine():
    e = _engine()
    yield e
    e.close()


def _frames(size, seed):
    import caffe_rtpose_amd as r
    return r.synth_frame(*size, 0, seed=seed), r.synth_frame(*size, 1, seed=seed + 1)


def _host(e, frame, tag, take):
    e.submit_frame(frame, tag=tag)
    return take()


def _held_export_then_next_frame(e, a, b, export_a, finish_b):
    """A's export on a held side stream, then B through the same slot with no host wait in between"""
    torch = _torch()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    e.submit_frame(a, tag=1)
    with torch.cuda.stream(side):
        torch.cuda._sleep(HOLD)
        export_a(side)
    e.submit_frame(b, tag=2)
    finish_b()
    side.synchronize()
    assert e.in_flight() == 0


def test_collect_rendered_device(render_engine):
    torch = _torch()
    e = render_engine
    a, b = _frames((640, 360), 81)
    want_a = _host(e, a, 1, e.collect_rendered)[3]
    want_b = _host(e, b, 2, e.collect_rendered)[3]
    assert not np.array_equal(want_a, want_b)
    out = torch.full((DISP_H, DISP_W, 3), GUARD, dtype=torch.uint8, device="cuda")
    out_b = torch.zeros_like(out)
    _held_export_then_next_frame(e, a, b, lambda s: e.collect_rendered_device(out, stream=s), lambda: e.collect_rendered_device(out_b, stream=0))
    got = out.cpu().numpy()
    assert np.array_equal(out_b.cpu().numpy(), want_b)
    assert not np.array_equal(got, want_b), "the held export delivered the NEXT frame's image"
    assert np.array_equal(got, want_a), f"the held export differs from its frame in {int((got != want_a).any(-1).sum())} pixels"


def test_collect_rendered_yuv_device(render_engine):
    torch = _torch()
    e = render_engine
    a, b = _frames((640, 360), 83)
    e.set_render_yuv(420)
    try:
        want_a = _host(e, a, 1, e.collect_rendered_yuv)[2:]
        want_b = _host(e, b, 2, e.collect_rendered_yuv)[2:]
        assert not np.array_equal(want_a[0], want_b[0])
        planes = [torch.full(p.shape, GUARD, dtype=torch.uint8, device="cuda") for p in want_a]
        planes_b = [torch.zeros_like(p) for p in planes]
        _held_export_then_next_frame(e, a, b, lambda s: e.collect_rendered_yuv_device(*planes, stream=s),
                                     lambda: e.collect_rendered_yuv_device(*planes_b, stream=0))
    finally:
        e.set_render_yuv(0)
    got = [p.cpu().numpy() for p in planes]
    assert all(np.array_equal(p.cpu().numpy(), w) for p, w in zip(planes_b, want_b))
    assert not np.array_equal(got[0], want_b[0]), "the held export delivered the NEXT frame's planes"
    for name, g, w in zip("yuv", got, want_a):
        assert np.array_equal(g, w), f"plane {name} of the held export differs from its frame in {int((g != w).sum())} samples"


def test_peek_maps_device(plain_engine):
    """grid lowres, f32: the next batch's conv stack is what overwrites the maps being read"""
    torch = _torch()
    e = plain_engine
    a, b = _frames((640, 360), 85)
    e.set_maps_output("lowres", "f32")
    try:
        shape, dt, _ = e.maps_info()
        assert dt == np.float32

        def host_maps():
            m = e.peek_maps()[1].copy()
            e.collect()
            return m
        want_a, want_b = _host(e, a, 1, host_maps), _host(e, b, 2, host_maps)
        assert not np.array_equal(want_a, want_b)
        out = torch.full(shape, -7.0, dtype=torch.float32, device="cuda")
        out_b = torch.zeros_like(out)

        def export_a(s):
            assert e.peek_maps_device(out, stream=s) == 1
            assert e.collect()[0] == 1

        def finish_b():
            assert e.peek_maps_device(out_b, stream=0) == 2
            assert e.collect()[0] == 2
        _held_export_then_next_frame(e, a, b, export_a, finish_b)
    finally:
        e.set_maps_output(None)
    got = out.cpu().numpy()
    assert np.array_equal(out_b.cpu().numpy(), want_b)
    assert not np.array_equal(got, want_b), "the held peek delivered the NEXT frame's maps"
    assert np.array_equal(got, want_a), f"the held peek differs from its frame in {int((got != want_a).sum())} values"


@pytest.mark.parametrize("size", [(640, 360), (DISP_W, DISP_H)], ids=["warped_display_image", "staged_frame_is_the_display_image"])
def test_peek_crops_device(plain_engine, size):
    """640x360: the crops are read from the warped display image.  320x180: disp_cur is the staged frame itself, and the writer is the
    next submit's H2D copy on the staging / copy stream."""
    torch = _torch()
    e = plain_engine
    a, b = _frames(size, 87)
    M = 8
    e.set_crops_output(64, 64, M, margin=0.15)
    try:
        def host_crops():
            _, boxes, crops = e.peek_crops()
            e.collect()
            return boxes, crops
        (boxes_a, want_a), (boxes_b, want_b) = _host(e, a, 1, host_crops), _host(e, b, 2, host_crops)
        n = len(boxes_a)
        assert n >= 1 and boxes_a[:, 5].sum() >= 1, "frame A needs a valid box"
        assert want_a.tobytes() != want_b.tobytes()
        out = torch.full((M, 64, 64, 3), GUARD, dtype=torch.uint8, device="cuda")
        out_b = torch.zeros_like(out)

        def export_a(s):
            t, bx = e.peek_crops_device(out, stream=s)
            assert t == 1 and bx.tobytes() == boxes_a.tobytes()
            assert e.collect()[0] == 1

        def finish_b():
            t, bx = e.peek_crops_device(out_b, stream=0)
            assert t == 2 and bx.tobytes() == boxes_b.tobytes()
            assert e.collect()[0] == 2
        _held_export_then_next_frame(e, a, b, export_a, finish_b)
    finally:
        e.set_crops_output(None)
    got = out.cpu().numpy()
    assert np.array_equal(out_b.cpu().numpy()[:len(boxes_b)], want_b)
    assert got[:n].tobytes() != out_b.cpu().numpy()[:n].tobytes(), "the held peek delivered the NEXT frame's crops"
    assert np.array_equal(got[:n], want_a), f"the held peek differs from its frame in crops {np.flatnonzero((got[:n] != want_a).reshape(n, -1).any(1)).tolist()}"
    assert (got[n:] == GUARD).all()

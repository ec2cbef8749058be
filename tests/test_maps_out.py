"""Maps mode on the GPU.  Every comparison is bit for bit (a NaN only has to be a NaN): the tap against _oracle.imresize and against
Engine.resize in three scale geometries and two orientations, the narrow formats against numpy, channel lists, the async path
against the low-res blobs its own batches read, the renderer modes, the device entry with guards on both store paths, every
refusal, and rtpose.bin --write_heatmaps against peek_maps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _mapscases as mc
import _oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
NET_W, NET_H, DISP_W, DISP_H = mc.NET_W, mc.NET_H, mc.DISP_W, mc.DISP_H
GUARD = 0x5A
LOWRES_BLOB = "concat_stage7"


def _torch():
    import torch   # (tests/conftest.py imported it before the engine library: one HIP runtime for both)
    return torch


def _engine(**kw):
    import caffe_rtpose_amd as r
    kw = dict(dict(net_w=NET_W, net_h=NET_H, disp_w=DISP_W, disp_h=DISP_H, frames_in_flight=4, batch_frames=2), **kw)
    return r.Engine(r.Config(**kw))


_tap_engines, _tap_refs = {}, {}


def _tap_engine(portrait, geo):
    """one small engine per (orientation, scale geometry), shared by the tap tests"""
    key = (portrait, geo)
    if key not in _tap_engines:
        n, start, gap = mc.GEOMETRIES[geo]
        w, h = (NET_H, NET_W) if portrait else (NET_W, NET_H)
        _tap_engines[key] = _engine(net_w=w, net_h=h, num_scales=n, start_scale=start, scale_gap=gap, frames_in_flight=1, batch_frames=1)
    return _tap_engines[key]


def _tap_ref(portrait, geo):
    """(planted low-res maps, the oracle's resized map [C][net_h][net_w]) of the case, computed once"""
    key = (portrait, geo)
    if key not in _tap_refs:
        e = _tap_engine(portrait, geo)
        n, start, gap = mc.GEOMETRIES[geo]
        low = mc.planted_lowres(e.N, e.heat_channels, e.low_h, e.low_w, e.num_parts)
        _tap_refs[key] = (low, orc.imresize(low, e.net_w, e.net_h, start, gap)[0])
    return _tap_refs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _tap_engines.values():
        e.close()
    _tap_engines.clear()


@pytest.mark.parametrize("geo", list(mc.GEOMETRIES))
@pytest.mark.parametrize("portrait", [False, True], ids=["160x96", "96x160"])
def test_tap_against_the_oracle(portrait, geo):
    e = _tap_engine(portrait, geo)
    low, want = _tap_ref(portrait, geo)
    allc = list(range(e.heat_channels))
    assert np.isnan(want).any() and (want > 1).any() and (want < -1).any(), "the planted maps must reach the clamps and hold a NaN"
    try:
        e.set_maps_output("net", "f32")
        shape, dt, nb = e.maps_info()
        assert shape == (1, e.heat_channels, e.net_h, e.net_w) and dt == np.float32 and nb == want.nbytes
        got = e.maps_from_lowres(low)[0]
        assert mc.same_f32(got, want), f"f32 vs the oracle: {int((got != want).sum())} values differ"
        assert mc.same_f32(got, e.resize(low)), "f32 vs Engine.resize"
        e.set_maps_output("net", "f16")
        got = e.maps_from_lowres(low)[0]
        assert got.dtype == np.float16 and mc.same_f16(got, mc.f16_ref(want)), "f16 vs numpy's conversion of the oracle's map"
        e.set_maps_output("net", "u8")
        got = e.maps_from_lowres(low)[0]
        ref = mc.u8_ref_planes(want, allc, e.num_parts)
        assert got.dtype == np.uint8 and np.array_equal(got, ref), f"u8: {int((got != ref).sum())} values differ"
        assert (ref == 0).any() and (ref == 255).any()
        # the low-res grid: the planted maps themselves (exact quantiser ties included), every format
        e.set_maps_output("lowres", "f32")
        assert e.maps_info()[0] == low.shape and mc.same_f32(e.maps_from_lowres(low), low)
        e.set_maps_output("lowres", "f32", allc[::-1])          # (not the natural order: through the kernel, not the plain copy)
        assert mc.same_f32(e.maps_from_lowres(low), low[:, ::-1])
        e.set_maps_output("lowres", "f16")
        assert mc.same_f16(e.maps_from_lowres(low), mc.f16_ref(low))
        e.set_maps_output("lowres", "u8")
        got, ref = e.maps_from_lowres(low), mc.u8_ref_planes(low, allc, e.num_parts)
        assert np.array_equal(got, ref), f"lowres u8: {int((got != ref).sum())} values differ"
    finally:
        e.set_maps_output(None)


@pytest.mark.parametrize("fmt", ["f32", "f16", "u8"])
def test_channel_lists(fmt):
    e = _tap_engine(False, "3")
    low, _ = _tap_ref(False, "3")
    same = {"f32": mc.same_f32, "f16": mc.same_f16, "u8": np.array_equal}[fmt]
    try:
        for grid in ("net", "lowres"):
            e.set_maps_output(grid, fmt)
            full = e.maps_from_lowres(low)
            for name in ("one_paf", "permuted_across_boundary", "repeat"):
                ch = mc.channels_of(name)
                e.set_maps_output(grid, fmt, ch)
                got = e.maps_from_lowres(low)
                assert got.shape == full.shape[:1] + (len(ch),) + full.shape[2:]
                for k, c in enumerate(ch):
                    assert same(got[:, k], full[:, c]), f"{grid} {fmt} {name}: plane {k} is not channel {c}"
    finally:
        e.set_maps_output(None)


def _frames(n=4, seed=31):
    import caffe_rtpose_amd as r
    sizes = [(DISP_W, DISP_H), (640, 360)]   # at the display size, and through the warp
    return [r.synth_frame(*sizes[i % 2], i, seed=seed) for i in range(n)]


def _run(e, frames, peek=None, collect=None):
    """submit all, then per frame: peek (if given), collect -> [(peeked, collected)]"""
    for i, f in enumerate(frames):
        e.submit_frame(f, tag=50 + i)
    out = []
    while e.in_flight():
        p = peek() if peek else None
        out.append((p, (collect or e.collect)()))
    return out


def _lowres_by_tag(e):
    """every context's last batch: tag -> that frame's own low-res maps [N][C][h][w]"""
    import caffe_rtpose_amd as r
    by_tag = {}
    for ci in range(64):
        try:
            blob, tags = e.get_batch_blob(ci, LOWRES_BLOB)
        except r.RtpError:
            break
        for j, t in enumerate(tags):
            by_tag[t] = blob[j * e.N:(j + 1) * e.N]
    return by_tag


def test_async_path_maps_are_each_frames_own():
    e = _engine(num_scales=2, start_scale=1.0, scale_gap=0.3)
    frames = _frames(4)
    try:
        off = _run(e, frames)
        e.set_maps_output("net", "f32")

        def peek_twice():
            t1, m1 = e.peek_maps()
            t2, m2 = e.peek_maps()
            assert t1 == t2 and m1.tobytes() == m2.tobytes(), "peeking twice gives the same maps"
            return t1, m1
        on = _run(e, frames, peek_twice)
        low = _lowres_by_tag(e)
        assert sorted(low) == [50, 51, 52, 53], "two contexts of two frames each hold the four frames"
        assert len({l.tobytes() for l in low.values()}) == 4, "the four frames must differ"
        for i, ((ptag, maps), (ctag, n, joints)) in enumerate(on):
            assert ptag == ctag == 50 + i
            want = orc.imresize(low[ctag], NET_W, NET_H, 1.0, 0.3)
            assert mc.same_f32(maps, want), f"frame {i}: the maps are not ImResize of this frame's own low-res maps"
            assert n == off[i][1][1] and np.array_equal(joints, off[i][1][2]), f"frame {i}: joints differ with maps on"
        # the low-res grid: the blob itself (the plain copy), and through the kernel as f16
        e.set_maps_output("lowres", "f32")
        for (ptag, maps), (ctag, _, _) in _run(e, frames, e.peek_maps):
            assert ptag == ctag and mc.same_f32(maps, _lowres_by_tag(e)[ctag])
        e.set_maps_output("lowres", "f16", [20, 0, 18])
        for (ptag, maps), (ctag, _, _) in _run(e, frames, e.peek_maps):
            assert mc.same_f16(maps, mc.f16_ref(_lowres_by_tag(e)[ctag][:, [20, 0, 18]]))
        # thresholds and scales may change while the mode is on; set_scales changes the maps as it changes ImResize
        e.set_scales(1.0, 0.25)
        e.set_maps_output("net", "u8", [0, 18, 19])
        for (ptag, maps), (ctag, _, _) in _run(e, frames[:3], e.peek_maps):   # (a full batch and a partial one)
            want = orc.imresize(_lowres_by_tag(e)[ctag], NET_W, NET_H, 1.0, 0.25)[:, [0, 18, 19]]
            assert np.array_equal(maps, mc.u8_ref_planes(want, [0, 18, 19], e.num_parts))
        # frames submitted as net inputs get maps too
        x = np.random.default_rng(5).uniform(-0.5, 0.5, (e.N, 3, NET_H, NET_W)).astype(np.float32)
        e.submit(x, tag=9)
        ptag, maps = e.peek_maps()
        assert ptag == 9 and e.collect()[0] == 9
        want = orc.imresize(_lowres_by_tag(e)[9], NET_W, NET_H, 1.0, 0.25)[:, [0, 18, 19]]
        assert np.array_equal(maps, mc.u8_ref_planes(want, [0, 18, 19], e.num_parts))
        # off again: the engine is what it was
        e.set_scales(1.0, 0.3)
        e.set_maps_output(None)
        again = _run(e, frames)
        assert all(a[1][1] == b[1][1] and np.array_equal(a[1][2], b[1][2]) for a, b in zip(again, off))
    finally:
        e.close()


@pytest.mark.parametrize("mode", ["raw", "yuv"])
def test_renderer_modes_are_unchanged_by_maps(mode):
    e = _engine(render=1)
    frames = _frames(3, seed=33)
    collect = e.collect_rendered if mode == "raw" else e.collect_rendered_yuv
    try:
        if mode == "yuv":
            e.set_render_yuv(420)
        off = _run(e, frames, None, collect)
        e.set_maps_output("net", "u8")
        on = _run(e, frames, e.peek_maps, collect)
        low = _lowres_by_tag(e)
        for (_, a), ((ptag, maps), b) in zip(off, on):
            assert ptag == a[0] == b[0]
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), "joints or the rendered frame changed with maps on"
            if ptag in low:
                want = orc.imresize(low[ptag], NET_W, NET_H)[0]
                assert np.array_equal(maps[0], mc.u8_ref_planes(want, list(range(e.heat_channels)), e.num_parts))
    finally:
        e.close()


def _layout(e, t):
    """the store path the host would choose for the device array t (the unexported query)"""
    from caffe_rtpose_amd import _lib
    from caffe_rtpose_amd.engine import maps_view
    shape, dt, _ = e.maps_info()
    f = maps_view(t, shape, dt)
    v = _lib.rtp_maps_view()
    v.struct_size = C.sizeof(v)
    v.data, v.channel_stride, v.row_stride = f["data"], f["channel_stride"], f["row_stride"]
    fn = _lib.lib.rtp_internal_maps_export_layout
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(_lib.rtp_maps_view)]
    return fn(e.h, C.byref(v))


def _guarded(torch, tdt, fmt, planes, H, W, dx, extra):
    """a tensor of planes + 2 guard planes, H + 3 rows and W + extra columns, and the planes x H x W window at (1, 2, dx) inside it"""
    big = torch.full((planes + 2, H + 3, W + extra), GUARD if fmt == "u8" else 3.0, dtype=tdt[fmt], device="cuda")
    return big, big[1:1 + planes, 2:2 + H, dx:dx + W]


def _guards_intact(torch, big, guard_value, planes, H, W, dx):
    after = big.clone()
    after[1:1 + planes, 2:2 + H, dx:dx + W] = guard_value
    return bool((after == guard_value).all())


def test_device_entry_both_store_paths():
    torch = _torch()
    e = _engine(num_scales=2)
    frames = _frames(2, seed=35)
    tdt = {"f32": torch.float32, "f16": torch.float16, "u8": torch.uint8}
    try:
        for grid, fmt, ch in (("net", "u8", [3, 19, 18, 40, 3]), ("net", "f16", None), ("net", "f32", [56, 0]), ("lowres", "u8", [1, 30]), ("lowres", "f32", None)):
            e.set_maps_output(grid, fmt, ch)
            (n0, nch, H, W), dt, _ = e.maps_info()
            planes = n0 * nch
            gv = GUARD if fmt == "u8" else 3.0
            view = lambda t: t.reshape(n0, nch, H, W) if t.is_contiguous() else t.unflatten(0, (n0, nch))
            # (a) an odd window: base 3 elements into a row, a pitch of W + 7 elements (u8: an unaligned base and a pitch that is no
            # multiple of 4) -> on the net grid the byte-wise path; (b) an aligned window with pitch padding and (c) an aligned dense
            # tensor -> the wide path
            odd_big, odd = _guarded(torch, tdt, fmt, planes, H, W, 3, 7)
            al_big, al = _guarded(torch, tdt, fmt, planes, H, W, 8, 24)
            dense = torch.zeros((planes, H, W), dtype=tdt[fmt], device="cuda")
            assert (W + 7) % 4 != 0 and odd.data_ptr() % 4 != 0 if fmt == "u8" else True
            if grid == "net":
                assert _layout(e, view(odd)) == 0, "an odd base and pitch must take the byte-wise path"
            assert _layout(e, view(al)) == 1 and _layout(e, view(dense)) == 1, "aligned views must take the wide path"
            side = torch.cuda.Stream()
            torch.cuda.synchronize()
            for f in frames:
                e.submit_frame(f, tag=7)
            # frame 0: the windows on the NULL stream (complete on return), the dense tensor on a caller's stream with a copy behind it
            tag, host = e.peek_maps()
            assert e.peek_maps_device(view(odd), stream=0) == tag == 7
            assert e.peek_maps_device(view(al), stream=0) == 7
            e.peek_maps_device(view(dense), stream=side)
            with torch.cuda.stream(side):
                later = dense.clone()            # enqueued on the caller's stream behind the peek: sees the maps
            side.synchronize()
            assert e.collect()[0] == 7
            same = {"f32": mc.same_f32, "f16": mc.same_f16, "u8": np.array_equal}[fmt]
            assert same(odd.cpu().numpy().reshape(host.shape), host), f"{grid} {fmt}: the odd window differs from the host peek"
            assert same(al.cpu().numpy().reshape(host.shape), host), f"{grid} {fmt}: the aligned window differs from the host peek"
            assert same(later.cpu().numpy().reshape(host.shape), host), f"{grid} {fmt}: the copy behind the peek on the caller's stream"
            assert _guards_intact(torch, odd_big, gv, planes, H, W, 3), f"{grid} {fmt}: a byte outside the odd window (guard planes, rows or pitch padding) was written"
            assert _guards_intact(torch, al_big, gv, planes, H, W, 8), f"{grid} {fmt}: a byte outside the aligned window was written"
            # frame 1 (the other slot of the batch) on a caller's stream, then straight into the next batch: that batch waits for the export
            e.peek_maps_device(view(dense), stream=side)
            _, host1 = e.peek_maps()
            assert e.collect()[0] == 7
            for f in frames:
                e.submit_frame(f, tag=8)
            side.synchronize()
            assert same(dense.cpu().numpy().reshape(host1.shape), host1)
            while e.in_flight():
                e.collect()
    finally:
        e.close()


def test_refusals_leave_the_engine_usable():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    torch = _torch()
    lib = _lib.lib
    e = _engine()
    frame = _frames(1, seed=37)[0]

    def works(mode_on=True):
        e.submit_frame(frame, tag=3)
        if mode_on:
            assert e.peek_maps()[0] == 3
        assert e.collect()[0] == 3 and e.in_flight() == 0

    def refused(call, code, *words, eng=None):
        """the call is refused with its reason; afterwards the engine still runs a frame (at once where it is idle; where the
        refusal happened with a frame in flight, that frame is peeked and collected further down)"""
        eng = eng or e
        before = eng.in_flight()
        with pytest.raises(r.RtpError) as ex:
            call()
        assert ex.value.code == code, ex.value
        for w in words:
            assert w in str(ex.value), ex.value
        assert eng.in_flight() == before
        if eng is e and before == 0:
            on = lib.rtp_maps_info(e.h, None, None, None) == r.RTP_OK
            works(on)

    def raw_set(**kw):
        cfg = _lib.rtp_maps_config()
        cfg.struct_size = C.sizeof(cfg)
        cfg.grid, cfg.format = 0, 2
        keep = None
        for k, v in kw.items():
            if k == "channels":
                keep = (C.c_int * len(v))(*v)
                cfg.channels = keep
            else:
                setattr(cfg, k, v)
        e._chk(lib.rtp_set_maps_output(e.h, C.byref(cfg)))

    def raw_view(**kw):
        (n0, nch, H, W), dt, nb = e.maps_info()
        t = torch.zeros((n0 * nch, H, W), dtype=torch.uint8, device="cuda")
        v = _lib.rtp_maps_view()
        v.struct_size = C.sizeof(v)
        v.data, v.channel_stride, v.row_stride = t.data_ptr(), H * W, W
        for k, val in kw.items():
            setattr(v, k, val)
        tag = C.c_uint64()
        e._chk(lib.rtp_peek_maps_device(e.h, C.byref(tag), C.byref(v), kw.get("_stream")))
        return t

    try:
        # ---- mode off
        refused(e.peek_maps, r.RTP_EINVAL)
        refused(e.maps_info, r.RTP_EINVAL)
        tag, buf = C.c_uint64(), np.zeros(64, np.uint8)
        assert lib.rtp_peek_maps(e.h, C.byref(tag), buf.ctypes.data_as(C.c_void_p), buf.size) == r.RTP_EINVAL and b"maps mode is off" in lib.rtp_last_error(e.h)
        assert lib.rtp_maps_from_lowres(e.h, None, buf.ctypes.data_as(C.c_void_p), buf.size) == r.RTP_EINVAL and b"maps mode is off" in lib.rtp_last_error(e.h)
        works(False)
        # ---- the switch
        refused(lambda: raw_set(struct_size=8), r.RTP_EINVAL, "struct_size")
        refused(lambda: raw_set(grid=2), r.RTP_EINVAL, "grid 2")
        refused(lambda: raw_set(format=3), r.RTP_EINVAL, "format 3")
        refused(lambda: raw_set(format=-1), r.RTP_EINVAL, "format -1")
        refused(lambda: raw_set(channels=[0, 57], num_channels=2), r.RTP_EINVAL, "channels[1] = 57")
        refused(lambda: raw_set(channels=[-1], num_channels=1), r.RTP_EINVAL, "channels[0] = -1")
        refused(lambda: raw_set(channels=[0], num_channels=0), r.RTP_EINVAL, "num_channels 0")
        refused(lambda: raw_set(channels=[0] * 71, num_channels=71), r.RTP_EINVAL, "num_channels 71")
        refused(e.maps_info, r.RTP_EINVAL)          # nothing was changed by a refused call
        works(False)
        e.submit_frame(frame, tag=1)
        refused(lambda: e.set_maps_output("net", "u8"), r.RTP_EAGAIN, "in flight")
        refused(lambda: e.set_maps_output(None), r.RTP_EAGAIN, "in flight")
        assert e.collect()[0] == 1
        e.set_maps_output("net", "u8", [0, 20])
        works()
        refused(lambda: raw_set(grid=7), r.RTP_EINVAL)
        assert e.maps_info()[0] == (1, 2, NET_H, NET_W)   # a refused switch keeps the mode that was on
        # ---- peeks
        refused(e.peek_maps, r.RTP_EAGAIN, "nothing in flight")
        nb = e.maps_info()[2]
        e.submit_frame(frame, tag=2)
        small = np.zeros(nb, np.uint8)
        assert lib.rtp_peek_maps(e.h, C.byref(tag), small.ctypes.data_as(C.c_void_p), nb - 1) == r.RTP_EINVAL and str(nb).encode() in lib.rtp_last_error(e.h)
        assert lib.rtp_peek_maps(e.h, C.byref(tag), None, nb) == r.RTP_EINVAL
        assert lib.rtp_maps_from_lowres(e.h, None, small.ctypes.data_as(C.c_void_p), nb) == r.RTP_EINVAL
        assert e.in_flight() == 1
        # views that fail the checks: fields, then memory
        refused(lambda: raw_view(struct_size=4), r.RTP_EINVAL, "struct_size")
        refused(lambda: raw_view(data=None), r.RTP_EINVAL, "NULL data")
        refused(lambda: raw_view(row_stride=NET_W - 1), r.RTP_EINVAL, "row_stride")
        refused(lambda: raw_view(channel_stride=NET_W * NET_H - 1), r.RTP_EINVAL, "channel_stride")
        exact = e.device_alloc(nb)                                                                        # an allocation of exactly one payload:
        try:
            raw_view(data=exact)                                                                          # the dense view fits,
            refused(lambda: raw_view(data=exact, channel_stride=NET_W * NET_H + 1), r.RTP_EINVAL, "allocation ends")   # one byte more per plane does not
        finally:
            e.synchronize()
            e.device_free(exact)
        host = np.zeros(nb, np.uint8)
        refused(lambda: raw_view(data=host.ctypes.data), r.RTP_EINVAL, "not memory of this library")        # pageable host memory
        with pytest.raises(ValueError):
            e.peek_maps_device(torch.zeros((2, NET_H, NET_W), dtype=torch.float32, device="cuda"))          # the wrapper: wrong dtype
        with pytest.raises(ValueError):
            e.peek_maps_device(torch.zeros((3, NET_H, NET_W), dtype=torch.uint8, device="cuda"))            # ... wrong shape
        # a capturing stream (the capture is opened and closed, never replayed)
        out = torch.zeros((2, NET_H, NET_W), dtype=torch.uint8, device="cuda")
        g = torch.cuda.CUDAGraph()
        x = torch.zeros(16, device="cuda")
        with torch.cuda.graph(g):
            x.add_(1)
            refused(lambda: e.peek_maps_device(out, stream=torch.cuda.current_stream()), r.RTP_EINVAL, "capturing")
        del g
        assert e.in_flight() == 1 and e.peek_maps()[0] == 2 and e.collect()[0] == 2
        refused(lambda: e.peek_maps_device(out), r.RTP_EAGAIN, "nothing in flight")
        e.submit_frame(frame, tag=4)
        refused(lambda: e.maps_from_lowres(np.zeros((e.N, e.heat_channels, e.low_h, e.low_w), np.float32)), r.RTP_EAGAIN, "idle")   # the tap needs an idle engine
        assert e.peek_maps()[0] == 4 and e.collect()[0] == 4
        works()
    finally:
        while e.in_flight():
            e.collect()
        e.close()
    # ---- a deferred-weights engine without weights
    d = _engine(defer_weights=1)
    try:
        d.set_maps_output("net", "u8")
        refused(d.peek_maps, r.RTP_EINVAL, "defer_weights", eng=d)
        refused(lambda: d.peek_maps_device(torch.zeros((57, NET_H, NET_W), dtype=torch.uint8, device="cuda")), r.RTP_EINVAL, "defer_weights", eng=d)
        refused(lambda: d.submit_frame(frame, tag=1), r.RTP_EINVAL, "defer_weights", eng=d)
    finally:
        d.close()


def test_cli_write_heatmaps_equals_peek_maps(tmp_path):
    import caffe_rtpose_amd as r
    prefix = tmp_path / "hm_"
    p = subprocess.run([BIN, "--video", "synthetic:320x180:6", "--model", "coco", "--net_resolution", "160x96", "--resolution", "320x180", "--write_heatmaps", str(prefix),
                        "--heatmap_channels", "all", "--no_frame_drops", "--no_display", "--num_gpu", "1"], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert sorted(os.listdir(tmp_path)) == ["hm_%06d.pgm" % i for i in range(6)]
    e = r.Engine(r.Config(net_w=NET_W, net_h=NET_H, disp_w=DISP_W, disp_h=DISP_H))   # the CLI's engine: its defaults
    try:
        e.set_maps_output("net", "u8")
        for i in range(6):
            e.submit_frame(r.synth_frame(320, 180, i, seed=2), tag=i)
            tag, maps = e.peek_maps()
            assert tag == i and e.collect()[0] == i
            img = mc.read_pgm(tmp_path / ("hm_%06d.pgm" % i))
            assert img.shape == (57 * NET_H, NET_W)
            assert np.array_equal(img.reshape(57, NET_H, NET_W), maps[0]), f"frame {i}: the file differs from peek_maps"
            assert maps.any(), "the maps of a synthetic frame are not all zero"
    finally:
        e.close()

"""Crops mode on the GPU.  Every comparison is byte for byte and float bit for float bit against rtp_crop_people (which
tests/test_crops_cpu.py holds to the numpy restatement): the parity tap on every case of tests/_cropcases.py in both layouts with both
store paths reached, the async path in graph and eager mode against the display image of debug_preprocess and the collected joints,
maps mode and the renderer next to it, frames without a display image, the device entry with guards, every refusal, the mode switched
off again, and rtpose.bin --write_crops against peek_crops."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import _cropcases as cc
import _cropref as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
NET_W, NET_H = 160, 96
GUARD = 0x5A
WIDE_CROPS = {(64, 64), (128, 96), (16, 48)}     # crop_w a multiple of 16: 16-byte stores into the engine's own buffers


def _torch():
    import torch   # (tests/conftest.py imported it before the engine library: one HIP runtime for both)
    return torch


def _engine(**kw):
    import caffe_rtpose_amd as r
    kw = dict(dict(net_w=NET_W, net_h=NET_H, disp_w=160, disp_h=96, frames_in_flight=4, batch_frames=2), **kw)
    e = r.Engine(r.Config(**kw))
    t = e.get_thresholds()
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], 2, 0.05)   # keep more "people" of the noise maps
    return e


def _layout(e, view=None):
    """the store path the host chooses in the engine's current mode (the unexported query): for its own buffers, or for a view"""
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_crops_layout
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(_lib.rtp_crops_view)]
    return fn(e.h, None if view is None else C.byref(view))


def _host(img, joints, e, **kw):
    """rtp_crop_people in the engine's current mode"""
    import caffe_rtpose_amd as r
    i = e.crops_info()
    return r.crop_people(img, joints, e.num_parts, i["crop_w"], i["crop_h"], i["max_crops"], layout=i["layout"], **kw)


def _same(got, want, what):
    gb, gc = got
    wb, wc = want
    assert cc.same_boxes(gb, wb), f"{what}: boxes differ in slots {np.flatnonzero((gb.view(np.uint32) != wb.view(np.uint32)).any(1)).tolist() if gb.shape == wb.shape else (gb.shape, wb.shape)}"
    assert gc.shape == wc.shape, f"{what}: {gc.shape} against {wc.shape}"
    bad = np.flatnonzero((gc != wc).reshape(len(wc), -1).any(1)).tolist() if len(wc) else []
    assert not bad, f"{what}: crops differ in slots {bad}"


@pytest.mark.parametrize("disp", cc.DISPLAYS, ids=lambda d: "%dx%d" % d)
def test_parity_tap_equals_the_host_definition_on_every_case(disp):
    W, H = disp
    e = _engine(disp_w=W, disp_h=H, frames_in_flight=1, batch_frames=1)
    img = cc.display(W, H)
    paths = set()
    try:
        for cw, ch in cc.CROPS:
            z = cc.zoo(W, H, cw, ch)
            joints = cc.joints_of(z)
            for layout in cc.LAYOUTS:
                e.set_crops_output(cw, ch, len(z), layout=layout)
                wide = _layout(e)
                assert wide == (1 if (cw, ch) in WIDE_CROPS else 0)
                paths.add(wide)
                got = e.crops_from_joints(img, joints)
                _same(got, _host(img, joints, e), f"{W}x{H} crop {cw}x{ch} layout {layout}")
                if layout == cr.HWC_BGR:
                    cc.check_predicates(z, got[0], got[1], W, H, cw, ch)
        assert paths == {0, 1}, "both store paths must be taken"
        for (vw, vh), (cw, ch), kw in cc.variations():
            if (vw, vh) != (W, H):
                continue
            z = cc.zoo(W, H, cw, ch)
            joints = cc.joints_of(z)
            for layout in cc.LAYOUTS:
                e.set_crops_output(cw, ch, len(z), layout=layout, **kw)
                _same(e.crops_from_joints(img, joints), _host(img, joints, e, **kw), f"{W}x{H} crop {cw}x{ch} layout {layout} {kw}")
        # people against max_crops: none, one, exactly max_crops, three more, and 96 of 96
        for people, max_crops, (cw, ch) in ((0, 4, (8, 8)), (1, 4, (64, 64)), (7, 7, (20, 12)), (10, 7, (16, 48)), (96, 96, (8, 8)), (96, 96, (16, 48))):
            joints = cc.joints_of(cc.zoo(W, H, cw, ch), people)
            e.set_crops_output(cw, ch, max_crops, margin=0.15)
            got = e.crops_from_joints(img, joints)
            assert len(got[0]) == len(got[1]) == min(people, max_crops)
            _same(got, _host(img, joints, e, margin=0.15), f"{people} people, max_crops {max_crops}")
            boxes_only, none = e.crops_from_joints(img, joints, pixels=False)
            assert none is None and cc.same_boxes(boxes_only, got[0])
    finally:
        e.close()


def _frames(n=4, seed=31, disp=(160, 96)):
    import caffe_rtpose_amd as r
    sizes = [disp, (640, 360)]   # at the display size (disp_cur is the frame itself), and through the warp
    return [r.synth_frame(*sizes[i % 2], i, seed=seed) for i in range(n)]


def _run(e, frames, peek=None, collect=None, tag0=50):
    """submit all, then per frame: peek (if given), collect -> [(peeked, collected)]"""
    for i, f in enumerate(frames):
        e.submit_frame(f, tag=tag0 + i)
    out = []
    while e.in_flight():
        p = peek() if peek else None
        out.append((p, (collect or e.collect)()))
    return out


def _peek_twice(e):
    def peek():
        t1, b1, c1 = e.peek_crops()
        t2, b2, c2 = e.peek_crops()
        assert t1 == t2 and cc.same_boxes(b1, b2) and c1.tobytes() == c2.tobytes(), "peeking twice gives the same"
        return t1, b1, c1
    return peek


def _check_frames(e, frames, results, what, kw):
    """every frame's peeked boxes and crops are rtp_crop_people(display image of debug_preprocess, collected joints); -> valid boxes per frame"""
    valid = []
    for f, ((ptag, boxes, crops), col) in zip(frames, results):
        ctag, n, joints = col[0], col[1], col[2]
        assert ptag == ctag
        _, disp, _ = e.debug_preprocess(f)
        _same((boxes, crops), _host(disp, joints[:n], e, **kw), f"{what}, tag {ctag}")
        valid.append(int(boxes[:, 5].sum()))
    return valid


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_async_path_boxes_and_crops_are_each_frames_own(mode):
    import caffe_rtpose_amd as r
    e = _engine(exec_mode=r.EXEC_GRAPH if mode == "graph" else r.EXEC_EAGER)
    frames = _frames(6)
    kw = dict(margin=0.15, min_parts=2)
    try:
        off = _run(e, frames)
        e.set_crops_output(64, 64, 16, **kw)
        assert _layout(e) == 1
        on = _run(e, frames, _peek_twice(e))
        for a, b in zip(off, on):
            assert a[1][1] == b[1][1] and np.array_equal(a[1][2], b[1][2]), "joints differ with crops on"
        valid = _check_frames(e, frames, on, f"{mode} 64x64", kw)
        print("valid boxes per frame:", valid, "people:", [c[1] for _, c in on])
        assert sum(v >= 1 for v in valid) >= 3, f"at least three frames need a valid box: {valid}"
        assert max(valid) >= 2, f"at least one frame needs two valid boxes: {valid}"
        assert len({c.tobytes() for (_, _, c), _ in on if len(c)}) >= 3, "the frames' crops must differ"
        # the byte-wise path, planar, the head parts, a partial batch at the end (5 frames in batches of 2)
        kw2 = dict(parts=r.crops_head_parts(r.MODEL_COCO_18), margin=1.0)
        e.set_crops_output(25, 17, 3, layout="chw_rgb", **kw2)
        assert _layout(e) == 0
        res = _run(e, frames[:5], _peek_twice(e))
        _check_frames(e, frames[:5], res, f"{mode} 25x17 planar head", kw2)
        assert any(len(b) == 3 and c[1] > 3 for (_, b, _), c in res), "a frame with more people than max_crops"
        # off again: the engine is what it was
        e.set_crops_output(None)
        again = _run(e, frames)
        assert all(a[1][1] == b[1][1] and np.array_equal(a[1][2], b[1][2]) for a, b in zip(again, off))
        with pytest.raises(r.RtpError):
            e.crops_info()
    finally:
        e.close()


def test_composes_with_maps_mode_and_the_renderer():
    e = _engine(render=1)
    frames = _frames(4, seed=33)
    kw = dict(margin=0.15)
    try:
        off = _run(e, frames, None, e.collect_rendered)
        e.set_maps_output("net", "u8", [0, 18])
        maps_only = _run(e, frames, e.peek_maps, e.collect_rendered)
        e.set_crops_output(64, 64, 8, **kw)

        def peek():
            mt, maps = e.peek_maps()
            t, b, c = e.peek_crops()
            assert mt == t
            return t, b, c, maps
        on = _run(e, frames, peek, e.collect_rendered)
        for a, m, b in zip(off, maps_only, on):
            assert len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1][1:], b[1][1:])), "joints or the rendered frame changed with crops on"
            assert np.array_equal(m[0][1], b[0][3]), "the maps changed with crops on"
        valid = _check_frames(e, frames, [((t, b, c), col) for (t, b, c, _), col in on], "render + maps", kw)   # (the un-rendered display image)
        assert sum(valid) >= 1
        assert any(not np.array_equal(col[3], e.debug_preprocess(f)[1]) for f, (_, col) in zip(frames, on)), "the renderer drew on some frame"
    finally:
        e.close()


def test_frames_without_a_display_image_get_boxes_and_no_pixels():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    torch = _torch()
    e = _engine()
    try:
        e.set_crops_output(64, 64, 16, margin=0.15)
        x, _, _ = e.debug_preprocess(_frames(1)[0])
        e.submit(x, tag=9)
        tag, boxes, crops = e.peek_crops()
        assert tag == 9 and crops is None
        cap = 16
        b2 = np.zeros((cap, r.CROP_BOX_FLOATS), np.float32)
        px = np.full((cap, 64, 64, 3), GUARD, np.uint8)
        n, has, t = C.c_int(), C.c_int(-1), C.c_uint64()
        e._chk(_lib.lib.rtp_peek_crops(e.h, C.byref(t), b2.ctypes.data_as(_lib.fp), C.byref(n), px.ctypes.data_as(C.POINTER(C.c_ubyte)), cap, C.byref(has)))
        assert has.value == 0 and (px == GUARD).all(), "no pixels: the caller's crop buffer stays untouched"
        with pytest.raises(r.RtpError) as ex:
            e.peek_crops_device(torch.zeros((16, 64, 64, 3), dtype=torch.uint8, device="cuda"))
        assert ex.value.code == r.RTP_EINVAL and "no display image" in str(ex.value)
        _, n_people, joints = e.collect()
        want, _ = _host(None, joints[:n_people], e, margin=0.15, pixels=False)
        assert cc.same_boxes(boxes, want) and n.value == len(want) and boxes[:, 5].sum() >= 1
        # the frame after it has pixels again
        f = _frames(1)[0]
        e.submit_frame(f, tag=10)
        tag, boxes, crops = e.peek_crops()
        assert tag == 10 and crops is not None and e.collect()[0] == 10
    finally:
        e.close()


def _view(t, stride):
    from caffe_rtpose_amd import _lib
    v = _lib.rtp_crops_view()
    v.struct_size = C.sizeof(v)
    v.data, v.crop_stride = t.data_ptr(), stride
    return v


def test_device_entry_both_store_paths_with_guards():
    torch = _torch()
    e = _engine()
    frames = _frames(2, seed=35)
    try:
        for (cw, ch), layout in (((64, 64), "hwc_bgr"), ((16, 48), "chw_rgb"), ((20, 12), "hwc_bgr")):
            M = 6
            e.set_crops_output(cw, ch, M, margin=0.15, layout=layout)
            shape = e.crops_info()["shape"]
            cb = e.crops_info()["crop_bytes"]
            # (a) a padded stride from an odd base address: the byte-wise path; (b) a padded stride of a multiple of 16 from an aligned
            # base and (c) a dense tensor: 16-byte stores where crop_w allows them
            odd_big = torch.full((1 + (M + 1) * (cb + 13),), GUARD, dtype=torch.uint8, device="cuda")
            odd = odd_big[1:].as_strided((M,) + shape, (cb + 13,) + tuple(int(np.prod(shape[i + 1:])) for i in range(3)))
            al_big = torch.full(((M + 1) * (cb + 48),), GUARD, dtype=torch.uint8, device="cuda")
            al = al_big[48:].as_strided((M,) + shape, (cb + 48,) + tuple(int(np.prod(shape[i + 1:])) for i in range(3)))
            dense = torch.full((M,) + shape, GUARD, dtype=torch.uint8, device="cuda")
            assert odd.data_ptr() % 2 == 1 and al.data_ptr() % 16 == 0
            wide_ok = 1 if cw % 16 == 0 else 0
            assert _layout(e, _view(odd, cb + 13)) == 0 and _layout(e, _view(al, cb + 48)) == wide_ok and _layout(e, _view(dense, cb)) == wide_ok
            side = torch.cuda.Stream()
            torch.cuda.synchronize()
            for f in frames:
                e.submit_frame(f, tag=7)
            tag, boxes, host = e.peek_crops()
            n = len(boxes)
            assert 1 <= n <= M
            t1, b1 = e.peek_crops_device(odd, stream=0)
            t2, b2 = e.peek_crops_device(al, stream=0)
            assert t1 == t2 == tag == 7 and cc.same_boxes(b1, boxes) and cc.same_boxes(b2, boxes)
            e.peek_crops_device(dense, stream=side)
            with torch.cuda.stream(side):
                later = dense.clone()            # enqueued on the caller's stream behind the peek: sees the crops
            side.synchronize()
            assert e.collect()[0] == 7
            for name, t, big, start, stride in (("odd", odd, odd_big, 1, cb + 13), ("aligned", al, al_big, 48, cb + 48)):
                assert np.array_equal(t[:n].cpu().numpy(), host), f"{cw}x{ch} {layout}: the {name} window differs from the host peek"
                flat = big.cpu().numpy().copy()
                for k in range(n):
                    flat[start + k * stride: start + k * stride + cb] = GUARD
                assert (flat == GUARD).all(), f"{cw}x{ch} {layout}: a byte outside the {n} crops of the {name} window was written (pitch padding, slots >= n, or around them)"
            assert np.array_equal(later[:n].cpu().numpy(), host) and (later[n:] == GUARD).all()
            # frame 1 (the other slot of the batch) on a caller's stream, then straight into the next batch: its staging waits for the export
            e.peek_crops_device(dense, stream=side)
            _, boxes1, host1 = e.peek_crops()
            assert e.collect()[0] == 7
            for f in frames:
                e.submit_frame(f, tag=8)
            side.synchronize()
            assert np.array_equal(dense[:len(boxes1)].cpu().numpy(), host1)
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
            assert e.peek_crops()[0] == 3
        assert e.collect()[0] == 3 and e.in_flight() == 0

    def refused(call, code, *words):
        before = e.in_flight()
        with pytest.raises(r.RtpError) as ex:
            call()
        assert ex.value.code == code, ex.value
        for w in words:
            assert w in str(ex.value), ex.value
        assert e.in_flight() == before
        if before == 0:
            works(lib.rtp_crops_info(e.h, None, None, None, None, None) == r.RTP_OK)

    keep = []

    def raw_set(**kw):
        cfg = _lib.rtp_crops_config()
        cfg.struct_size = C.sizeof(cfg)
        cfg.crop_w, cfg.crop_h, cfg.max_crops, cfg.min_parts = 64, 64, 4, 1
        for k, v in kw.items():
            if k == "parts":
                arr = (C.c_int * len(v))(*v)
                keep.append(arr)
                cfg.parts, cfg.num_parts = arr, len(v)
            else:
                setattr(cfg, k, v)
        e._chk(lib.rtp_set_crops_output(e.h, C.byref(cfg)))

    def raw_peek_device(t=None, **kw):
        t = torch.zeros((4, 64, 64, 3), dtype=torch.uint8, device="cuda") if t is None else t
        v = _lib.rtp_crops_view()
        v.struct_size = C.sizeof(v)
        v.data, v.crop_stride = (t if isinstance(t, int) else t.data_ptr()), 64 * 64 * 3
        for k, val in kw.items():
            if not k.startswith("_"):
                setattr(v, k, val)
        boxes = np.zeros((4, r.CROP_BOX_FLOATS), np.float32)
        n, tag = C.c_int(), C.c_uint64()
        e._chk(lib.rtp_peek_crops_device(e.h, C.byref(tag), boxes.ctypes.data_as(_lib.fp), C.byref(n), kw.get("_capacity", 4), C.byref(v), None))

    try:
        # ---- mode off
        refused(e.peek_crops, r.RTP_EINVAL)
        refused(e.crops_info, r.RTP_EINVAL)
        refused(lambda: e.crops_from_joints(np.zeros((96, 160, 3), np.uint8), np.zeros((1, 18, 3), np.float32)), r.RTP_EINVAL)
        works(False)
        # ---- the switch: every field
        refused(lambda: raw_set(struct_size=8), r.RTP_EINVAL, "struct_size")
        for bad, word in ((dict(crop_w=7), "crop_w"), (dict(crop_w=513), "crop_w"), (dict(crop_h=7), "crop_h"), (dict(crop_h=513), "crop_h"), (dict(max_crops=0), "max_crops"),
                          (dict(max_crops=97), "max_crops"), (dict(min_score=-1.0), "min_score"), (dict(min_score=float("nan")), "min_score"), (dict(min_parts=0), "min_parts"),
                          (dict(margin=-0.5), "margin"), (dict(margin=float("nan")), "margin"), (dict(margin=17.0), "margin"), (dict(layout=2), "layout"), (dict(layout=-1), "layout"),
                          (dict(parts=[0, 18]), "listed part"), (dict(parts=[-1]), "listed part"), (dict(parts=[0] * 71), "num_parts"), (dict(parts=[0], num_parts=0), "num_parts")):
            refused(lambda: raw_set(**bad), r.RTP_EINVAL, word)
        refused(e.crops_info, r.RTP_EINVAL)          # nothing was changed by a refused call
        e.submit_frame(frame, tag=1)
        refused(lambda: e.set_crops_output(64, 64, 4), r.RTP_EAGAIN, "in flight")
        refused(lambda: e.set_crops_output(None), r.RTP_EAGAIN, "in flight")
        assert e.collect()[0] == 1
        e.set_crops_output(64, 64, 4, margin=0.15)
        works()
        refused(lambda: raw_set(crop_w=5), r.RTP_EINVAL)
        assert e.crops_info()["crop_w"] == 64 and e.crops_info()["max_crops"] == 4    # a refused switch keeps the mode that was on
        # ---- peeks
        refused(e.peek_crops, r.RTP_EAGAIN, "nothing in flight")
        e.submit_frame(frame, tag=2)
        boxes = np.full((4, r.CROP_BOX_FLOATS), 7.5, np.float32)
        px = np.full((4, 64, 64, 3), GUARD, np.uint8)
        n, tag = C.c_int(-1), C.c_uint64()
        assert lib.rtp_peek_crops(e.h, C.byref(tag), None, C.byref(n), None, 4, None) == r.RTP_EINVAL
        assert lib.rtp_peek_crops(e.h, C.byref(tag), boxes.ctypes.data_as(_lib.fp), None, None, 4, None) == r.RTP_EINVAL
        rc = lib.rtp_peek_crops(e.h, C.byref(tag), boxes.ctypes.data_as(_lib.fp), C.byref(n), px.ctypes.data_as(C.POINTER(C.c_ubyte)), 0, None)
        if n.value > 0:    # fewer slots than the frame has boxes: the count comes back, nothing else is written
            assert rc == r.RTP_ERANGE and (boxes == 7.5).all() and (px == GUARD).all()
        assert e.in_flight() == 1
        # views that fail the checks: fields, then memory
        refused(lambda: raw_peek_device(struct_size=4), r.RTP_EINVAL, "struct_size")
        refused(lambda: raw_peek_device(data=None), r.RTP_EINVAL, "NULL data")
        refused(lambda: raw_peek_device(crop_stride=64 * 64 * 3 - 1), r.RTP_EINVAL, "crop_stride")
        exact = e.device_alloc(4 * 64 * 64 * 3)                                                          # an allocation of exactly max_crops crops:
        try:
            raw_peek_device(exact)                                                                        # the dense view fits,
            refused(lambda: raw_peek_device(exact, crop_stride=64 * 64 * 3 + 1), r.RTP_EINVAL, "allocation ends")   # one byte more per crop does not
        finally:
            e.synchronize()
            e.device_free(exact)
        host = np.zeros(4 * 64 * 64 * 3, np.uint8)
        refused(lambda: raw_peek_device(host.ctypes.data), r.RTP_EINVAL, "not memory of this library")      # pageable host memory
        with pytest.raises(ValueError):
            e.peek_crops_device(torch.zeros((4, 64, 64, 3), dtype=torch.float32, device="cuda"))           # the wrapper: wrong dtype
        with pytest.raises(ValueError):
            e.peek_crops_device(torch.zeros((3, 64, 64, 3), dtype=torch.uint8, device="cuda"))             # ... wrong shape
        assert e.in_flight() == 1 and e.peek_crops()[0] == 2 and e.collect()[0] == 2                     # the frame stayed peekable
        refused(lambda: e.peek_crops_device(torch.zeros((4, 64, 64, 3), dtype=torch.uint8, device="cuda")), r.RTP_EAGAIN, "nothing in flight")
        e.submit_frame(frame, tag=4)
        refused(lambda: e.crops_from_joints(np.zeros((96, 160, 3), np.uint8), np.zeros((1, 18, 3), np.float32)), r.RTP_EAGAIN, "idle")   # the tap needs an idle engine
        assert e.peek_crops()[0] == 4 and e.collect()[0] == 4
        works()
    finally:
        while e.in_flight():
            e.collect()
        e.close()


def test_mode_switched_off_is_an_engine_that_never_had_it():
    """joints and the launches of a batch (the per-stage timing counters have one entry per stage) are those of a fresh engine"""
    a, b = _engine(), _engine()
    frames = _frames(4, seed=41)
    try:
        b.set_crops_output(64, 64, 16)
        _run(b, frames, b.peek_crops)
        b.set_crops_output(None)
        ra, rb = _run(a, frames), _run(b, frames)
        for (_, x), (_, y) in zip(ra, rb):
            assert x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2])
        ma, mb = a.last_stage_ms(), b.last_stage_ms()
        assert list(ma) == list(mb) and all((ma[k] > 0) == (mb[k] > 0) for k in ma), (ma, mb)
    finally:
        a.close()
        b.close()


def _read_ppm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    assert parts[0] == b"P6" and parts[2] == b"255"
    w, h = (int(v) for v in parts[1].split())
    assert len(parts[3]) == w * h * 3
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def test_cli_write_crops_equals_peek_crops(tmp_path):
    import caffe_rtpose_amd as r
    prefix = tmp_path / "cr_"
    p = subprocess.run([BIN, "--video", "synthetic:320x180:6", "--model", "coco", "--net_resolution", "160x96", "--resolution", "160x96", "--write_crops", str(prefix),
                        "--crop_size", "48x64", "--crop_parts", "head", "--crop_margin", "0.5", "--max_crops", "5", "--no_frame_drops", "--no_display", "--num_gpu", "1"],
                       capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    files = sorted(os.listdir(tmp_path))
    e = r.Engine(r.Config(net_w=NET_W, net_h=NET_H, disp_w=160, disp_h=96))   # the CLI's engine: its defaults
    expect = []
    total = 0
    try:
        e.set_crops_output(48, 64, 5, parts=r.crops_head_parts(r.MODEL_COCO_18), margin=0.5)
        for i in range(6):
            e.submit_frame(r.synth_frame(320, 180, i, seed=2), tag=i)
            tag, boxes, crops = e.peek_crops()
            assert tag == i and e.collect()[0] == i
            expect.append("cr_%06d_boxes.json" % i)
            doc = json.load(open(tmp_path / expect[-1]))
            assert doc["frame"] == i and (doc["crop_w"], doc["crop_h"]) == (48, 64) and len(doc["boxes"]) == len(boxes)
            for k, (b, rec) in enumerate(zip(doc["boxes"], boxes)):
                got = np.array([b["left"], b["top"], b["width"], b["height"], b["parts"], b["valid"]], np.float32)
                assert b["person"] == k and cc.same_boxes(got, rec), f"frame {i} person {k}: {b} against {rec.tolist()}"
                if rec[5]:
                    expect.append("cr_%06d_%02d.ppm" % (i, k))
                    assert np.array_equal(_read_ppm(tmp_path / expect[-1]), crops[k][:, :, ::-1]), f"frame {i} person {k}: the file differs from peek_crops"
                    total += 1
    finally:
        e.close()
    assert files == sorted(expect) and total >= 1

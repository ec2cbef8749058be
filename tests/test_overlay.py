"""Overlay mode on the GPU.  Every comparison is integer for integer and byte for byte against rtp_overlay_update and rtp_overlay_draw
(which tests/test_overlay_cpu.py holds to the numpy restatement): the parity tap on every case sequence of tests/_overlaycases.py for
COCO and MPI, images whose sizes are multiples of no tile with items that end on tile borders and a frame whose 3168 items all cross
one tile, the async path — where the trail table is carried from frame to frame across the engine's streams and contexts — in graph
and eager mode at three pipeline shapes against a replay in submit order, the export modes, the mode switched off again, every
refusal and the life cycle of the state, and rtpose.bin --track --draw_tracks against the replay."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _overlaycases as oc
import _overlayref as orf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
NET_W, NET_H = 160, 96


def _engine(min_subset_cnt=2, **kw):
    import caffe_rtpose_amd as r
    kw = dict(dict(net_w=NET_W, net_h=NET_H, disp_w=160, disp_h=96, frames_in_flight=4, batch_frames=2, render=1), **kw)
    e = r.Engine(r.Config(**kw))
    t = e.get_thresholds()
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], min_subset_cnt, 0.05)   # keep more "people" of the noise maps
    return e


def _modes(e, tcfg, ocfg, scfg=None, next_id=1):
    """every mode off and on again: empty tables"""
    import caffe_rtpose_amd as r
    e.set_track_overlay(None)
    e.set_smoothing(None)
    e.set_tracking(None)
    e.set_tracking(tcfg)
    if next_id != 1:
        ts = r.TrackState(e.num_parts)
        ts.next_id = next_id
        e.set_track_state(ts)
    if scfg is not None:
        e.set_smoothing(scfg)
    e.set_track_overlay(ocfg)


@pytest.mark.parametrize("model", ["coco", "mpi"])
def test_parity_tap_equals_the_host_definitions_on_every_case(model):
    import caffe_rtpose_amd as r
    P = 18 if model == "coco" else 15
    e = _engine(frames_in_flight=1, batch_frames=1, model=r.MODEL_COCO_18 if model == "coco" else r.MODEL_MPI_15)
    bg = oc.background()
    try:
        assert e.num_parts == P
        for case in oc.cases(P):
            tcfg, ocfg = r.track_config(**case["tcfg"]), r.overlay_config(**case["ocfg"])
            _modes(e, tcfg, ocfg, next_id=case["next_id"])
            ts, st = r.TrackState(P), r.TrailState(P)
            ts.next_id = case["next_id"]
            items, states, recs = [], [], []
            for i, (joints, num_people) in enumerate(case["frames"]):
                want_recs = r.track_update(ts, joints, num_people, tcfg)
                want = r.overlay_update(st, joints, num_people, want_recs, ocfg)
                want_img = r.overlay_draw(want, bg.copy())
                got_recs, got, img = e.overlay_from_joints(joints, num_people, image=bg)
                assert np.array_equal(got_recs, want_recs), f"{case['name']} frame {i}: records\n{got_recs}\nthe host definition's\n{want_recs}"
                assert np.array_equal(got, want), f"{case['name']} frame {i}: items\n{got}\nthe host definition's\n{want}"
                got_state = e.overlay_state()
                assert got_state == st, f"{case['name']} frame {i}: the trail table differs: {orf.same_state(oc.as_ref(st), got_state)}"
                assert e.track_state() == ts, f"{case['name']} frame {i}: the track table differs"
                assert np.array_equal(img, want_img), f"{case['name']} frame {i}: the image differs at {np.argwhere((img != want_img).any(axis=2))[:5].tolist()}"
                items.append(oc.as_tuples(got))
                states.append(oc.as_ref(got_state))
                recs.append(got_recs.astype(np.int64))
            oc.check_predicates(case, items, states, recs)
    finally:
        e.close()


def _corners(P, x0, y0, x1, y1):
    """a person of three scored parts whose box (margin 0) is exactly [x0, x1] x [y0, y1]"""
    j = np.zeros((P, 3), np.float32)
    j[0], j[1], j[2] = (x0, y0, 1.0), (x1, y1, 1.0), (x0, y1, 1.0)
    return j


def test_tile_edges_and_a_tile_with_more_items_than_the_lds_list_holds():
    """168 x 100 is a multiple of no tile (32 x 16 pixels; tile columns start at multiples of 32, rows at multiples of 16).  Frame 0:
    boxes that end exactly on tile borders, on both sides of them, and one-pixel boxes in the last column and row.  Then 32 frames of 96
    people inside one tile: the last frames have 96 * 33 = 3168 half-transparent, overlapping items through it, 6 times what the LDS
    list holds, and the blends do not commute: without the rounds, or with a compaction that loses the order, the image differs."""
    import caffe_rtpose_amd as r
    P, W, H = 18, 168, 100
    e = _engine(frames_in_flight=1, batch_frames=1, disp_w=W, disp_h=H)
    bg = oc.background(W, H)
    tcfg = r.track_config(min_parts=1, min_common=1)
    try:
        ocfg = r.overlay_config(box_margin=0, line_width=1, alpha=128, trail_len=32, trail_radius=2)
        _modes(e, tcfg, ocfg)
        ts, st = r.TrackState(P), r.TrailState(P)
        edges = np.stack([_corners(P, 32, 16, 63, 31), _corners(P, 64, 32, 64, 47), _corners(P, 31, 48, 32, 63), _corners(P, 96, 15, 127, 16), _corners(P, 0, 0, 31, 15),
                          _corners(P, 167, 99, 167, 99), _corners(P, 160, 96, 167, 99), _corners(P, 167, 40, 167, 40), _corners(P, 80, 99, 80, 99), _corners(P, 128, 64, 200, 120)])
        seq = [(edges, ocfg)]
        # the crowd: 96 people in tile (2, 2) = [64, 95] x [32, 47], 2 x 1.5 pixels apart, drifting by a quarter pixel per frame
        base = np.stack([oc.body(P, 62 + 2.0 * (k % 12), 26 + 1.5 * (k // 12)) for k in range(96)]).astype(np.float32)
        crowd_cfg = r.overlay_config(box_margin=1, line_width=2, alpha=128, trail_len=32, trail_radius=3, label_scale=1)
        seq += [(base + np.array([0.25 * i, 0.5 * (i % 2), 0], np.float32), crowd_cfg) for i in range(33)]
        most = 0
        for i, (joints, cfg) in enumerate(seq):
            e.set_track_overlay(cfg)        # (a new configuration keeps the table)
            want_recs = r.track_update(ts, joints, None, tcfg)
            want = r.overlay_update(st, joints, None, want_recs, cfg)
            want_img = r.overlay_draw(want, bg.copy())
            got_recs, got, img = e.overlay_from_joints(joints, image=bg)
            assert np.array_equal(got_recs, want_recs), f"frame {i}: records"
            assert np.array_equal(got, want), f"frame {i}: items"
            assert np.array_equal(img, want_img), f"frame {i} ({len(want)} items): the image differs at {np.argwhere((img != want_img).any(axis=2))[:5].tolist()}"
            most = max(most, len(want))
            if i == 0:
                assert len(want) == 2 * len(edges) and (img[99, 167] != bg[99, 167]).any() and (img[99, 80] != bg[99, 80]).any() and (img[40, 167] != bg[40, 167]).any()
        assert e.overlay_state() == st and most == r.OVERLAY_MAX_ITEMS == 3168, most
        # so that the last frame cannot pass by accident: the same list in reverse order gives another image
        assert not np.array_equal(r.overlay_draw(want[::-1].copy(), bg.copy()), want_img)
        in_tile = sum(1 for it in want if min(it[1], it[3]) - 3 <= 95 and max(it[1], it[3]) + 3 >= 64 and min(it[2], it[4]) - 3 <= 47 and max(it[2], it[4]) + 3 >= 32)
        assert in_tile > 4 * 512, in_tile
    finally:
        e.close()


def test_state_round_trip():
    import caffe_rtpose_amd as r
    e = _engine(frames_in_flight=1, batch_frames=1)
    try:
        e.set_tracking()
        e.set_track_overlay()
        rng = np.random.default_rng(3)
        st = r.TrailState(18)
        st.frames = 0xFFFFFFF0
        st.slot["owner"][:] = rng.integers(-2 ** 31, 2 ** 31, 128)
        st.slot["count"][:] = rng.integers(0, 33, 128)
        st.slot["head"][:] = rng.integers(0, 32, 128)
        st.slot["pts"][:] = rng.integers(-2 ** 31, 2 ** 31, (128, 32, 2))     # any bits
        e.set_overlay_state(st)
        assert e.overlay_state() == st
        ts = e.track_state()
        e.overlay_reset()
        assert e.overlay_state() == r.TrailState(18) and e.track_state() == ts
        # the tracker's reset and state entries leave the trail table alone
        e.set_overlay_state(st)
        e.track_reset()
        e.set_track_state(r.TrackState(18))
        assert e.overlay_state() == st
    finally:
        e.close()


def _frames(order="AABAABBA", seed=41):
    import caffe_rtpose_amd as r
    content = {"A": r.synth_frame(160, 96, 0, seed=seed), "B": r.synth_frame(640, 360, 1, seed=seed)}   # B goes through the warp
    return [content[c] for c in order]


def _stream(e, frames, depth, smooth=False, overlay=True, collect=None, tag0=70, extra=None):
    """submit as many frames as fit before each collect; per frame peek_tracks, peek_smoothed, peek_overlay_items (twice), extra() and
    collect -> [dict(recs, js, items, extra, col)]"""
    out, nxt = [], 0
    while nxt < len(frames) or e.in_flight():
        while nxt < len(frames) and e.in_flight() < depth:
            e.submit_frame(frames[nxt], tag=tag0 + nxt)
            nxt += 1
        d = dict(recs=e.peek_tracks()[1])
        if smooth:
            d["js"] = e.peek_smoothed()[1]
        if overlay:
            t1, d["items"] = e.peek_overlay_items()
            t2, again = e.peek_overlay_items()
            assert t1 == t2 == tag0 + len(out) and np.array_equal(d["items"], again), "peeking twice gives the same"
        d["extra"] = extra() if extra else None
        d["col"] = (collect or e.collect_rendered)()
        assert d["col"][0] == tag0 + len(out)
        out.append(d)
    return out


def _replay(e, results, frames, tcfg, ocfg, scfg=None, P=18):
    """the host definitions over the collected raw joints in submit order -> per frame (records, items, expected rendered image), states"""
    import caffe_rtpose_amd as r
    ts, ss, st = r.TrackState(P), r.SmoothState(P), r.TrailState(P)
    late = scfg is not None and scfg.apply & r.SMOOTH_RENDER
    want = []
    for d, f in zip(results, frames):
        n, joints = d["col"][1], d["col"][2]
        recs = r.track_update(ts, joints[:n], cfg=tcfg)
        js = r.smooth_update(ss, joints[:n], None, recs, scfg)[0] if scfg is not None else None
        poses = js if late else joints[:n]
        items = r.overlay_update(st, poses, None, recs, ocfg)
        img = e.render(e.debug_preprocess(f)[1], poses, n)
        want.append((recs, items, r.overlay_draw(items, img.copy()), img))
    return want, ts, st


PIPELINES = [(4, 2), (6, 1), (2, 2)]


@pytest.mark.parametrize("mode", ["graph", "eager"])
@pytest.mark.parametrize("pipe", PIPELINES, ids=lambda p: "inflight%d_batch%d" % p)
def test_async_path_draws_every_frame_in_submit_order(mode, pipe):
    """What this test shows: the draw lists, records, tables and rendered frames of frames that ran on different streams and contexts
    equal a replay in submit order.  Like tests/test_smooth.py it does NOT show that the wait in front of each frame's track kernel is
    needed: that the event is recorded behind the update kernel and waited for by the next frame rests on reading engine_track.cpp,
    engine_smooth.cpp and engine_overlay.cpp."""
    import caffe_rtpose_amd as r
    depth, batch = pipe
    e = _engine(frames_in_flight=depth, batch_frames=batch, exec_mode=r.EXEC_GRAPH if mode == "graph" else r.EXEC_EAGER)
    frames = _frames()
    tcfg, ocfg = r.track_config(), r.overlay_config(trail_len=4, alpha=160)
    kinds = {}
    try:
        for scfg in (None, r.smooth_config(apply=0), r.smooth_config(apply=r.SMOOTH_RENDER, beta=0.3)):
            _modes(e, tcfg, ocfg, scfg)
            res = _stream(e, frames, depth, smooth=scfg is not None)
            tables = e.track_state(), e.overlay_state()
            want, ts, st = _replay(e, res, frames, tcfg, ocfg, scfg)
            assert tables == (ts, st), f"{mode} {pipe}: the final tables differ from the replay's"
            assert st.frames == len(frames)
            for i, (d, (recs, items, img, plain)) in enumerate(zip(res, want)):
                assert np.array_equal(d["recs"], recs), f"{mode} {pipe} frame {i}: records"
                assert np.array_equal(d["items"], items), f"{mode} {pipe} frame {i}: items\n{d['items']}\nthe replay's\n{items}"
                assert np.array_equal(d["col"][3], img), f"{mode} {pipe} frame {i}: the rendered frame"
                assert len(items) == 0 or not np.array_equal(img, plain)
                for k in items[:, 0]:
                    kinds[int(k)] = kinds.get(int(k), 0) + 1
        print(mode, pipe, "item kinds seen:", kinds)
        assert all(kinds.get(k, 0) >= 1 for k in (1, 2, 3)), "so that the test cannot pass vacuously: boxes, labels and trails were drawn"
    finally:
        e.close()


def test_export_modes_carry_the_drawing():
    import torch
    import caffe_rtpose_amd as r
    e = _engine()
    frames = _frames("ABAB", seed=43)
    tcfg, ocfg = r.track_config(), r.overlay_config(label_scale=2)
    try:
        _modes(e, tcfg, ocfg)
        want, _, _ = _replay(e, _stream(e, frames, 4), frames, tcfg, ocfg)
        assert sum(len(w[1]) for w in want) >= 1, "the frames need tracked people"
        out = torch.zeros((96, 160, 3), dtype=torch.uint8, device="cuda")

        def collect_device():
            t, n, j = e.collect_rendered_device(out)
            torch.cuda.synchronize()
            return t, n, j, out.cpu().numpy().copy()

        def collect_yuv():
            t, j, y, u, v = e.collect_rendered_yuv()
            return t, len(j), j, (y.copy(), u.copy(), v.copy())
        for form, collect in (("device", collect_device), ("yuv", collect_yuv), ("jpeg", e.collect_rendered_jpeg)):
            _modes(e, tcfg, ocfg)
            if form == "yuv":
                e.set_render_yuv(420)
            if form == "jpeg":
                e.set_render_yuv(0)
                e.set_render_jpeg(90)
            res = _stream(e, frames, 4, collect=collect)
            for i, (d, (recs, items, img, _)) in enumerate(zip(res, want)):
                assert np.array_equal(d["items"], items), f"{form} frame {i}: items"
                got = d["col"][3]
                if form == "device":
                    assert np.array_equal(got, img), f"{form} frame {i}"
                elif form == "yuv":
                    assert all(np.array_equal(a, b) for a, b in zip(got, r.convert_bgr_to_yuv(img, 420))), f"{form} frame {i}"
                else:
                    assert got == r.encode_jpeg(img, 90), f"{form} frame {i}"
        e.set_render_jpeg(0)
    finally:
        e.close()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(p).view(np.uint8), np.asarray(q).view(np.uint8)) for p, q in zip(a, b))


def test_mode_off_changes_nothing():
    """an engine that had the mode on and switched it off again returns the bytes of an engine with tracking (and smoothing) alone:
    rendered frames, crops, maps, records and smoothed arrays"""
    import caffe_rtpose_amd as r
    e = _engine()
    frames = _frames("ABBA", seed=43)
    tcfg, scfg = r.track_config(), r.smooth_config(apply=r.SMOOTH_RENDER | r.SMOOTH_CROPS)

    def run(overlay):
        e.set_track_overlay(None)
        e.set_smoothing(None)
        e.set_tracking(None)
        e.set_tracking(tcfg)
        e.set_smoothing(scfg)
        if overlay:
            e.set_track_overlay(r.overlay_config())
        e.set_maps_output("net", "u8", [0, 18])
        e.set_crops_output(64, 64, 16, margin=0.15)
        res = _stream(e, frames, 4, smooth=True, overlay=overlay, extra=lambda: (e.peek_smoothed()[1:], e.peek_crops()[1:], e.peek_maps()[1]))
        e.set_crops_output(None)
        e.set_maps_output(None)
        return res
    try:
        alone = run(False)
        drawn = run(True)
        after = run(False)
        for a, b, c in zip(alone, after, drawn):
            assert a["col"][1] == b["col"][1] and _same(a["col"][2:], b["col"][2:]), "the rendered frames and joints of the tracking-only engine"
            assert np.array_equal(a["recs"], b["recs"]) and _same(a["extra"][0], b["extra"][0]) and _same(a["extra"][1], b["extra"][1]) and np.array_equal(a["extra"][2], b["extra"][2])
            # and with the mode on only the rendered frame changes
            assert np.array_equal(a["recs"], c["recs"]) and _same(a["extra"][0], c["extra"][0]) and _same(a["extra"][1], c["extra"][1]) and np.array_equal(a["extra"][2], c["extra"][2])
            assert np.array_equal(a["col"][2].view(np.uint32), c["col"][2].view(np.uint32))
            assert np.array_equal(c["col"][3], r.overlay_draw(c["items"], a["col"][3].copy()))
        assert sum(len(c["items"]) for c in drawn) >= 1
    finally:
        e.close()


def test_frames_without_a_display_image_and_synchronous_taps():
    import caffe_rtpose_amd as r
    e = _engine()
    try:
        e.set_tracking()
        e.set_track_overlay()
        f = _frames("A")[0]
        x, disp, _ = e.debug_preprocess(f)
        e.forward_debug(x)
        e.render(disp, oc.body(18, 40, 20)[None], 1)
        e.track_from_joints(oc.body(18, 40, 20)[None])     # the tracker's own tap advances the tracker alone
        assert e.overlay_state() == r.TrailState(18) and e.track_state().frames == 1
        e.track_reset()
        # a net input is a submitted frame like any other: the table advances and the frame has a list, nothing is drawn
        e.submit(x, tag=1)
        _, recs = e.peek_tracks()
        _, items = e.peek_overlay_items()
        _, n, joints = e.collect()
        ts, st = r.TrackState(18), r.TrailState(18)
        want_recs = r.track_update(ts, joints[:n])
        assert np.array_equal(recs, want_recs) and np.array_equal(items, r.overlay_update(st, joints[:n], None, want_recs)) and e.overlay_state() == st and st.frames == 1
        # and a frame with an image continues from there
        e.submit_frame(f, tag=2)
        _, items2 = e.peek_overlay_items()
        _, n2, j2, img = e.collect_rendered()
        want2 = r.overlay_update(st, j2[:n2], None, r.track_update(ts, j2[:n2]))
        assert np.array_equal(items2, want2) and np.array_equal(img, r.overlay_draw(want2, e.render(disp, j2[:n2], n2).copy()))
        assert len(want2) >= 1, "the frame needs a tracked person"
    finally:
        e.close()


def test_refusals_and_lifecycle():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    one = np.zeros((1, 18, 3), np.float32)
    plain = _engine(render=0)
    try:
        plain.set_tracking()
        with pytest.raises(r.RtpError) as ex:
            plain.set_track_overlay()
        assert ex.value.code == r.RTP_EINVAL and "render" in str(ex.value)
    finally:
        plain.close()
    e = _engine()
    frames = _frames("AB", seed=45)
    try:
        with pytest.raises(r.RtpError) as ex:     # tracking off: no overlay
            e.set_track_overlay()
        assert ex.value.code == r.RTP_EINVAL and "tracking" in str(ex.value)
        e.set_track_overlay(None)        # off while off is fine
        tcfg = r.track_config(min_parts=2)
        e.set_tracking(tcfg)
        for call in (e.peek_overlay_items, e.overlay_reset, e.overlay_state, lambda: e.set_overlay_state(r.TrailState(18)), lambda: e.overlay_from_joints(one)):
            with pytest.raises(r.RtpError) as ex:
                call()
            assert ex.value.code == r.RTP_EINVAL and "off" in str(ex.value)
        for kw in (dict(what=0), dict(what=8), dict(min_score=-1.0), dict(min_score=float("nan")), dict(box_margin=-1), dict(box_margin=1025), dict(line_width=0),
                   dict(line_width=17), dict(label_scale=0), dict(label_scale=9), dict(trail_len=-1), dict(trail_len=33), dict(trail_radius=-1), dict(trail_radius=17),
                   dict(alpha=-1), dict(alpha=257)):
            with pytest.raises(r.RtpError) as ex:
                e.set_track_overlay(r.overlay_config(**kw))
            assert ex.value.code == r.RTP_EINVAL, kw
        bad = r.overlay_config()
        bad.struct_size += 4
        with pytest.raises(r.RtpError):
            e.set_track_overlay(bad)
        ocfg = r.overlay_config(trail_len=3)
        e.set_track_overlay(ocfg)
        with pytest.raises(r.RtpError) as ex:
            e.peek_overlay_items()
        assert ex.value.code == r.RTP_EAGAIN   # nothing in flight
        with pytest.raises(r.RtpError) as ex:  # the tracker cannot go while the overlay needs it; a new tracking configuration is fine
            e.set_tracking(None)
        assert ex.value.code == r.RTP_EINVAL and "overlay" in str(ex.value)
        e.set_tracking(tcfg)
        with pytest.raises(r.RtpError) as ex:
            e.set_overlay_state(r.TrailState(15))
        assert ex.value.code == r.RTP_EINVAL and "parts" in str(ex.value)
        for field, v in (("count", 33), ("head", 32), ("head", -1)):
            broken = r.TrailState(18)
            broken.slot[field][5] = v
            with pytest.raises(r.RtpError) as ex:
                e.set_overlay_state(broken)
            assert ex.value.code == r.RTP_EINVAL
        wrong = r.TrailState(18)
        wrong.c.struct_size = 12
        with pytest.raises(r.RtpError):
            e.set_overlay_state(wrong)
        big = np.zeros((97, 161, 3), np.uint8)
        for img in (big[:, :160], big[:96]):
            with pytest.raises(r.RtpError) as ex:
                e.overlay_from_joints(one, image=img)
            assert ex.value.code == r.RTP_EINVAL and "display" in str(ex.value)
        assert e.overlay_state() == r.TrailState(18), "a refused tap advances nothing"
        # with a frame in flight: no switch, no reset, no state entry, no tap
        e.submit_frame(frames[0], tag=1)
        for call in (lambda: e.set_track_overlay(None), lambda: e.set_track_overlay(r.overlay_config()), e.overlay_reset, e.overlay_state,
                     lambda: e.set_overlay_state(r.TrailState(18)), lambda: e.overlay_from_joints(one)):
            with pytest.raises(r.RtpError) as ex:
                call()
            assert ex.value.code == r.RTP_EAGAIN
        # capacity below the count: RTP_ERANGE with *num_items set, and the frame stays peekable
        tag, items = e.peek_overlay_items()
        m = len(items)
        assert tag == 1 and m >= 1, "the frame needs a tracked person"
        buf = np.full((m, 9), 77, np.int32)
        got_m, t = C.c_int(-1), C.c_uint64()
        assert _lib.lib.rtp_peek_overlay_items(e.h, C.byref(t), buf.ctypes.data_as(_lib.ip), C.byref(got_m), m - 1) == r.RTP_ERANGE
        assert got_m.value == m and (buf == 77).all()
        assert _lib.lib.rtp_peek_overlay_items(e.h, C.byref(t), None, C.byref(got_m), m) == r.RTP_EINVAL
        assert _lib.lib.rtp_peek_overlay_items(e.h, C.byref(t), buf.ctypes.data_as(_lib.ip), C.byref(got_m), m) == r.RTP_OK and np.array_equal(buf, items)
        _, recs = e.peek_tracks()
        _, n1, j1, _ = e.collect_rendered()
        ts, st = r.TrackState(18), r.TrailState(18)
        assert np.array_equal(recs, r.track_update(ts, j1[:n1], cfg=tcfg)) and np.array_equal(items, r.overlay_update(st, j1[:n1], None, recs, ocfg)) and e.overlay_state() == st
        # a new configuration while the mode is on keeps the table
        ocfg2 = r.overlay_config(trail_len=2, what=r.OVERLAY_BOX | r.OVERLAY_TRAIL)
        e.set_track_overlay(ocfg2)
        assert e.overlay_state() == st
        # the tap advances both tables (without an image too), and frames submitted next continue from them
        person = oc.body(18, 40, 20)[None]
        got_recs, got, img = e.overlay_from_joints(person)
        want_recs = r.track_update(ts, person, cfg=tcfg)
        assert img is None and np.array_equal(got_recs, want_recs) and np.array_equal(got, r.overlay_update(st, person, None, want_recs, ocfg2))
        assert e.overlay_state() == st and e.track_state() == ts
        e.submit_frame(frames[1], tag=2)
        _, recs2 = e.peek_tracks()
        _, items2 = e.peek_overlay_items()
        _, n2, j2, _ = e.collect_rendered()
        assert np.array_equal(recs2, r.track_update(ts, j2[:n2], cfg=tcfg)) and np.array_equal(items2, r.overlay_update(st, j2[:n2], None, recs2, ocfg2))
        assert e.overlay_state() == st and st.frames == 3
        # a reset mid-stream, and off -> on: both start from an empty table
        for restart in (e.overlay_reset, lambda: (e.set_track_overlay(None), e.set_track_overlay(ocfg2))):
            restart()
            assert e.overlay_state() == r.TrailState(18)
        e.set_track_overlay(None)
        e.set_track_overlay(None)         # off twice is fine
        with pytest.raises(r.RtpError):
            e.overlay_state()
        e.set_tracking(None)          # and now the tracker may go
    finally:
        e.close()


def test_cli_draw_tracks_equals_the_replay(tmp_path):
    """rtpose.bin --track --draw_tracks --write_video: drawn on the GPU (the engine's mode, then the GPU's YUV conversion) and, with
    --host_draw, by the re-orderer on the raw rendered frame (rtp_overlay_update + rtp_overlay_draw, then the host conversion): the
    same bytes, and the frames of a replay through an engine of the CLI's shape"""
    import caffe_rtpose_amd as r
    files = {}
    for mode in ("gpu", "host"):
        out = tmp_path / f"{mode}.y4m"
        p = subprocess.run([BIN, "--video", "synthetic:320x180:6", "--model", "coco", "--net_resolution", "160x96", "--resolution", "160x96", "--write_video", str(out), "--track",
                            "--track_min_parts", "2", "--track_max_misses", "1", "--draw_tracks", "--trail_len", "4", "--label_scale", "2", "--draw_alpha", "200",
                            "--no_frame_drops", "--no_display", "--num_gpu", "1"] + (["--host_draw"] if mode == "host" else []), capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        assert (b"on the GPU" in p.stderr) == (mode == "gpu"), p.stderr.decode()[-3000:]
        files[mode] = open(out, "rb").read()
    assert files["gpu"] == files["host"] and len(files["gpu"]) > 0
    e = r.Engine(r.Config(net_w=NET_W, net_h=NET_H, disp_w=160, disp_h=96, render=1))   # the CLI's engine: its defaults
    want = tmp_path / "want.y4m"
    wr = r.VideoWriter(want, 160, 96)
    items_seen = 0
    try:
        tcfg, ocfg = r.track_config(min_parts=2, max_misses=1), r.overlay_config(trail_len=4, label_scale=2, alpha=200)
        e.set_tracking(tcfg)
        e.set_track_overlay(ocfg)
        ts, st = r.TrackState(18), r.TrailState(18)
        for i in range(6):
            f = r.synth_frame(320, 180, i, seed=2)
            e.submit_frame(f, tag=i)
            _, items = e.peek_overlay_items()
            _, n, joints, img = e.collect_rendered()
            recs = r.track_update(ts, joints[:n], cfg=tcfg)
            assert np.array_equal(items, r.overlay_update(st, joints[:n], None, recs, ocfg)), f"frame {i}"
            assert np.array_equal(img, r.overlay_draw(items, e.render(e.debug_preprocess(f)[1], joints[:n], n).copy())), f"frame {i}"
            wr.write_bgr(img)
            items_seen += len(items)
    finally:
        wr.close()
        e.close()
    assert items_seen >= 1, "the frames need tracked people"
    assert open(want, "rb").read() == files["gpu"]


def _draw_list(e, items, image):
    """the unexported entry that runs overlay_draw_kernel alone on a caller's list (idle engine, mode on) -> the image with the drawing"""
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_overlay_draw_list
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, _lib.ip, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int]
    it = orf.as_array(items)
    img = np.ascontiguousarray(image, np.uint8).copy()
    e._chk(fn(e.h, it.ctypes.data_as(_lib.ip) if it.size else None, len(it), img.ctypes.data_as(C.POINTER(C.c_ubyte)), img.shape[1], img.shape[0]))
    return img


def test_the_draw_kernel_on_hand_written_lists():
    """what the update kernel never emits: kinds that do not exist, sizes, alphas and coordinates out of their range, rectangles with
    x0 > x1, every label scale, items outside the image and across each border; at the display size and at sizes that are multiples
    of no tile"""
    import caffe_rtpose_amd as r
    e = _engine(frames_in_flight=1, batch_frames=1, disp_w=168, disp_h=100)
    try:
        e.set_tracking()
        e.set_track_overlay()
        for w, h in ((160, 96), (168, 100), (37, 23), (1, 1)):
            bg = oc.background(w, h)
            for name, items in oc.draw_lists(w, h) + [("overlapping_%d" % o, oc.overlapping(o)) for o in (0, 1)] + [("empty", [])]:
                want = r.overlay_draw(orf.as_array(items), bg.copy())
                got = _draw_list(e, items, bg)
                assert np.array_equal(got, want), f"{name} {w}x{h}: the image differs at {np.argwhere((got != want).any(axis=2))[:5].tolist()}"
        assert e.overlay_state() == r.TrailState(18), "no table is touched"
    finally:
        e.close()


def test_cli_host_draw_with_smoothing_draws_the_smoothed_people(tmp_path):
    """--smooth with one GPU worker renders the smoothed people (RTP_SMOOTH_RENDER), and so does the overlay on either path: the
    re-orderer takes the smoothed joints the engine handed out, and the files are the same bytes"""
    files = {}
    for mode in ("gpu", "host"):
        out = tmp_path / f"{mode}.y4m"
        p = subprocess.run([BIN, "--video", "synthetic:320x180:6", "--model", "coco", "--net_resolution", "160x96", "--resolution", "160x96", "--write_video", str(out), "--track",
                            "--track_min_parts", "2", "--smooth", "--smooth_beta", "0.1", "--draw_tracks", "--trail_len", "6", "--no_frame_drops", "--no_display",
                            "--num_gpu", "1"] + (["--host_draw"] if mode == "host" else []), capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        files[mode] = open(out, "rb").read()
    assert files["gpu"] == files["host"] and len(files["gpu"]) > 0

"""Smoothing mode on the GPU.  Every comparison is float bit for float bit and byte for byte against rtp_smooth_update (which
tests/test_smooth_cpu.py holds to the numpy restatement): the parity tap on every case sequence of tests/_smoothcases.py for COCO
and MPI in both workgroup sizes, the state round trip, the async path — where both tables are carried from frame to frame across
the engine's streams and contexts — in graph and eager mode at three pipeline shapes against a replay in submit order, the apply
flags against the render and crops definitions on the smoothed people, the other output modes next to it, every refusal, the life
cycle of the state, and rtpose.bin --track --smooth against peek_smoothed."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import _smoothcases as sc
import _smoothref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
NET_W, NET_H = 160, 96
VARIANTS = {"wg256": 0, "wg1024": 1}   # kernels.h RTP_SMOOTH_*: the workgroup's size


def _engine(min_subset_cnt=2, **kw):
    import caffe_rtpose_amd as r
    kw = dict(dict(net_w=NET_W, net_h=NET_H, disp_w=160, disp_h=96, frames_in_flight=4, batch_frames=2), **kw)
    e = r.Engine(r.Config(**kw))
    t = e.get_thresholds()
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], min_subset_cnt, 0.05)   # keep more "people" of the noise maps
    return e


def _variant(e, v):
    """the unexported switch between the kernel's two builds (idle engine) -> the previous one"""
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_smooth_variant
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    before = fn(e.h, v)
    assert before >= 0, before
    return before


def _modes(e, tcfg, scfg):
    """both modes off and on again: empty tables"""
    e.set_smoothing(None)
    e.set_tracking(None)
    e.set_tracking(tcfg)
    e.set_smoothing(scfg)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("model", ["coco", "mpi"])
def test_parity_tap_equals_the_host_definition_on_every_case(model, variant):
    import caffe_rtpose_amd as r
    P = 18 if model == "coco" else 15
    e = _engine(frames_in_flight=1, batch_frames=1, model=r.MODEL_COCO_18 if model == "coco" else r.MODEL_MPI_15)
    try:
        assert e.num_parts == P
        assert _variant(e, VARIANTS[variant]) in VARIANTS.values()
        e.set_tracking()
        for case in sc.cases(P):
            tcfg, scfg = r.track_config(**case["tcfg"]), r.smooth_config(**case["scfg"])
            _modes(e, tcfg, scfg)
            ts, st = r.TrackState(P), r.SmoothState(P)
            outs, states, recs = [], [], []
            for i, (joints, num_people) in enumerate(case["frames"]):
                want_recs = r.track_update(ts, joints, num_people, tcfg)
                want = r.smooth_update(st, joints, num_people, want_recs, scfg)
                got_recs, js, vel, flags = e.smooth_from_joints(joints, num_people)
                assert np.array_equal(got_recs, want_recs), f"{case['name']} frame {i}: records\n{got_recs}\nthe host definition's\n{want_recs}"
                diff = sr.same_out(want, (js, vel, flags))
                assert diff is None, f"{case['name']} frame {i}: {diff}"
                got_state = e.smooth_state()
                assert got_state == st, f"{case['name']} frame {i}: the filter table differs: {sr.same_state(sc.as_ref(st), got_state)}"
                assert e.track_state() == ts, f"{case['name']} frame {i}: the track table differs"
                outs.append((js, vel, flags))
                states.append(sc.as_ref(got_state))
                recs.append(got_recs.astype(np.int64))
            sc.check_predicates(case, outs, states, recs)
    finally:
        e.close()


def test_state_round_trip():
    import caffe_rtpose_amd as r
    e = _engine(frames_in_flight=1, batch_frames=1)
    try:
        e.set_tracking()
        e.set_smoothing()
        rng = np.random.default_rng(3)
        st = r.SmoothState(18)
        st.frames = 0xFFFFFFF0
        st.cell.view(np.uint32).reshape(-1)[:] = rng.integers(0, 1 << 32, 128 * 70 * 7, dtype=np.uint64).astype(np.uint32)   # any bits, NaNs included
        assert np.isnan(st.cell["pos"]).any()
        e.set_smooth_state(st)
        assert e.smooth_state() == st
        ts = e.track_state()
        e.smooth_reset()
        assert e.smooth_state() == r.SmoothState(18) and e.track_state() == ts
        # the tracker's reset and state entries leave the filter table alone
        e.set_smooth_state(st)
        e.track_reset()
        e.set_track_state(r.TrackState(18))
        assert e.smooth_state() == st
    finally:
        e.close()


def _frames(order="AABAABBA", seed=41):
    import caffe_rtpose_amd as r
    content = {"A": r.synth_frame(160, 96, 0, seed=seed), "B": r.synth_frame(640, 360, 1, seed=seed)}   # B goes through the warp
    return [content[c] for c in order]


def _stream(e, frames, depth, smooth=True, collect=None, tag0=70, extra=None):
    """submit as many frames as fit before each collect; per frame peek_tracks, peek_smoothed (twice), extra() and collect
    -> [dict(recs, js, vel, flags, extra, col)]"""
    out, nxt = [], 0
    while nxt < len(frames) or e.in_flight():
        while nxt < len(frames) and e.in_flight() < depth:
            e.submit_frame(frames[nxt], tag=tag0 + nxt)
            nxt += 1
        d = dict(recs=e.peek_tracks()[1])
        if smooth:
            t1, d["js"], d["vel"], d["flags"] = e.peek_smoothed()
            t2, js2, vel2, flags2 = e.peek_smoothed()
            assert t1 == t2 == tag0 + len(out) and sr.same_out((d["js"], d["vel"], d["flags"]), (js2, vel2, flags2)) is None, "peeking twice gives the same"
        d["extra"] = extra() if extra else None
        d["col"] = (collect or e.collect)()
        assert d["col"][0] == tag0 + len(out)
        out.append(d)
    return out


def _replay(results, tcfg, scfg, P=18, ts=None, st=None):
    """rtp_track_update and rtp_smooth_update over the collected raw joints in submit order -> (records, outputs) per frame, states"""
    import caffe_rtpose_amd as r
    ts, st = ts or r.TrackState(P), st or r.SmoothState(P)
    want = []
    for d in results:
        n, joints = d["col"][1], d["col"][2]
        recs = r.track_update(ts, joints[:n], cfg=tcfg)
        want.append((recs, r.smooth_update(st, joints[:n], None, recs, scfg)))
    return want, ts, st


def _check_replay(res, want, what):
    for i, (d, (recs, out)) in enumerate(zip(res, want)):
        assert np.array_equal(d["recs"], recs), f"{what} frame {i}: records"
        diff = sr.same_out(out, (d["js"], d["vel"], d["flags"]))
        assert diff is None, f"{what} frame {i}: {diff}"


def _same_collects(a, b):
    return all(x["col"][1] == y["col"][1] and all(np.array_equal(np.asarray(p).view(np.uint8), np.asarray(q).view(np.uint8)) for p, q in zip(x["col"][2:], y["col"][2:]))
               for x, y in zip(a, b)) and len(a) == len(b)


PIPELINES = [(4, 2), (6, 1), (2, 2)]


@pytest.mark.parametrize("mode", ["graph", "eager"])
@pytest.mark.parametrize("pipe", PIPELINES, ids=lambda p: "inflight%d_batch%d" % p)
def test_async_path_updates_both_tables_in_submit_order(mode, pipe):
    """What this test shows: the smoothed people, records, both tables and the tags of frames that ran on different streams and
    contexts equal a replay in submit order, and rtp_collect's joints are the raw ones.  Like tests/test_track.py it does NOT show
    that the wait in front of each frame's track kernel is needed: that the event is recorded behind the smooth kernel and waited for
    by the next frame rests on reading engine_track.cpp and engine_smooth.cpp."""
    import caffe_rtpose_amd as r
    depth, batch = pipe
    e = _engine(frames_in_flight=depth, batch_frames=batch, exec_mode=r.EXEC_GRAPH if mode == "graph" else r.EXEC_EAGER)
    frames = _frames()
    flags_seen = {}
    try:
        for kw in (dict(), dict(max_hold=0, beta=0.3)):
            tcfg, scfg = r.track_config(), r.smooth_config(**kw)
            e.set_tracking(None)
            e.set_tracking(tcfg)       # (an empty table)
            raw = _stream(e, frames, depth, smooth=False)
            _modes(e, tcfg, scfg)
            res = _stream(e, frames, depth)
            assert _same_collects(raw, res), "rtp_collect's joints stay the raw ones"
            assert all(np.array_equal(a["recs"], b["recs"]) for a, b in zip(raw, res)), "the records do not depend on smoothing"
            want, ts, st = _replay(res, tcfg, scfg)
            _check_replay(res, want, f"{mode} {pipe} {kw}")
            assert e.smooth_state() == st and e.track_state() == ts, f"{mode} {pipe} {kw}: the final tables differ from the replay's"
            assert st.frames == len(frames)
            for d in res:
                for v, c in zip(*np.unique(d["flags"], return_counts=True)):
                    flags_seen[int(v)] = flags_seen.get(int(v), 0) + int(c)
            e.set_smoothing(None)
        print(mode, pipe, "flags seen:", flags_seen)
        # so that the test cannot pass vacuously: the repeated frame's people are filtered, new people start
        assert flags_seen.get(2, 0) >= 1 and flags_seen.get(1, 0) >= 1
    finally:
        e.close()


def _perturbed(st, dx):
    """the filter table with every live cell's position moved by dx pixels: the next frame's filtered people are visibly not the raw ones"""
    out = st.copy()
    live = out.cell["last"] != 0
    out.cell["pos"][live] += np.float32(dx)
    return out


def test_apply_flags_render_and_crop_the_smoothed_people():
    import caffe_rtpose_amd as r
    e = _engine(render=1)
    frames = _frames("AAB", seed=43)
    tcfg = r.track_config()
    crop = dict(crop_w=32, crop_h=48, max_crops=8, margin=0.25)
    try:
        e.set_crops_output(crop["crop_w"], crop["crop_h"], crop["max_crops"], margin=crop["margin"])
        e.set_tracking(tcfg)
        disps = [e.debug_preprocess(f)[1] for f in frames]

        def run(apply):
            """frame 0, then every live cell moved by 6 pixels, then the rest; apply None = tracking alone"""
            e.set_smoothing(None)
            e.track_reset()
            scfg = r.smooth_config(apply=apply) if apply is not None else None
            if scfg is not None:
                e.set_smoothing(scfg)
            kw = dict(smooth=scfg is not None, collect=e.collect_rendered, extra=lambda: e.peek_crops()[1:])
            first = _stream(e, frames[:1], 4, **kw)
            if scfg is not None:
                st0 = e.smooth_state()
                assert (st0.cell["last"] != 0).any(), "frame 0 needs a tracked person"
                e.set_smooth_state(_perturbed(st0, 6.0))
            return first + _stream(e, frames[1:], 4, tag0=71, **kw), scfg
        alone, _ = run(None)
        plain, scfg0 = run(0)
        assert _same_collects(alone, plain), "apply 0: the rendered frames are the tracking-only run's"
        assert all(np.array_equal(a["extra"][0].view(np.uint32), b["extra"][0].view(np.uint32)) and np.array_equal(a["extra"][1], b["extra"][1]) for a, b in zip(alone, plain)), \
            "apply 0: boxes and crops are the tracking-only run's"
        moved = any(not np.array_equal(d["js"].view(np.uint32), d["col"][2].view(np.uint32)) for d in plain)
        assert moved, "some frame's smoothed people must differ from the raw ones"
        for apply in (r.SMOOTH_RENDER, r.SMOOTH_CROPS, r.SMOOTH_RENDER | r.SMOOTH_CROPS):
            res, scfg = run(apply)
            assert sr.same_out((plain[1]["js"], plain[1]["vel"], plain[1]["flags"]), (res[1]["js"], res[1]["vel"], res[1]["flags"])) is None
            differs = {"render": 0, "crops": 0}
            for i, (d, disp, base) in enumerate(zip(res, disps, alone)):
                n = d["col"][1]
                assert np.array_equal(d["col"][2].view(np.uint32), base["col"][2].view(np.uint32)), "the collected joints stay raw"
                poses = d["js"] if apply & r.SMOOTH_RENDER else d["col"][2]
                assert np.array_equal(d["col"][3], e.render(disp, poses[:n], n)), f"apply {apply} frame {i}: the rendered frame"
                differs["render"] += int(not np.array_equal(d["col"][3], base["col"][3]))
                poses = d["js"] if apply & r.SMOOTH_CROPS else d["col"][2]
                boxes, crops = r.crop_people(disp, poses[:n], 18, crop["crop_w"], crop["crop_h"], crop["max_crops"], margin=crop["margin"])
                assert np.array_equal(d["extra"][0].view(np.uint32), boxes.view(np.uint32)), f"apply {apply} frame {i}: the boxes"
                assert np.array_equal(d["extra"][1], crops), f"apply {apply} frame {i}: the crops"
                differs["crops"] += int(not np.array_equal(d["extra"][0].view(np.uint32), base["extra"][0].view(np.uint32)))
            assert (differs["render"] >= 1) == bool(apply & r.SMOOTH_RENDER) and (differs["crops"] >= 1) == bool(apply & r.SMOOTH_CROPS), (apply, differs)
    finally:
        e.close()


def test_off_changes_nothing_and_composes_with_the_other_modes():
    import caffe_rtpose_amd as r
    e = _engine(render=1)
    frames = _frames("ABBA", seed=43)
    tcfg, scfg = r.track_config(), r.smooth_config(apply=r.SMOOTH_RENDER | r.SMOOTH_CROPS)
    try:
        off = _stream_plain(e, frames, e.collect_rendered)
        e.set_tracking(tcfg)
        tracked = _stream(e, frames, 4, smooth=False, collect=e.collect_rendered)
        # maps mode, crops mode and the YUV / JPEG forms of the rendered frame next to smoothing
        e.set_smoothing(scfg)
        e.set_maps_output("net", "u8", [0, 18])
        e.set_crops_output(64, 64, 16, margin=0.15)
        def collect_yuv():
            t, j, y, u, v = e.collect_rendered_yuv()
            return t, len(j), j, y, u, v
        for form, collect in (("raw", e.collect_rendered), ("yuv", collect_yuv), ("jpeg", e.collect_rendered_jpeg)):
            e.set_smoothing(None)
            e.track_reset()
            e.set_smoothing(scfg)
            if form == "yuv":
                e.set_render_yuv(420)
            if form == "jpeg":
                e.set_render_yuv(0)
                e.set_render_jpeg(90)
            res = _stream(e, frames, 4, collect=collect, extra=lambda: (e.peek_crops()[1], e.peek_maps()))
            want, ts, st = _replay(res, tcfg, scfg)
            _check_replay(res, want, form)
            assert e.smooth_state() == st and e.track_state() == ts
            for d, base in zip(res, tracked):
                n = d["col"][1]
                assert n == base["col"][1] and np.array_equal(d["col"][2].view(np.uint32), base["col"][2].view(np.uint32)), f"{form}: the collected joints"
                boxes, _ = r.crop_people(None, d["js"][:n], 18, 64, 64, 16, margin=0.15, pixels=False)
                assert np.array_equal(boxes.view(np.uint32), d["extra"][0].view(np.uint32)), f"{form}: crops slot k is smoothed person k"
        e.set_render_jpeg(0)
        # smoothing off after on: the tracking-only outputs; everything off: the engine is what it was
        e.set_smoothing(None)
        e.set_crops_output(None)
        e.set_maps_output(None)
        e.track_reset()
        again = _stream(e, frames, 4, smooth=False, collect=e.collect_rendered)
        assert _same_collects(tracked, again) and all(np.array_equal(a["recs"], b["recs"]) for a, b in zip(tracked, again))
        e.set_tracking(None)
        assert _same_collects(off, _stream_plain(e, frames, e.collect_rendered))
    finally:
        e.close()


def _stream_plain(e, frames, collect, depth=4, tag0=70):
    out, nxt = [], 0
    while nxt < len(frames) or e.in_flight():
        while nxt < len(frames) and e.in_flight() < depth:
            e.submit_frame(frames[nxt], tag=tag0 + nxt)
            nxt += 1
        out.append(dict(col=collect()))
    return out


def test_synchronous_taps_do_not_advance_the_filter():
    e = _engine()
    try:
        e.set_tracking()
        e.set_smoothing()
        f = _frames("A")[0]
        x, _, _ = e.debug_preprocess(f)
        e.forward_debug(x)
        e.track_from_joints(sc.body(18, 40, 20)[None])     # the tracker's own tap advances the tracker alone
        assert e.smooth_state().frames == 0 and e.track_state().frames == 1 and not e.smooth_state().cell["last"].any()
        e.submit(x, tag=1)          # a net input is a submitted frame like any other
        _, js, _, flags = e.peek_smoothed()
        _, n, joints = e.collect()
        assert len(js) == n and e.smooth_state().frames == 1 and e.track_state().frames == 2
    finally:
        e.close()


def test_refusals_and_lifecycle():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    e = _engine()
    frames = _frames("AB", seed=45)
    ubp = C.POINTER(C.c_ubyte)
    one = np.zeros((1, 18, 3), np.float32)
    try:
        # tracking off: no smoothing
        with pytest.raises(r.RtpError) as ex:
            e.set_smoothing()
        assert ex.value.code == r.RTP_EINVAL and "tracking" in str(ex.value)
        e.set_smoothing(None)        # off while off is fine
        tcfg = r.track_config(min_parts=2)
        e.set_tracking(tcfg)
        for call in (e.peek_smoothed, e.smooth_reset, e.smooth_state, lambda: e.set_smooth_state(r.SmoothState(18)), lambda: e.smooth_from_joints(one)):
            with pytest.raises(r.RtpError) as ex:
                call()
            assert ex.value.code == r.RTP_EINVAL and "off" in str(ex.value)
        for kw in (dict(min_cutoff=0.0), dict(min_cutoff=float("nan")), dict(beta=-1.0), dict(beta=float("inf")), dict(d_cutoff=0.0), dict(d_cutoff=float("inf")),
                   dict(max_hold=-1), dict(max_hold=1001), dict(min_score=-1.0), dict(apply=8)):
            with pytest.raises(r.RtpError) as ex:
                e.set_smoothing(r.smooth_config(**kw))
            assert ex.value.code == r.RTP_EINVAL, kw
        bad = r.smooth_config()
        bad.struct_size += 4
        with pytest.raises(r.RtpError):
            e.set_smoothing(bad)
        with pytest.raises(r.RtpError):
            e.peek_smoothed()          # still off
        scfg = r.smooth_config(max_hold=3)
        e.set_smoothing(scfg)
        with pytest.raises(r.RtpError) as ex:
            e.peek_smoothed()
        assert ex.value.code == r.RTP_EAGAIN   # nothing in flight
        # the tracker cannot go while the filter needs it; a new tracking configuration is fine
        with pytest.raises(r.RtpError) as ex:
            e.set_tracking(None)
        assert ex.value.code == r.RTP_EINVAL and "smoothing" in str(ex.value)
        e.set_tracking(tcfg)
        with pytest.raises(r.RtpError) as ex:
            e.set_smooth_state(r.SmoothState(15))
        assert ex.value.code == r.RTP_EINVAL and "parts" in str(ex.value)
        wrong = r.SmoothState(18)
        wrong.c.struct_size = 12
        with pytest.raises(r.RtpError):
            e.set_smooth_state(wrong)
        # with a frame in flight: no switch, no reset, no state entry, no tap
        e.submit_frame(frames[0], tag=1)
        for call in (lambda: e.set_smoothing(None), lambda: e.set_smoothing(r.smooth_config()), e.smooth_reset, e.smooth_state, lambda: e.set_smooth_state(r.SmoothState(18)),
                     lambda: e.smooth_from_joints(one)):
            with pytest.raises(r.RtpError) as ex:
                call()
            assert ex.value.code == r.RTP_EAGAIN
        # capacity below n: RTP_ERANGE with *num_people = n, and the frame stays peekable
        tag, js, vel, flags = e.peek_smoothed()
        n = len(js)
        assert tag == 1 and n >= 1, "the frame needs a person"
        buf = np.full((n, 18, 3), 77, np.float32)
        got_n, t = C.c_int(-1), C.c_uint64()
        assert _lib.lib.rtp_peek_smoothed(e.h, C.byref(t), buf.ctypes.data_as(_lib.fp), None, None, C.byref(got_n), n - 1) == r.RTP_ERANGE
        assert got_n.value == n and (buf == 77).all()
        assert _lib.lib.rtp_peek_smoothed(e.h, C.byref(t), None, None, None, C.byref(got_n), n) == r.RTP_EINVAL
        assert _lib.lib.rtp_peek_smoothed(e.h, C.byref(t), buf.ctypes.data_as(_lib.fp), None, None, C.byref(got_n), n) == r.RTP_OK    # vel and flags may be NULL
        assert np.array_equal(buf.view(np.uint32), js.view(np.uint32))
        _, recs = e.peek_tracks()
        _, n1, j1 = e.collect()
        ts, st = r.TrackState(18), r.SmoothState(18)
        assert np.array_equal(recs, r.track_update(ts, j1[:n1], cfg=tcfg))
        assert sr.same_out(r.smooth_update(st, j1[:n1], None, recs, scfg), (js, vel, flags)) is None and e.smooth_state() == st
        # a new configuration while the mode is on keeps the state
        scfg0 = r.smooth_config(max_hold=0, beta=0.2)
        e.set_smoothing(scfg0)
        assert e.smooth_state() == st
        # the tap advances both states, and frames submitted next continue from them
        person = sc.body(18, 40, 20)[None]
        got = e.smooth_from_joints(person)
        want_recs = r.track_update(ts, person, cfg=tcfg)
        assert np.array_equal(got[0], want_recs) and sr.same_out(r.smooth_update(st, person, None, want_recs, scfg0), got[1:]) is None
        assert e.smooth_state() == st and e.track_state() == ts
        e.submit_frame(frames[1], tag=2)
        _, recs2 = e.peek_tracks()
        got2 = e.peek_smoothed()[1:]
        _, n2, j2 = e.collect()
        assert np.array_equal(recs2, r.track_update(ts, j2[:n2], cfg=tcfg)) and sr.same_out(r.smooth_update(st, j2[:n2], None, recs2, scfg0), got2) is None
        assert e.smooth_state() == st and st.frames == 3
        # a reset mid-stream, and off -> on: both start from an empty table
        for restart in (e.smooth_reset, lambda: (e.set_smoothing(None), e.set_smoothing(scfg0))):
            restart()
            assert e.smooth_state() == r.SmoothState(18)
        e.set_smoothing(None)
        e.set_smoothing(None)         # off twice is fine
        with pytest.raises(r.RtpError):
            e.smooth_state()
        e.set_tracking(None)          # and now the tracker may go
    finally:
        e.close()


def test_cli_smooth_equals_peek_smoothed(tmp_path):
    import caffe_rtpose_amd as r
    out = tmp_path / "json"
    out.mkdir()
    p = subprocess.run([BIN, "--video", "synthetic:320x180:6", "--model", "coco", "--net_resolution", "160x96", "--resolution", "160x96", "--write_json", str(out), "--track",
                        "--track_min_parts", "2", "--track_max_misses", "1", "--smooth", "--smooth_max_hold", "2", "--smooth_beta", "0.1", "--no_frame_drops", "--no_display",
                        "--num_gpu", "1"], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    files = sorted(glob.glob(str(out / "*.json")))
    assert len(files) == 6
    e = r.Engine(r.Config(net_w=NET_W, net_h=NET_H, disp_w=160, disp_h=96))   # the CLI's engine: its defaults
    people = 0
    try:
        e.set_tracking(r.track_config(min_parts=2, max_misses=1))
        e.set_smoothing(r.smooth_config(max_hold=2, beta=0.1, apply=r.SMOOTH_RENDER | r.SMOOTH_CROPS))
        for i, f in enumerate(files):
            scale = e.submit_frame(r.synth_frame(320, 180, i, seed=2), tag=i)
            _, recs = e.peek_tracks()
            tag, js, _, _ = e.peek_smoothed()
            assert tag == i and e.collect()[0] == i
            assert open(f, "rb").read() == r.format_json_tracked(js, 18, scale, recs), f"frame {i}"
            people += len(js)
    finally:
        e.close()
    assert people >= 1, "the frames need people"

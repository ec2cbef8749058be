"""Tracking mode on the GPU.  Every comparison is integer for integer and float bit for float bit against rtp_track_update (which
tests/test_track_cpu.py holds to the numpy restatement): the parity tap on every case sequence of tests/_trackcases.py for COCO and
MPI, the state round trip, the async path — where the table is carried from frame to frame across the engine's streams and
contexts — in graph and eager mode at three pipeline shapes against a replay in submit order, the other output modes next to it,
every refusal, the life cycle of the state, and rtpose.bin --track against peek_tracks."""
import ctypes as C
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import _trackcases as tc
import _trackref as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
NET_W, NET_H = 160, 96


def _engine(min_subset_cnt=2, **kw):
    import caffe_rtpose_amd as r
    kw = dict(dict(net_w=NET_W, net_h=NET_H, disp_w=160, disp_h=96, frames_in_flight=4, batch_frames=2), **kw)
    e = r.Engine(r.Config(**kw))
    t = e.get_thresholds()
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], min_subset_cnt, 0.05)   # keep more "people" of the noise maps
    return e


VARIANTS = {"argmin256": 0, "argmin1024": 1, "sort256": 2, "sort1024": 3}   # kernels.h RTP_TRACK_*: the assignment's form and the workgroup's size


def _variant(e, v):
    """the unexported switch between the kernel's four builds (idle engine) -> the previous one"""
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_track_variant
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    before = fn(e.h, v)
    assert before >= 0, before
    return before


def _same_recs(got, want):
    got, want = np.ascontiguousarray(got, np.int32), np.ascontiguousarray(want, np.int32)
    return got.shape == want.shape and np.array_equal(got, want)


def _dense_case(P):
    """every (track, person) pair is a candidate: 96 people a tenth of a pixel apart, twice (9216 candidates in the second frame, all
    but 96 of them refused by the walk / struck out by the rounds), then 96 more live tracks than people can match"""
    crowd = np.stack([tc.shifted(tc.body(P, 100, 100), 0.125 * (i % 12), 0.125 * (i // 12)) for i in range(96)]).astype(np.float32)
    return dict(name=f"dense_P{P}", P=P, cfg=dict(max_misses=3), frames=[(crowd, None), (crowd[::-1].copy(), None), (crowd[:40].copy(), None)],
                pred=lambda r, s: all(int(x) != 0 for x in r[1][:, 0]) and (r[1][:, 2] == 2).all() and (s[2].misses[:96] > 0).sum() == 56)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("model", ["coco", "mpi"])
def test_parity_tap_equals_the_host_definition_on_every_case(model, variant):
    import caffe_rtpose_amd as r
    P = 18 if model == "coco" else 15
    e = _engine(frames_in_flight=1, batch_frames=1, model=r.MODEL_COCO_18 if model == "coco" else r.MODEL_MPI_15)
    try:
        assert e.num_parts == P
        default = _variant(e, VARIANTS[variant])
        assert default == VARIANTS["sort1024"], "the variant the engine runs unless told otherwise (kernels.h)"
        for case in tc.cases(P) + [_dense_case(P)]:
            cfg = r.track_config(**case["cfg"])
            e.set_tracking(None)
            e.set_tracking(cfg)
            st = r.TrackState(P)
            recs, states = [], []
            for i, (joints, num_people) in enumerate(case["frames"]):
                want = r.track_update(st, joints, num_people, cfg)
                got = e.track_from_joints(joints, num_people)
                assert _same_recs(got, want), f"{case['name']} frame {i}: records\n{got}\nthe host definition's\n{want}"
                recs.append(got)
                states.append(e.track_state())
                assert states[-1] == st, f"{case['name']} frame {i}: the table differs: {tr.same_state(_as_ref(st), states[-1])}"
            tc.check_predicates(case, recs, states)
    finally:
        e.close()


def _as_ref(ts):
    s = tr.State(ts.num_parts)
    s.next_id, s.frames = ts.next_id, ts.frames
    s.id, s.hits, s.misses, s.joints = ts.id.copy(), ts.hits.copy(), ts.misses.copy(), ts.joints.copy()
    return s


def test_state_round_trip():
    import caffe_rtpose_amd as r
    e = _engine(frames_in_flight=1, batch_frames=1)
    try:
        e.set_tracking()
        rng = np.random.default_rng(3)
        st = r.TrackState(18)
        st.next_id, st.frames = 0xFFFFFFF0, 123456
        st.id[:] = rng.integers(0, 1 << 31, 128)
        st.id[::5] = 0
        st.hits[:] = rng.integers(0, 1000, 128)
        st.misses[:] = rng.integers(0, 16, 128)
        st.joints.reshape(-1).view(np.uint32)[:] = rng.integers(0, 1 << 32, 128 * 70 * 3, dtype=np.uint64).astype(np.uint32)   # any bits, NaNs included
        e.set_track_state(st)
        assert e.track_state() == st
        e.track_reset()
        assert e.track_state() == r.TrackState(18)
    finally:
        e.close()


def _frames(order="AABAABBA", seed=41):
    import caffe_rtpose_amd as r
    content = {"A": r.synth_frame(160, 96, 0, seed=seed), "B": r.synth_frame(640, 360, 1, seed=seed)}   # B goes through the warp
    return [content[c] for c in order]


def _stream(e, frames, depth, peek=True, collect=None, tag0=70):
    """submit as many frames as fit before each collect; per frame peek_tracks (twice) then collect -> [(records, (tag, n, joints, ..))]"""
    out, nxt = [], 0
    while nxt < len(frames) or e.in_flight():
        while nxt < len(frames) and e.in_flight() < depth:
            e.submit_frame(frames[nxt], tag=tag0 + nxt)
            nxt += 1
        recs = None
        if peek:
            t1, recs = e.peek_tracks()
            t2, again = e.peek_tracks()
            assert t1 == t2 and np.array_equal(recs, again), "peeking twice gives the same"
        col = (collect or e.collect)()
        assert col[0] == tag0 + len(out) and (not peek or t1 == col[0])
        out.append((recs, col))
    return out


def _replay(results, cfg, P=18):
    """rtp_track_update over the collected joints in submit order -> (records per frame, final state, states)"""
    import caffe_rtpose_amd as r
    st = r.TrackState(P)
    want, live = [], []
    for _, col in results:
        want.append(r.track_update(st, col[2][:col[1]], cfg=cfg))
        live.append(set(st.live().values()))
    return want, st, live


PIPELINES = [(4, 2), (6, 1), (2, 2)]


@pytest.mark.parametrize("mode", ["graph", "eager"])
@pytest.mark.parametrize("pipe", PIPELINES, ids=lambda p: "inflight%d_batch%d" % p)
def test_async_path_updates_the_table_in_submit_order(mode, pipe):
    """What this test shows: records, table and tags of frames that ran on different streams and contexts equal a replay in submit
    order.  What it does NOT show: that the hipStreamWaitEvent in front of each track kernel is needed.  The chains are launched in
    submit order and each takes far longer than the track kernel, so a build without the wait would very likely pass too; that the
    wait, the event record and the launch order are right rests on reading engine_track.cpp track_launch."""
    import caffe_rtpose_amd as r
    depth, batch = pipe
    e = _engine(frames_in_flight=depth, batch_frames=batch, exec_mode=r.EXEC_GRAPH if mode == "graph" else r.EXEC_EAGER)
    frames = _frames()
    seen_hits2 = births_later = deaths = 0
    try:
        for kw in (dict(), dict(max_misses=0)):
            cfg = r.track_config(**kw)
            e.set_tracking(None)
            e.set_tracking(cfg)
            res = _stream(e, frames, depth)
            want, st, live = _replay(res, cfg)
            print(mode, pipe, kw, "people per frame:", [c[1] for _, c in res], "tracked:", [int((rc[:, 0] != 0).sum()) for rc, _ in res],
                  "matched:", [int((rc[:, 2] >= 2).sum()) for rc, _ in res], "live tracks:", [len(x) for x in live])
            for i, ((got, _), w) in enumerate(zip(res, want)):
                assert _same_recs(got, w), f"{mode} {pipe} {kw} frame {i}: records\n{got}\nthe replay's\n{w}"
            assert e.track_state() == st, f"{mode} {pipe} {kw}: the final table differs from the replay's: {tr.same_state(_as_ref(st), e.track_state())}"
            seen_hits2 += sum(int((rc[:, 2] >= 2).sum()) for rc, _ in res)
            births_later += sum(int((rc[:, 2] == 1).sum()) for rc, _ in res[1:])
            deaths += sum(len(a - b) for a, b in zip(live, live[1:]))
        # so that the test cannot pass vacuously
        assert seen_hits2 >= 1, "no record with hits >= 2: the repeated frame must match its own people"
        assert births_later >= 1, "no birth after frame 0"
        assert deaths >= 1, "no track died"
    finally:
        e.close()


def test_off_changes_nothing_and_composes_with_the_other_modes():
    import caffe_rtpose_amd as r
    e = _engine(render=1)
    frames = _frames("ABBA", seed=43)
    cfg = r.track_config()
    try:
        off = _stream(e, frames, 4, peek=False, collect=e.collect_rendered)
        e.set_tracking(cfg)
        on = _stream(e, frames, 4, collect=e.collect_rendered)
        for a, b in zip(off, on):
            assert a[1][1] == b[1][1] and all(np.array_equal(x, y) for x, y in zip(a[1][2:], b[1][2:])), "joints or the rendered frame changed with tracking on"
        want, st, _ = _replay(on, cfg)
        assert all(_same_recs(g, w) for (g, _), w in zip(on, want)) and e.track_state() == st
        # maps mode and crops mode next to it: record k's person is crops slot k's
        e.set_maps_output("net", "u8", [0, 18])
        e.set_crops_output(64, 64, 16, margin=0.15)
        e.track_reset()
        boxes = []

        def collect():
            boxes.append(e.peek_crops()[1])
            e.peek_maps()
            return e.collect_rendered()
        both = _stream(e, frames, 4, collect=collect)
        for a, (recs, col), bx in zip(off, both, boxes):
            assert a[1][1] == col[1] and all(np.array_equal(x, y) for x, y in zip(a[1][2:], col[2:]))
            assert len(recs) == col[1] and len(bx) == min(col[1], 16)
            host_boxes, _ = r.crop_people(None, col[2][:col[1]], 18, 64, 64, 16, margin=0.15, pixels=False)
            assert np.array_equal(host_boxes.view(np.uint32), bx.view(np.uint32)), "crops slot k is person k"
        want2, st2, _ = _replay(both, cfg)
        assert all(_same_recs(g, w) for (g, _), w in zip(both, want2)) and e.track_state() == st2 and st2 == st
        assert sum(len(rc) for rc, _ in both) >= 1
        # off again: the engine is what it was
        e.set_tracking(None)
        e.set_crops_output(None)
        e.set_maps_output(None)
        again = _stream(e, frames, 4, peek=False, collect=e.collect_rendered)
        assert all(a[1][1] == b[1][1] and all(np.array_equal(x, y) for x, y in zip(a[1][2:], b[1][2:])) for a, b in zip(off, again))
    finally:
        e.close()


def test_synchronous_taps_do_not_advance_the_tracker():
    e = _engine()
    try:
        e.set_tracking()
        f = _frames("A")[0]
        x, _, _ = e.debug_preprocess(f)
        e.forward_debug(x)
        assert e.track_state().frames == 0 and not e.track_state().id.any()
        e.submit(x, tag=1)          # a net input is a submitted frame like any other
        _, recs = e.peek_tracks()
        _, n, joints = e.collect()
        assert len(recs) == n and e.track_state().frames == 1
    finally:
        e.close()


def test_refusals_and_lifecycle():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    e = _engine()
    frames = _frames("AB", seed=45)
    try:
        for call in (e.peek_tracks, e.track_reset, e.track_state, lambda: e.set_track_state(r.TrackState(18)), lambda: e.track_from_joints(np.zeros((1, 18, 3), np.float32))):
            with pytest.raises(r.RtpError) as ex:
                call()
            assert ex.value.code == r.RTP_EINVAL and "off" in str(ex.value)
        for kw in (dict(max_cost=0.0), dict(min_parts=0), dict(min_common=0), dict(max_misses=-1), dict(min_score=-1.0), dict(max_cost=float("nan"))):
            with pytest.raises(r.RtpError) as ex:
                e.set_tracking(r.track_config(**kw))
            assert ex.value.code == r.RTP_EINVAL, kw
        bad = r.track_config()
        bad.struct_size += 4
        with pytest.raises(r.RtpError):
            e.set_tracking(bad)
        with pytest.raises(r.RtpError):
            e.peek_tracks()          # still off
        cfg = r.track_config(min_parts=2)
        e.set_tracking(cfg)
        with pytest.raises(r.RtpError) as ex:
            e.peek_tracks()
        assert ex.value.code == r.RTP_EAGAIN   # nothing in flight
        with pytest.raises(r.RtpError) as ex:
            e.set_track_state(r.TrackState(15))
        assert ex.value.code == r.RTP_EINVAL and "parts" in str(ex.value)
        wrong = r.TrackState(18)
        wrong.c.struct_size = 12
        with pytest.raises(r.RtpError):
            e.set_track_state(wrong)
        # with a frame in flight: no switch, no reset, no state entry, no tap
        e.submit_frame(frames[0], tag=1)
        for call in (lambda: e.set_tracking(None), lambda: e.set_tracking(r.track_config()), e.track_reset, e.track_state, lambda: e.set_track_state(r.TrackState(18)),
                     lambda: e.track_from_joints(np.zeros((1, 18, 3), np.float32))):
            with pytest.raises(r.RtpError) as ex:
                call()
            assert ex.value.code == r.RTP_EAGAIN
        # capacity below n: RTP_ERANGE with *num_recs = n, and the frame stays peekable
        tag, recs = e.peek_tracks()
        n = len(recs)
        assert tag == 1 and n >= 1, "the frame needs a person"
        buf = np.full((n, 4), 77, np.int32)
        got_n, t = C.c_int(-1), C.c_uint64()
        assert _lib.lib.rtp_peek_tracks(e.h, C.byref(t), buf.ctypes.data_as(_lib.ip), C.byref(got_n), n - 1) == r.RTP_ERANGE
        assert got_n.value == n and (buf == 77).all()
        assert _lib.lib.rtp_peek_tracks(e.h, C.byref(t), None, C.byref(got_n), n) == r.RTP_EINVAL
        assert np.array_equal(e.peek_tracks()[1], recs)
        _, n1, j1 = e.collect()
        st = r.TrackState(18)
        assert _same_recs(recs, r.track_update(st, j1[:n1], cfg=cfg)) and e.track_state() == st
        first_ids = sorted(int(x) for x in recs[:, 0] if x)
        assert first_ids and first_ids[0] == 1
        # a new configuration while the mode is on keeps the state
        cfg0 = r.track_config(min_parts=2, max_misses=0)
        e.set_tracking(cfg0)
        assert e.track_state() == st
        # the tap advances the engine's state, and frames submitted next continue from it
        person = tc.body(18, 40, 20)[None]
        got = e.track_from_joints(person)
        assert _same_recs(got, r.track_update(st, person, cfg=cfg0)) and e.track_state() == st
        e.submit_frame(frames[1], tag=2)
        _, recs2 = e.peek_tracks()
        _, n2, j2 = e.collect()
        assert _same_recs(recs2, r.track_update(st, j2[:n2], cfg=cfg0)) and e.track_state() == st and st.frames == 3
        # a reset mid-stream, and off -> on: both start at id 1
        for restart in (e.track_reset, lambda: (e.set_tracking(None), e.set_tracking(cfg))):
            restart()
            assert e.track_state() == r.TrackState(18)
            e.submit_frame(frames[0], tag=3)
            _, recs3 = e.peek_tracks()
            e.collect()
            assert np.array_equal(recs3, recs), "the same frame on an empty table gets the same records, from id 1"
        e.set_tracking(None)
        e.set_tracking(None)         # off twice is fine
        with pytest.raises(r.RtpError):
            e.track_state()
    finally:
        e.close()


def test_cli_track_equals_peek_tracks(tmp_path):
    import caffe_rtpose_amd as r
    out = tmp_path / "json"
    out.mkdir()
    p = subprocess.run([BIN, "--video", "synthetic:320x180:6", "--model", "coco", "--net_resolution", "160x96", "--resolution", "160x96", "--write_json", str(out), "--track",
                        "--track_min_parts", "2", "--track_max_misses", "1", "--no_frame_drops", "--no_display", "--num_gpu", "1"], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    files = sorted(glob.glob(str(out / "*.json")))
    assert len(files) == 6
    e = r.Engine(r.Config(net_w=NET_W, net_h=NET_H, disp_w=160, disp_h=96))   # the CLI's engine: its defaults
    total = 0
    try:
        e.set_tracking(r.track_config(min_parts=2, max_misses=1))
        for i, f in enumerate(files):
            e.submit_frame(r.synth_frame(320, 180, i, seed=2), tag=i)
            tag, recs = e.peek_tracks()
            assert tag == i and e.collect()[0] == i
            bodies = json.load(open(f))["bodies"]
            assert [b["id"] for b in bodies] == [int(x) for x in recs[:, 0]], f"frame {i}"
            total += int((recs[:, 0] != 0).sum())
    finally:
        e.close()
    assert total >= 1, "somebody must be tracked"

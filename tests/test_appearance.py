"""Appearance-aided tracking on the GPU.  Every comparison is integer for integer and float bit for float bit against
rtp_appearance_describe and rtp_track_update_appearance (which tests/test_appearance_cpu.py holds to the numpy restatement): the
describe tap on every describe case, the track tap in all four kernel forms for COCO and MPI on every update case, the crossing and a
dense case, the async path in graph and eager mode at three pipeline shapes against a replay in submit order, the other output modes
next to it, frames without a display image, and the life cycle of the mode and its table."""
import ctypes as C

import numpy as np
import pytest

import _appearcases as ac
import _appearref as ar
import _trackcases as tc

pytestmark = pytest.mark.gpu

NET_W, NET_H = 160, 96
VARIANTS = {"argmin256": 0, "argmin1024": 1, "sort256": 2, "sort1024": 3}   # kernels.h RTP_TRACK_*
PIPELINES = [(4, 2), (6, 1), (2, 2)]
ALL_PARTS = dict(parts=list(range(18)), min_parts=2)   # the "people" of the noise maps rarely have three torso parts


def _engine(min_subset_cnt=2, **kw):
    import caffe_rtpose_amd as r
    kw = dict(dict(net_w=NET_W, net_h=NET_H, disp_w=ac.W, disp_h=ac.H, frames_in_flight=4, batch_frames=2), **kw)
    e = r.Engine(r.Config(**kw))
    t = e.get_thresholds()
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], min_subset_cnt, 0.05)   # keep more "people" of the noise maps
    return e


def _variant(e, v):
    from caffe_rtpose_amd import _lib
    fn = _lib.lib.rtp_internal_track_variant
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    before = fn(e.h, v)
    assert before >= 0, before
    return before


def _same(got, want, what):
    for g, w, name in zip(got, want, ("records", "bins", "valid")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), f"{what}: {name}\n{g}\nthe host definition's\n{w}"


def test_describe_tap_equals_the_host_definition():
    """every describe case whose image has the engine's display size, then 96, 0, -1 and 200 people; the cases with an image of another
    size run on engines of their own below"""
    import caffe_rtpose_amd as r
    e = _engine(frames_in_flight=1, batch_frames=1)
    try:
        e.set_tracking()
        ran = 0
        for case in ac.describe_cases(18):
            if case["image"].shape != (ac.H, ac.W, 3):
                continue
            cfg = r.appearance_config(**case["cfg"])
            e.set_track_appearance(cfg)
            got = e.appearance_from_joints(case["image"], case["joints"])
            _same(got, r.appearance_describe(case["image"], case["joints"], 18, cfg), case["name"])
            assert case["pred"](*got), case["name"]
            ran += 1
        assert ran >= 15
        rng = np.random.default_rng(11)
        img = rng.integers(0, 256, (ac.H, ac.W, 3), dtype=np.uint8)
        crowd = np.stack([tc.body(18, rng.uniform(-20, ac.W), rng.uniform(-20, ac.H), w=4.0 * rng.integers(1, 12), h=4.0 * rng.integers(1, 12)) for _ in range(96)])
        cfg = r.appearance_config(margin=0.25)
        e.set_track_appearance(cfg)
        want = r.appearance_describe(img, crowd, 18, cfg)
        assert want[1].all()
        _same(e.appearance_from_joints(img, crowd), want, "96 people")
        _same(e.appearance_from_joints(img, crowd, 200), want, "num_people 200 counts as 96")
        for people in (0, -1):
            b, v = e.appearance_from_joints(img, crowd, people)
            assert b.shape == (0, 128) and v.shape == (0,), people
        b, v = e.appearance_from_joints(None, crowd)
        assert b.shape == (96, 128) and not b.any() and not v.any(), "no display image: nobody has a descriptor"
        assert e.appearance_state() == r.AppearanceState() and e.track_state() == r.TrackState(18), "the describe tap touches no table"
    finally:
        e.close()


def test_describe_tap_on_the_cases_of_another_image_size():
    """the describe cases whose image is not 160 x 96 (the image of one pixel), each on an engine with that display"""
    import caffe_rtpose_amd as r
    cases = [c for c in ac.describe_cases(18) if c["image"].shape != (ac.H, ac.W, 3)]
    assert any(c["image"].shape == (1, 1, 3) for c in cases)
    for case in cases:
        h, w = case["image"].shape[:2]
        e = _engine(frames_in_flight=1, batch_frames=1, disp_w=w, disp_h=h)
        try:
            e.set_tracking()
            cfg = r.appearance_config(**case["cfg"])
            e.set_track_appearance(cfg)
            got = e.appearance_from_joints(case["image"], case["joints"])
            _same(got, r.appearance_describe(case["image"], case["joints"], 18, cfg), case["name"])
            assert case["pred"](*got), case["name"]
        finally:
            e.close()


def test_describe_tap_at_an_odd_display_size_hits_the_clamp_at_both_edges():
    import caffe_rtpose_amd as r
    W, H = 97, 61
    e = _engine(frames_in_flight=1, batch_frames=1, disp_w=W, disp_h=H)
    try:
        e.set_tracking()
        rng = np.random.default_rng(12)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        people = np.stack([tc.body(18, -6, -8), tc.body(18, W - 6, H - 8), tc.body(18, -300, -300), tc.body(18, W + 300, H + 300), tc.body(18, W - 13, H - 17),
                           tc.body(18, 0, 0, w=160.0, h=96.0), tc.body(18, -40, -40, w=240.0, h=176.0)])
        for margin in (0.0, 0.5):
            cfg = r.appearance_config(margin=margin)
            e.set_track_appearance(cfg)
            want = r.appearance_describe(img, people, 18, cfg)
            assert want[1].all()
            _same(e.appearance_from_joints(img, people), want, f"margin {margin}")
        corner = np.zeros(128, np.int64)
        for half, (y, x) in ((0, (0, 0)), (64, (0, 0))):
            b_, g_, r_ = (int(v) for v in img[y, x])
            corner[half + (r_ >> 6) * 16 + (g_ >> 6) * 4 + (b_ >> 6)] += 512
        assert np.array_equal(want[0][2], corner), "wholly outside at the top left: 1024 samples of pixel (0, 0)"
    finally:
        e.close()


def _dense_case(P):
    """96 people a fraction of a pixel apart against 128 live tracks that all have descriptors: 96 births, then 32 more far away fill the
    table, then the 96 come back in another order over another image: each is a candidate of each of the 96 near tracks, 9216 pairs
    that pass the motion gate and take the 128-bin distance, all but 96 of them refused by the walk / struck out by the rounds."""
    def crowd(n, phase):
        return np.stack([tc.shifted(tc.body(P, 60, 40), 0.125 * ((i + phase) % 12), 0.125 * ((i + phase) // 12)) for i in range(n)]).astype(np.float32)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (ac.H, ac.W, 3), dtype=np.uint8)
    far = np.stack([tc.shifted(b, 4000, 0) for b in crowd(32, 0)])
    frames = [(crowd(96, 0), None, img), (far, None, img), (crowd(96, 5)[::-1].copy(), None, img[::-1].copy()), (crowd(40, 2), None, img)]
    return dict(name=f"dense_P{P}", P=P, cfg=dict(weight=0.5, rate=64), track=dict(max_misses=3), frames=frames,
                pred=lambda r, ts, ap, d: ts[1].id.all() and (ap[1].owner == ts[1].id).all() and d[2][1].all() and (r[2][:, 2] == 2).all()
                and len({int(x) for x in r[2][:, 3]}) > 1 and (r[3][:, 2] == 3).all() and (ts[3].misses[:96] > 0).sum() == 56)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("model", ["coco", "mpi"])
def test_track_tap_equals_the_host_definitions_on_every_case(model, variant):
    import caffe_rtpose_amd as r
    P = 18 if model == "coco" else 15
    e = _engine(frames_in_flight=1, batch_frames=1, model=r.MODEL_COCO_18 if model == "coco" else r.MODEL_MPI_15)
    try:
        assert e.num_parts == P
        assert _variant(e, VARIANTS[variant]) == VARIANTS["sort1024"]
        for case in ac.update_cases(P) + [_dense_case(P)]:
            tcfg, acfg = r.track_config(**case["track"]), r.appearance_config(**case["cfg"])
            e.set_track_appearance(None)
            e.set_tracking(None)
            e.set_tracking(tcfg)
            e.set_track_appearance(acfg)
            ts, ap = r.TrackState(P), r.AppearanceState()
            result = ([], [], [], [])
            for i, (joints, num_people, image) in enumerate(case["frames"]):
                b, v = r.appearance_describe(image, joints, P, acfg) if image is not None else (None, None)
                want = r.track_update_appearance(ts, ap, joints, num_people, b, v, tcfg, acfg)
                got = e.track_from_frame(image, joints, num_people)
                n = len(want)
                _same(got, (want, b if b is not None else np.zeros((n, 128), np.uint16), v if v is not None else np.zeros(n, np.uint8)), f"{case['name']} frame {i}")
                gts, gap = e.track_state(), e.appearance_state()
                assert gts == ts, f"{case['name']} frame {i}: the track table differs"
                assert gap == ap, f"{case['name']} frame {i}: the descriptor table differs: {ar.same_state(ap, gap)}"
                for lst, x in zip(result, (got[0], gts, gap, (b, v))):
                    lst.append(x)
            ac.check_predicates(case, *result)
    finally:
        e.close()


def _frames(order="AABAABBA", seed=41):
    import caffe_rtpose_amd as r
    content = {"A": r.synth_frame(160, 96, 0, seed=seed), "B": r.synth_frame(640, 360, 1, seed=seed)}   # B goes through the warp
    return [content[c] for c in order]


def _stream(e, frames, depth, peek=True, collect=None, tag0=70, net_input=()):
    """submit as many frames as fit before each collect; per frame peek_tracks and peek_appearance (twice each) then collect
    -> [(records, bins, valid, collect's result)].  net_input: the indices of the frames submitted without a display image"""
    out, nxt = [], 0
    pre = {i: e.debug_preprocess(frames[i])[0] for i in net_input}   # (a tap: the engine is still idle here)
    while nxt < len(frames) or e.in_flight():
        while nxt < len(frames) and e.in_flight() < depth:
            if nxt in net_input:
                e.submit(pre[nxt], tag=tag0 + nxt)
            else:
                e.submit_frame(frames[nxt], tag=tag0 + nxt)
            nxt += 1
        recs = b = v = None
        if peek:
            t1, recs = e.peek_tracks()
            t2, b, v = e.peek_appearance()
            t3, b2, v2 = e.peek_appearance()
            assert t1 == t2 == t3 and np.array_equal(b, b2) and np.array_equal(v, v2), "peeking twice gives the same"
        col = (collect or e.collect)()
        assert col[0] == tag0 + len(out) and (not peek or t1 == col[0])
        out.append((recs, b, v, col))
    return out


def _replay(e, frames, results, tcfg, acfg, net_input=()):
    """the two host definitions over the collected joints and the display images of debug_preprocess, in submit order (idle engine)"""
    import caffe_rtpose_amd as r
    ts, ap = r.TrackState(18), r.AppearanceState()
    want = []
    for i, (f, (_, _, _, col)) in enumerate(zip(frames, results)):
        joints = col[2][:col[1]]
        if i in net_input:
            b, v = None, None
        else:
            b, v = r.appearance_describe(e.debug_preprocess(f)[1], joints, 18, acfg)
        recs = r.track_update_appearance(ts, ap, joints, None, b, v, tcfg, acfg)
        n = len(recs)
        want.append((recs, b if b is not None else np.zeros((n, 128), np.uint16), v if v is not None else np.zeros(n, np.uint8)))
    return want, ts, ap


@pytest.mark.parametrize("mode", ["graph", "eager"])
@pytest.mark.parametrize("pipe", PIPELINES, ids=lambda p: "inflight%d_batch%d" % p)
def test_async_path_equals_a_replay_in_submit_order(mode, pipe):
    import caffe_rtpose_amd as r
    depth, batch = pipe
    e = _engine(frames_in_flight=depth, batch_frames=batch, exec_mode=r.EXEC_GRAPH if mode == "graph" else r.EXEC_EAGER)
    frames = _frames()
    try:
        tcfg, acfg = r.track_config(max_misses=0), r.appearance_config(weight=0.25, rate=64, **ALL_PARTS)
        plain = _stream(e, frames, depth, peek=False)
        e.set_tracking(tcfg)
        e.set_track_appearance(acfg)
        res = _stream(e, frames, depth)
        for a, b in zip(plain, res):
            assert a[3][1] == b[3][1] and np.array_equal(a[3][2], b[3][2]), "joints changed with the mode on"
        want, ts, ap = _replay(e, frames, res, tcfg, acfg)
        print(mode, pipe, "people per frame:", [c[1] for *_, c in res], "valid:", [int(v.sum()) for _, _, v, _ in res], "matched:", [int((rc[:, 2] >= 2).sum()) for rc, *_ in res])
        for i, (got, w) in enumerate(zip(res, want)):
            _same(got[:3], w, f"{mode} {pipe} frame {i}")
        assert e.track_state() == ts and e.appearance_state() == ap, f"{mode} {pipe}: a final table differs from the replay's: {ar.same_state(ap, e.appearance_state())}"
        # so that the test cannot pass vacuously
        assert sum(int(v.sum()) for _, _, v, _ in res) >= 2 and sum(int((rc[:, 2] >= 2).sum()) for rc, *_ in res) >= 1 and ap.owner.any()
    finally:
        e.close()


def test_frames_without_a_display_image_track_as_unknown():
    import caffe_rtpose_amd as r
    e = _engine()
    frames = _frames("AAAA", seed=41)
    try:
        tcfg, acfg = r.track_config(), r.appearance_config(weight=0.25, unknown=0.5, **ALL_PARTS)
        e.set_tracking(tcfg)
        e.set_track_appearance(acfg)
        res = _stream(e, frames, 4, net_input={1, 2})
        want, ts, ap = _replay(e, frames, res, tcfg, acfg, net_input={1, 2})
        for i, (got, w) in enumerate(zip(res, want)):
            _same(got[:3], w, f"frame {i}")
        assert e.track_state() == ts and e.appearance_state() == ap
        assert res[0][2].any() and not res[1][2].any() and not res[2][2].any() and res[3][2].any()
        matched = res[1][0][res[1][0][:, 2] >= 2]
        assert len(matched) >= 1 and (matched[:, 3].view(np.uint32) >= np.float32(0.125).view(np.uint32)).all(), "every match of a frame without an image carries weight * unknown"
    finally:
        e.close()


def test_next_to_the_other_modes():
    """Smoothing (RENDER | CROPS), overlay, crops and redaction on.  With the neutral configuration (weight 0, max_dist 1, unknown 0) the
    records are tracking mode's, so every byte the other modes hand out must be what it is with this mode off.  With a weight, records
    and descriptors equal the replay, and every other mode's output equals its own host definition on those records: the smoothed joints
    rtp_smooth_update's, and, from the smoothed joints (both apply flags are on), the draw list rtp_overlay_update's, the boxes and
    crops rtp_crop_people's on the un-rendered display image, and the redaction records rtp_redact_regions'."""
    import caffe_rtpose_amd as r
    e = _engine(render=1)
    frames = _frames("ABBA", seed=43)
    try:
        tcfg, scfg = r.track_config(), r.smooth_config(apply=r.SMOOTH_RENDER | r.SMOOTH_CROPS)
        e.set_tracking(tcfg)
        e.set_smoothing(scfg)
        e.set_track_overlay()
        e.set_crops_output(64, 64, 16, margin=0.15)
        e.set_redaction()
        extras = []

        def collect():
            extras.append((e.peek_smoothed()[1:], e.peek_overlay_items()[1], e.peek_crops()[1:], e.peek_redactions()[1]))
            return e.collect_rendered()

        def run(peek):
            extras.clear()
            e.track_reset()
            e.smooth_reset()
            e.overlay_reset()
            return _stream(e, frames, 4, peek=peek, collect=collect), list(extras)

        def flat(x):
            return [np.asarray(a) for a in (x if isinstance(x, (tuple, list)) else [x]) if a is not None]
        base, base_x = run(False)
        e.set_track_appearance(r.appearance_config(weight=0.0, max_dist=1.0, unknown=0.0, **ALL_PARTS))
        neutral, neutral_x = run(True)
        for i, (a, b, xa, xb) in enumerate(zip(base, neutral, base_x, neutral_x)):
            assert a[3][1] == b[3][1] and all(np.array_equal(x, y) for x, y in zip(a[3][2:], b[3][2:])), f"frame {i}: joints or the rendered frame"
            for ma, mb, name in zip(xa, xb, ("smoothed", "overlay items", "crops", "redactions")):
                fa, fb = flat(ma), flat(mb)
                assert len(fa) == len(fb) and all(np.array_equal(x, y) for x, y in zip(fa, fb)), f"frame {i}: {name} changed with the neutral mode on"
        acfg = r.appearance_config(weight=0.25, **ALL_PARTS)
        e.set_track_appearance(acfg)
        e.appearance_reset()
        on, on_x = run(True)
        want, ts, ap = _replay(e, frames, on, tcfg, acfg)
        sm, trail = r.SmoothState(18), r.TrailState(18)
        disps = [e.debug_preprocess(f)[1] for f in frames]
        for i, (got, w, x) in enumerate(zip(on, want, on_x)):
            _same(got[:3], w, f"frame {i}")
            js, vel, flags = r.smooth_update(sm, got[3][2][:got[3][1]], recs=got[0], cfg=scfg)
            assert np.array_equal(js.view(np.uint32), x[0][0].view(np.uint32)) and np.array_equal(flags, x[0][2]), f"frame {i}: the smoothed joints"
            assert np.array_equal(r.overlay_update(trail, js, recs=got[0]), x[1]), f"frame {i}: the draw list"
            boxes, crops = r.crop_people(disps[i], js, 18, 64, 64, 16, margin=0.15)
            assert np.array_equal(boxes.view(np.uint32), x[2][0].view(np.uint32)) and np.array_equal(crops, x[2][1]), f"frame {i}: boxes and crops"
            assert np.array_equal(r.redact_regions(js, 18), x[3]), f"frame {i}: the redaction records"
        assert e.track_state() == ts and e.appearance_state() == ap and sum(int(g[2].sum()) for g in on) >= 1
    finally:
        e.close()


def test_life_cycle_and_refusals():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    e = _engine()
    frames = _frames("AB", seed=45)
    one = np.zeros((1, 18, 3), np.float32)
    img = np.zeros((ac.H, ac.W, 3), np.uint8)
    try:
        with pytest.raises(r.RtpError) as ex:
            e.set_track_appearance()          # tracking mode is off
        assert ex.value.code == r.RTP_EINVAL and "tracking" in str(ex.value)
        e.set_track_appearance(None)          # off while off is fine
        tcfg = r.track_config(min_parts=2)
        e.set_tracking(tcfg)
        for call in (e.peek_appearance, e.appearance_reset, e.appearance_state, lambda: e.set_appearance_state(r.AppearanceState()), lambda: e.appearance_from_joints(img, one),
                     lambda: e.track_from_frame(img, one)):
            with pytest.raises(r.RtpError) as ex:
                call()
            assert ex.value.code == r.RTP_EINVAL and "off" in str(ex.value)
        for kw in (dict(weight=-1.0), dict(max_dist=0.0), dict(max_dist=2.0), dict(unknown=-0.5), dict(rate=0), dict(rate=257), dict(margin=17.0), dict(min_parts=0), dict(parts=[18]),
                   dict(weight=float("nan"))):
            with pytest.raises(r.RtpError) as ex:
                e.set_track_appearance(r.appearance_config(**kw))
            assert ex.value.code == r.RTP_EINVAL, kw
        bad = r.appearance_config()
        bad.struct_size += 4
        with pytest.raises(r.RtpError):
            e.set_track_appearance(bad)
        # mode off again is an engine that never had it
        e.submit_frame(frames[0], tag=1)
        _, alone = e.peek_tracks()
        e.collect()
        acfg = r.appearance_config(weight=0.25, **ALL_PARTS)
        e.set_track_appearance(acfg)
        with pytest.raises(r.RtpError) as ex:
            e.set_tracking(None)              # the mode needs the tracker
        assert ex.value.code == r.RTP_EINVAL and "appearance" in str(ex.value)
        with pytest.raises(r.RtpError) as ex:
            e.peek_appearance()
        assert ex.value.code == r.RTP_EAGAIN   # nothing in flight
        wrong = r.AppearanceState()
        wrong.c.struct_size = 12
        with pytest.raises(r.RtpError):
            e.set_appearance_state(wrong)
        # the state round trip, with arbitrary bits
        rng = np.random.default_rng(3)
        st = r.AppearanceState()
        st.owner[:] = rng.integers(-(1 << 31), 1 << 31, 128)
        st.desc[:] = rng.integers(0, 1 << 16, (128, 128))
        e.set_appearance_state(st)
        assert e.appearance_state() == st
        e.appearance_reset()
        assert e.appearance_state() == r.AppearanceState()
        # with a frame in flight: no switch, no reset, no state entry, no tap
        e.track_reset()
        e.submit_frame(frames[0], tag=2)
        for call in (lambda: e.set_track_appearance(None), lambda: e.set_track_appearance(acfg), e.appearance_reset, e.appearance_state, lambda: e.set_appearance_state(st),
                     lambda: e.appearance_from_joints(img, one), lambda: e.track_from_frame(img, one)):
            with pytest.raises(r.RtpError) as ex:
                call()
            assert ex.value.code == r.RTP_EAGAIN
        # capacity below n: RTP_ERANGE with *num = n, nothing written, and the frame stays peekable
        tag, bins, valid = e.peek_appearance()
        n = len(valid)
        assert tag == 2 and n >= 1, "the frame needs a person"
        bb, vb = np.full((n, 128), 77, np.uint16), np.full(n, 77, np.uint8)
        got_n, t = C.c_int(-1), C.c_uint64()
        u16p, u8p = C.POINTER(C.c_uint16), C.POINTER(C.c_ubyte)
        assert _lib.lib.rtp_peek_appearance(e.h, C.byref(t), bb.ctypes.data_as(u16p), vb.ctypes.data_as(u8p), C.byref(got_n), n - 1) == r.RTP_ERANGE
        assert got_n.value == n and (bb == 77).all() and (vb == 77).all()
        assert _lib.lib.rtp_peek_appearance(e.h, C.byref(t), None, vb.ctypes.data_as(u8p), C.byref(got_n), n) == r.RTP_EINVAL
        _, recs = e.peek_tracks()
        _, n1, j1 = e.collect()
        assert np.array_equal(recs, alone), "the first frame on empty tables: the records of tracking alone (every pair is a birth)"
        ts, ap = r.TrackState(18), r.AppearanceState()
        b, v = r.appearance_describe(e.debug_preprocess(frames[0])[1], j1[:n1], 18, acfg)
        assert np.array_equal(b, bins) and np.array_equal(v, valid)
        assert np.array_equal(recs, r.track_update_appearance(ts, ap, j1[:n1], None, b, v, tcfg, acfg)) and e.track_state() == ts and e.appearance_state() == ap
        # a new configuration while the mode is on keeps both tables; off -> on starts from an empty descriptor table and keeps the track table
        e.set_track_appearance(r.appearance_config(weight=0.5, **ALL_PARTS))
        assert e.appearance_state() == ap and e.track_state() == ts
        # the joints-only tap while the mode is on: a frame without a display image
        person = tc.body(18, 40, 20)[None]
        got = e.track_from_joints(person)
        assert np.array_equal(got, r.track_update_appearance(ts, ap, person, None, None, None, tcfg, r.appearance_config(weight=0.5, **ALL_PARTS)))
        assert e.track_state() == ts and e.appearance_state() == ap
        e.set_track_appearance(None)
        e.set_track_appearance(acfg)
        assert e.appearance_state() == r.AppearanceState() and e.track_state() == ts
        e.set_track_appearance(None)
        with pytest.raises(r.RtpError):
            e.appearance_state()
        # off again: records equal tracking alone
        e.track_reset()
        e.submit_frame(frames[0], tag=3)
        _, again = e.peek_tracks()
        e.collect()
        assert np.array_equal(again, alone)
        e.set_tracking(None)                  # and the tracker can be switched off again
    finally:
        e.close()


def test_cli_track_appearance_equals_peek_tracks(tmp_path):
    """rtpose.bin --track --track_appearance on one GPU worker runs the engine's mode: the ids of its JSON files are peek_tracks' of an
    engine with the same two configurations fed the same frames"""
    import glob
    import json
    import os
    import subprocess
    import caffe_rtpose_amd as r
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "json"
    out.mkdir()
    p = subprocess.run([os.path.join(root, "caffe_rtpose_amd", "rtpose.bin"), "--video", "synthetic:320x180:6", "--model", "coco", "--net_resolution", "160x96", "--resolution",
                        "160x96", "--write_json", str(out), "--track", "--track_min_parts", "2", "--track_max_misses", "1", "--track_max_cost", "4", "--track_appearance",
                        "--appearance_weight", "8", "--appearance_rate", "128", "--appearance_parts", "all", "--no_frame_drops", "--no_display", "--num_gpu", "1"],
                       capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    files = sorted(glob.glob(str(out / "*.json")))
    assert len(files) == 6
    e = r.Engine(r.Config(net_w=NET_W, net_h=NET_H, disp_w=160, disp_h=96))   # the CLI's engine: its defaults
    total = valid_total = 0
    try:
        e.set_tracking(r.track_config(min_parts=2, max_misses=1, max_cost=4.0))
        e.set_track_appearance(r.appearance_config(parts=list(range(18)), weight=8.0, rate=128))
        for i, f in enumerate(files):
            e.submit_frame(r.synth_frame(320, 180, i, seed=2), tag=i)
            tag, recs = e.peek_tracks()
            valid_total += int(e.peek_appearance()[2].sum())
            assert tag == i and e.collect()[0] == i
            bodies = json.load(open(f))["bodies"]
            assert [b["id"] for b in bodies] == [int(x) for x in recs[:, 0]], f"frame {i}"
            total += int((recs[:, 2] >= 2).sum())
    finally:
        e.close()
    assert total >= 1 and valid_total >= 1, "somebody must be matched, and somebody must have a descriptor"


def test_cli_two_workers_on_a_video_file_equal_the_host_replay(tmp_path):
    """rtpose.bin --video x.y4m --num_gpu 2 --track --track_appearance: two real workers (on one device), so the re-orderer runs the host
    definitions, and the producer hands BGR frames instead of the file's planes so that it can: the ids of the JSON files equal
    rtp_appearance_describe + rtp_track_update_appearance over the joints and display images an engine gives for the same frames."""
    import glob
    import json
    import os
    import subprocess
    import caffe_rtpose_amd as r
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path, out, N = str(tmp_path / "clip.y4m"), tmp_path / "json", 6
    out.mkdir()
    wr = r.VideoWriter(path, 320, 180)
    for i in range(N):
        wr.write_bgr(r.synth_frame(320, 180, i // 2, seed=2))   # every frame twice: its people match themselves
    wr.close()
    p = subprocess.run([os.path.join(root, "caffe_rtpose_amd", "rtpose.bin"), "--video", path, "--model", "coco", "--net_resolution", "160x96", "--resolution", "160x96",
                        "--write_json", str(out), "--track", "--track_min_parts", "2", "--track_max_cost", "4", "--track_appearance", "--appearance_weight", "8",
                        "--appearance_rate", "128", "--appearance_parts", "all", "--no_frame_drops", "--no_display", "--num_gpu", "2", "--devices", "0,0"],
                       capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    files = sorted(glob.glob(str(out / "*.json")))
    assert len(files) == N
    tcfg, acfg = r.track_config(min_parts=2, max_cost=4.0), r.appearance_config(parts=list(range(18)), weight=8.0, rate=128)
    ts, ap = r.TrackState(18), r.AppearanceState()
    e = r.Engine(r.Config(net_w=NET_W, net_h=NET_H, disp_w=160, disp_h=96))   # the CLI's engines: their defaults
    v = r.Video(path)
    matched = valid_total = 0
    try:
        for i, f in enumerate(files):
            frame = v.read()
            disp = e.debug_preprocess(frame)[1]
            e.submit_frame(frame, tag=i)
            _, n, joints = e.collect()
            b, vv = r.appearance_describe(disp, joints[:n], 18, acfg)
            recs = r.track_update_appearance(ts, ap, joints[:n], None, b, vv, tcfg, acfg)
            assert [x["id"] for x in json.load(open(f))["bodies"]] == [int(x) for x in recs[:, 0]], f"frame {i}"
            matched += int((recs[:, 2] >= 2).sum())
            valid_total += int(vv.sum())
    finally:
        v.close()
        e.close()
    assert matched >= 1 and valid_total >= 1, "somebody must be matched, and somebody must have a descriptor"

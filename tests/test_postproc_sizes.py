"""Post-processing kernels at max_peaks and thresholds other than the built-in ones, against the CPU oracle, bit for bit.

One test per (engine, input) of tests/_postcases.py; tests/test_postproc_sizes_cpu.py lists the branches of csrc/postproc.hip this matrix is
for (B1..B10) and asserts, without a GPU, that each is reached and that the oracle accepts every case.  For every threshold set of a case
(applied with set_thresholds on an engine that has run before):

  * low-res inputs: post_from_lowres (the production path: fused ImResize + NMS, fused pair kernel) == orc.imresize -> orc.nms ->
    orc.connect — peaks with their counts and the slots NMS does not write, the number of people, the joints, the JSON text; the
    map-materialising taps resize / nms / connect give the same; a second call gives the same again.
  * (resized map, peaks) inputs, which NMS cannot produce (exact ties, one-sided limbs, a late max_people cap): the connect tap == orc.connect,
    twice.

and at the end an all-zero map gives no peaks and no people: the people counter does not keep what the case before left in it.

Every comparison is np.array_equal / ==.  connect_inter_min_above_threshold < 0 is outside the reference's arithmetic (a score of 0 / 0):
rtp_set_thresholds refuses it, which is tested here; nothing out of range is ever run."""
import numpy as np
import pytest

import _oracle as orc
import _postcases as pc

pytestmark = pytest.mark.gpu

_ORDER = ("nms_threshold", "inter_threshold", "inter_min_above", "min_subset_cnt", "min_subset_score")


@pytest.fixture(scope="module")
def engines():
    """one engine per entry of the matrix, created at first use (and run once, on an empty map), closed at module teardown"""
    import caffe_rtpose_amd as r
    cache = {}

    def get(name):
        if name not in cache:
            e = r.Engine(pc.config(name))
            model, mp, _, N, _ = pc.ENGINES[name]
            assert e.max_peaks == mp and e.num_parts == orc.model_tables(model)[0]
            assert e.get_thresholds() == orc.default_thresholds(model)
            _, _, n = e.post_from_lowres(np.zeros((N, e.heat_channels, pc.LOW_H, pc.LOW_W), np.float32))
            assert n == 0
            cache[name] = e
        return cache[name]

    yield get
    for e in cache.values():
        e.close()


def _set(e, thr):
    e.set_thresholds(*[thr[k] for k in _ORDER])
    got = e.get_thresholds()
    assert all(np.float32(thr[k]) == np.float32(got[k]) for k in _ORDER), (thr, got)


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_postproc_matches_oracle(engines, case):
    import caffe_rtpose_amd as r
    engine, name, sets = case
    e = engines(engine)
    inp = pc.inputs(engine, name)
    stale = pc.stale_peaks(engine)
    for thr_name in sets:
        key = (engine, name, thr_name)
        _set(e, pc.thresholds(engine, thr_name))
        ref_res, ref_peaks, rn, rj = pc.reference(engine, name, thr_name)
        ref_json = orc.write_json(rj, rn, e.num_parts, 1.5)
        if inp["kind"] == "low":
            peaks, joints, n = e.post_from_lowres(inp["low"], stale)
            print(key, "people", n, "of", rn, "peak counts", int(ref_peaks[:, 0, 0].min()), "..", int(ref_peaks[:, 0, 0].max()))
            assert np.array_equal(peaks, ref_peaks), key
            assert n == rn and np.array_equal(joints, rj), key
            assert r.format_json(joints, n, e.num_parts, 1.5) == ref_json, key
            res = e.resize(inp["low"])
            assert np.array_equal(res, ref_res), key
            peaks2 = e.nms(res, stale)
            assert np.array_equal(peaks2, ref_peaks), key
            n2, joints2 = e.connect(res, peaks2)
            assert n2 == rn and np.array_equal(joints2[:n2], rj), key
            peaks3, joints3, n3 = e.post_from_lowres(inp["low"], stale)
            assert n3 == rn and np.array_equal(peaks3, ref_peaks) and np.array_equal(joints3, rj), key
        else:
            for _ in range(2):
                n, joints = e.connect(ref_res, ref_peaks)
                print(key, "people", n, "of", rn)
                assert n == rn and np.array_equal(joints[:n], rj), key
                assert not joints[n:].any(), key
                assert r.format_json(joints[:n], n, e.num_parts, 1.5) == ref_json, key
    model, mp, _, N, _ = pc.ENGINES[engine]
    _set(e, pc.thresholds(engine, "default"))
    peaks0, _, n0 = e.post_from_lowres(np.zeros((N, e.heat_channels, pc.LOW_H, pc.LOW_W), np.float32), stale)
    assert n0 == 0 and not peaks0[:, 0, 0].any() and np.array_equal(peaks0[:, 1:], stale[:, 1:])


def test_set_thresholds_refuses_a_negative_inter_min_above(engines):
    """count > inter_min_above with inter_min_above < 0 accepts pairs whose score is 0 / 0: refused, and the engine keeps its thresholds"""
    import caffe_rtpose_amd as r
    e = engines("coco2")
    thr = pc.thresholds("coco2", "sub1_0")
    _set(e, thr)
    before = e.post_from_lowres(pc.inputs("coco2", "noise")["low"])
    for bad in (-1, -10, -2 ** 31):
        with pytest.raises(r.RtpError) as ei:
            e.set_thresholds(0.5, 0.5, bad, 7, 0.9)
        assert ei.value.code == r.RTP_EINVAL
        assert all(np.float32(thr[k]) == np.float32(e.get_thresholds()[k]) for k in _ORDER)
    after = e.post_from_lowres(pc.inputs("coco2", "noise")["low"])
    assert before[2] == after[2] >= 1 and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_thresholds_set_between_batches_apply_to_the_next_frame():
    """COCO at max_peaks 127, batches of two frames, graph replay: after the batch graphs exist and have been replayed, set_thresholds with another
    set; the frames submitted next come back with the oracle's post-processing of their own low-res maps under the NEW thresholds (and not under
    the old ones).  This does NOT reach invalidate_graphs: the production library launches the post-processing chains eagerly behind the replayed
    convolution graph (capturing them is a knob of the experiments build only), so set_thresholds stores five numbers that the next launch reads.
    What is checked is the observable contract: graphs captured and replayed at max_peaks 127, then new thresholds, then the next frames obey them."""
    import caffe_rtpose_amd as r
    W, H = pc.NET_W, pc.NET_H
    e = r.Engine(pc.config("coco127", frames_in_flight=4, batch_frames=2, exec_mode=r.EXEC_GRAPH))
    frames = [r.preprocess_frame(r.synth_frame(640, 360, i, seed=21), 640, 360, W, H, 1, 1.0, 0.3)[0] for i in range(4)]
    lows = [e.forward_debug(f)["lowres"] for f in frames]
    old = orc.default_thresholds(0)
    new = dict(old, inter_min_above=4, min_subset_cnt=2, min_subset_score=0.05)

    def oracle(low, thr):
        res = orc.imresize(low, W, H, 1.0, 0.3)[0]
        peaks = orc.nms(res, 18, 127, thr["nms_threshold"])
        n, joints = orc.connect(0, res, peaks, 127, W, H, 1280, 720, thr)
        return n, joints[:n]

    def run(tag0):
        out = {}
        for rep in range(2):                      # the second pass replays the graphs the first one captured
            for i, f in enumerate(frames):
                e.submit(f, tag=tag0 + 10 * rep + i)
            while e.in_flight():
                tag, n, joints = e.collect()
                out[tag] = (n, joints)
        return out

    got = run(100)
    want_old = [oracle(low, old) for low in lows]
    for rep in range(2):
        for i in range(4):
            n, joints = got[100 + 10 * rep + i]
            assert n == want_old[i][0] and np.array_equal(joints, want_old[i][1]), (rep, i)
    _set(e, new)
    got = run(200)
    want_new = [oracle(low, new) for low in lows]
    print("people per frame, old thresholds", [w[0] for w in want_old], "new", [w[0] for w in want_new])
    for rep in range(2):
        for i in range(4):
            n, joints = got[200 + 10 * rep + i]
            assert n == want_new[i][0] and np.array_equal(joints, want_new[i][1]), (rep, i)
            assert not (n == want_old[i][0] and np.array_equal(joints, want_old[i][1])), (rep, i)
    e.close()

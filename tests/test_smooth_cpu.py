"""Smoothing mode without a GPU: rtp_smooth_update against the numpy restatement of the header's text (tests/_smoothref.py) on every
case of tests/_smoothcases.py, what the filter does to noise and to a ramp, every refusal, and rtpose.bin --track --smooth under
--dry_engine (where the re-orderer runs the host definitions)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import _smoothcases as sc
import _smoothref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
ALL_CASES = [c for P in (15, 18) for c in sc.cases(P)]
_REF = {}
F = np.float32


def ref_of(case):
    """the restatements' (outputs, states, records) of a case, computed once and shared"""
    if case["name"] not in _REF:
        _REF[case["name"]] = sc.run_ref(case)
    return _REF[case["name"]]


def test_the_abi_declares_and_exports_smoothing():
    from caffe_rtpose_amd import _lib
    for name in ("rtp_smooth_config_default", "rtp_smooth_state_init", "rtp_smooth_update", "rtp_set_smoothing", "rtp_smooth_reset", "rtp_smooth_get_state",
                 "rtp_smooth_set_state", "rtp_peek_smoothed", "rtp_smooth_from_joints"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    assert C.sizeof(_lib.rtp_smooth_state) == 12 + 128 * 70 * 28 and C.sizeof(_lib.rtp_smooth_config) == 28
    import caffe_rtpose_amd as r
    d = r.smooth_config()
    third = float(F(1.0) / F(30.0))
    assert (d.struct_size, d.min_score, d.min_cutoff, d.beta, d.d_cutoff, d.max_hold, d.apply) == (28, 0.0, third, float(F(0.01)), third, 5, 0)
    st = r.SmoothState(18)
    assert (st.num_parts, st.frames) == (18, 0) and not any(st.tobytes()[12:])
    assert sr.bits(sr.TWO_PI) == 0x40C90FDB and float(sr.TWO_PI) == float(F(6.2831855))


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["name"])
def test_the_restatement_reaches_every_cases_target(case):
    sc.check_predicates(case, *ref_of(case))


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["name"])
def test_host_definition_equals_the_restatement(case):
    """float bits, flags and the whole state after every frame"""
    import caffe_rtpose_amd as r
    ref_out, ref_states, ref_recs = ref_of(case)
    ts, st = r.TrackState(case["P"]), r.SmoothState(case["P"])
    tcfg, scfg = r.track_config(**case["tcfg"]), r.smooth_config(**case["scfg"])
    for i, (joints, num_people) in enumerate(case["frames"]):
        recs = r.track_update(ts, joints, num_people, tcfg)
        assert np.array_equal(recs.astype(np.int64) & 0xFFFFFFFF, ref_recs[i] & 0xFFFFFFFF), f"{case['name']} frame {i}: the records"
        got = r.smooth_update(st, joints, num_people, recs, scfg)
        diff = sr.same_out(ref_out[i], got)
        assert diff is None, f"{case['name']} frame {i}: {diff}"
        diff = sr.same_state(ref_states[i], st)
        assert diff is None, f"{case['name']} frame {i}: {diff}"


def _one_part(update, values, **cfg):
    """a tracked person of ONE part at (values[i], 7) in frame i through `update` -> the filtered x per frame"""
    out = np.zeros(len(values), np.float32)
    recs = np.array([[1, 0, 1, 0]], np.int32)
    j = np.zeros((1, 1, 3), np.float32)
    j[0, 0] = (0, 7, 1)
    for i, v in enumerate(values):
        j[0, 0, 0] = v
        out[i] = update(j, recs)[0][0, 0, 0]
    return out


def _lib_update(**cfg):
    import caffe_rtpose_amd as r
    st, c = r.SmoothState(1), r.smooth_config(**cfg)
    return lambda j, recs: r.smooth_update(st, j, None, recs, c)


def _ref_update(**cfg):
    st = sr.State(1)
    return lambda j, recs: sr.update(st, j, None, recs, **cfg)


def _alpha():
    r = float(sr.TWO_PI) * sr.DEFAULTS["min_cutoff"]
    return r / (r + 1.0)


@pytest.mark.parametrize("which", ["restatement", "library"])
def test_noise_attenuation(which):
    """beta 0: the filter is an exponential average with the constant a = r / (r + 1), r = TWO_PI * min_cutoff; white noise of variance
    1 leaves it with variance a / (2 - a).  20000 frames: the output's samples are correlated (1 - a = 0.83 from one to the next), which
    leaves about 3700 independent ones, so the variance estimate's standard error is about 2.3 % and 20 % a margin of six and more."""
    noise = np.random.default_rng(20260114).normal(0.0, 1.0, 20000).astype(np.float32)
    x = (F(300.0) + noise).astype(np.float32)
    out = _one_part((_ref_update if which == "restatement" else _lib_update)(beta=0.0), x)
    a = _alpha()
    want = a / (2.0 - a)
    ratio = float(np.var(out.astype(np.float64))) / float(np.var(x.astype(np.float64)))
    print(f"{which}: variance ratio {ratio:.5f}, expected {want:.5f} ({ratio / want - 1:+.2%})")
    assert abs(ratio / want - 1.0) <= 0.20


def test_lag_on_a_ramp():
    """beta 0 on a ramp of 2 pixels per frame: the exponential average trails by 2 * (1 - a) / a once it has settled ((1 - a)^200 is
    3e-17); with beta 0.05 the cutoff opens with the speed and the lag is strictly smaller."""
    ramp = (F(2.0) * np.arange(201, dtype=np.float32)).astype(np.float32)
    a = _alpha()
    want = 2.0 * (1.0 - a) / a
    lags = {}
    for name, upd in (("restatement", _ref_update), ("library", _lib_update)):
        out = _one_part(upd(beta=0.0), ramp)
        lags[name] = float(ramp[200]) - float(out[200])
        print(f"{name}: lag {lags[name]:.5f} pixels after 200 frames, expected {want:.5f}")
        assert abs(lags[name] - want) <= 0.01
    fast = _one_part(_lib_update(beta=0.05), ramp)
    assert 0.0 < float(ramp[200]) - float(fast[200]) < lags["library"]


def test_every_refusal_leaves_the_state_untouched():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    lib = _lib.lib
    P = 18
    two = np.stack([sc.body(P, 100, 100), sc.body(P, 400, 100)]).astype(np.float32)
    ts, st = r.TrackState(P), r.SmoothState(P)
    recs0 = r.track_update(ts, two)
    r.smooth_update(st, two, None, recs0)
    before = st.tobytes()
    good = r.smooth_config()
    js, vel, flags = np.full((96, P, 3), 7, np.float32), np.full((96, P, 2), 7, np.float32), np.full((96, P), 7, np.uint8)
    ubp = C.POINTER(C.c_ubyte)

    def call(state=st.c, cfg=good, joints=two, n=None, recs=recs0, out=js, v=vel, f=flags):
        n = len(two) if n is None else n
        return lib.rtp_smooth_update(C.byref(state) if state is not None else None, C.byref(cfg) if cfg is not None else None,
                                     joints.ctypes.data_as(_lib.fp) if joints is not None else None, n, recs.ctypes.data_as(_lib.ip) if recs is not None else None,
                                     out.ctypes.data_as(_lib.fp) if out is not None else None, v.ctypes.data_as(_lib.fp) if v is not None else None,
                                     f.ctypes.data_as(ubp) if f is not None else None)
    bad_cfgs = [dict(min_score=-0.1), dict(min_score=float("nan")), dict(min_score=float("inf")), dict(min_cutoff=0.0), dict(min_cutoff=-1.0), dict(min_cutoff=float("inf")),
                dict(min_cutoff=float("nan")), dict(beta=-0.5), dict(beta=float("inf")), dict(beta=float("nan")), dict(d_cutoff=0.0), dict(d_cutoff=float("nan")),
                dict(d_cutoff=float("inf")), dict(max_hold=-1), dict(max_hold=1001), dict(apply=4)]
    for kw in bad_cfgs:
        assert call(cfg=r.smooth_config(**kw)) == r.RTP_EINVAL, kw
        assert st.tobytes() == before, kw
    wrong = r.smooth_config()
    wrong.struct_size -= 4
    assert call(cfg=wrong) == r.RTP_EINVAL
    assert call(state=None) == call(cfg=None) == call(out=None) == call(joints=None) == call(recs=None) == r.RTP_EINVAL
    # two tracked records that name the same slot; a slot outside the table
    for slot0, slot1 in ((0, 0), (1, 1), (128, 1), (-1, 1), (0, 1 << 20)):
        recs = recs0.copy()
        recs[0, 1], recs[1, 1] = slot0, slot1
        assert call(recs=recs) == r.RTP_EINVAL, (slot0, slot1)
        assert st.tobytes() == before, (slot0, slot1)
    assert st.tobytes() == before and (js == 7).all() and (vel == 7).all() and (flags == 7).all(), "a refused call writes nothing"
    # (an untracked record's slot is not looked at; vel and flags may be NULL; nobody to read: NULL joints and records)
    recs = recs0.copy()
    recs[1] = (0, -1, 0, 0)
    probe = st.copy()
    assert call(state=probe.c, recs=recs, v=None, f=None) == 2 and probe.frames == st.frames + 1
    assert call(state=probe.c, joints=None, recs=None, n=0) == 0 and call(state=probe.c, joints=None, recs=None, n=-5) == 0 and probe.frames == st.frames + 3
    st2 = r.SmoothState(P)
    for field, v in (("struct_size", 8), ("num_parts", 0), ("num_parts", 71)):
        bad = st2.copy()
        setattr(bad.c, field, v)
        keep = bad.tobytes()
        assert call(state=bad.c) == r.RTP_EINVAL and bad.tobytes() == keep, (field, v)
    assert lib.rtp_smooth_state_init(C.byref(st2.c), 0) == r.RTP_EINVAL and lib.rtp_smooth_state_init(C.byref(st2.c), 71) == r.RTP_EINVAL
    assert lib.rtp_smooth_state_init(None, 18) == r.RTP_EINVAL and lib.rtp_smooth_config_default(None) == r.RTP_EINVAL
    assert st.tobytes() == before


def test_frames_wraps_past_zero():
    import caffe_rtpose_amd as r
    P = 15
    st, ref = r.SmoothState(P), sr.State(P)
    st.frames = ref.frames = 0xFFFFFFFE
    one = sc.body(P, 100, 100)[None]
    recs = np.array([[9, 3, 1, 0]], np.int32)
    for i in range(3):   # frames 0xFFFFFFFF, 1 (0 is skipped), 2: the gap across the wrap is 2 in uint32 arithmetic
        got = r.smooth_update(st, one + F(i), None, recs)
        want = sr.update(ref, one + F(i), None, recs)
        assert sr.same_out(want, got) is None and sr.same_state(ref, st) is None
        assert [int(v) for v in got[2][0]] == [1 if i == 0 else 2] * P
    assert st.frames == 2


DRY = ["--video", "synthetic:64x48:24", "--dry_engine", "400", "--dry_people", "4", "--model", "coco", "--resolution", "64x48", "--net_resolution", "64x48", "--no_display",
       "--no_frame_drops"]


def _cli(out, *extra):
    os.makedirs(out, exist_ok=True)
    p = subprocess.run([BIN] + DRY + ["--write_json", out] + list(extra), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    files = sorted(glob.glob(os.path.join(out, "*.json")))
    assert len(files) == 24
    return {os.path.basename(f): open(f, "rb").read() for f in files}


def _dry_people(index, people, P):
    """the stand-in worker's people of frame `index` (rtpose_main.cpp dry_collect: a xorshift of the frame's index)"""
    M = (1 << 64) - 1
    x = (0x9E3779B97F4A7C15 * (index + 1)) & M
    j = np.zeros((people * P, 3), np.float32)
    for i in range(people * P):
        x ^= (x << 13) & M
        x ^= x >> 7
        x ^= (x << 17) & M
        j[i] = (F(x % 1280000) / F(1000.0), F((x >> 20) % 720000) / F(1000.0), F((x >> 40) % 1000) / F(1000.0))
    return j.reshape(people, P, 3)


def test_cli_dry_engine_smooths_in_the_reorderer(tmp_path):
    import caffe_rtpose_amd as r
    args = ["--track", "--track_max_cost", "1000", "--track_min_parts", "1", "--smooth", "--smooth_max_hold", "2", "--smooth_beta", "0.5"]
    one = _cli(str(tmp_path / "one"), *args, "--num_gpu", "1")
    two = _cli(str(tmp_path / "two"), *args, "--num_gpu", "2")
    assert one == two, "the re-orderer filters in frame order whatever the number of workers"
    ts, st = r.TrackState(18), r.SmoothState(18)
    tcfg, scfg = r.track_config(max_cost=1000, min_parts=1), r.smooth_config(max_hold=2, beta=0.5, apply=r.SMOOTH_RENDER | r.SMOOTH_CROPS)
    seen = set()
    for i, name in enumerate(sorted(one)):
        j = _dry_people(i + 1, 4, 18)   # (the program counts its frames from 1)
        recs = r.track_update(ts, j, cfg=tcfg)
        js, _, flags = r.smooth_update(st, j, None, recs, scfg)
        seen |= set(int(v) for v in flags.reshape(-1))
        assert one[name] == r.format_json_tracked(js, 18, 1.0, recs), name
        assert i == 0 or one[name] != r.format_json_tracked(j, 18, 1.0, recs), f"{name}: the raw joints"
    assert 2 in seen, "some part must have been filtered"
    tracked = _cli(str(tmp_path / "tracked"), *args[:5], "--num_gpu", "1")
    plain = _cli(str(tmp_path / "plain"), "--track", "--track_max_cost", "1000", "--track_min_parts", "1", "--num_gpu", "2")
    assert tracked == plain and tracked != one, "without --smooth the files are what --track alone writes"
    p = subprocess.run([BIN] + DRY + ["--write_json", str(tmp_path / "bad"), "--smooth"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--smooth needs --track" in p.stderr
    p = subprocess.run([BIN] + DRY + ["--write_json", str(tmp_path / "bad"), "--track", "--smooth", "--smooth_min_cutoff", "0"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--smooth_min_cutoff" in p.stderr
    h = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(w in h for w in ("--smooth", "--smooth_min_cutoff", "--smooth_beta", "--smooth_d_cutoff", "--smooth_max_hold", "rtp_smooth_update", "raw joints"))

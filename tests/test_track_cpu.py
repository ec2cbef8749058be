"""Tracking mode without a GPU: rtp_track_update against the numpy restatement of the header's text (tests/_trackref.py) on every case
of tests/_trackcases.py, every refusal, rtp_format_json_tracked, rtpose.bin --track under --dry_engine (where the re-orderer runs the
host definition), and the host definition under the address / undefined sanitizers in a program of its own."""
import ctypes as C
import glob
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import _trackcases as tc
import _trackref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
ALL_CASES = [c for P in (15, 18, 70) for c in tc.cases(P)]
_REF = {}


def ref_of(case):
    """the restatement's (records, states) of a case, computed once and shared"""
    if case["name"] not in _REF:
        _REF[case["name"]] = tc.run_ref(case)
    return _REF[case["name"]]


def test_the_abi_declares_and_exports_tracking():
    from caffe_rtpose_amd import _lib
    for name in ("rtp_track_config_default", "rtp_track_state_init", "rtp_track_update", "rtp_set_tracking", "rtp_track_reset", "rtp_track_get_state",
                 "rtp_track_set_state", "rtp_peek_tracks", "rtp_track_from_joints", "rtp_format_json_tracked"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    assert C.sizeof(_lib.rtp_track_state) == 16 + 3 * 128 * 4 + 128 * 70 * 3 * 4 and C.sizeof(_lib.rtp_track_config) == 24
    import caffe_rtpose_amd as r
    d = r.track_config()
    assert (d.struct_size, d.min_score, d.min_parts, d.min_common, d.max_cost, d.max_misses) == (24, 0.0, 3, 2, 0.0625, 15)
    st = r.TrackState(18)
    assert (st.num_parts, st.next_id, st.frames) == (18, 1, 0) and not st.id.any() and not st.joints.any()


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["name"])
def test_the_restatement_reaches_every_cases_target(case):
    tc.check_predicates(case, *ref_of(case))


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["name"])
def test_host_definition_equals_the_restatement(case):
    import caffe_rtpose_amd as r
    ref_recs, ref_states = ref_of(case)
    st = r.TrackState(case["P"])
    cfg = r.track_config(**case["cfg"])
    for i, (joints, num_people) in enumerate(case["frames"]):
        recs = r.track_update(st, joints, num_people, cfg)
        assert tr.same_recs(ref_recs[i], recs), f"{case['name']} frame {i}: records\n{recs}\nexpected\n{ref_recs[i]}"
        diff = tr.same_state(ref_states[i], st)
        assert diff is None, f"{case['name']} frame {i}: {diff}"


def test_every_refusal_leaves_the_state_untouched():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    lib = _lib.lib
    case = tc.cases(18)[0]
    st = r.TrackState(18)
    r.track_update(st, case["frames"][0][0], cfg=r.track_config(**case["cfg"]))
    before = st.tobytes()
    j = np.ascontiguousarray(case["frames"][1][0], np.float32)
    recs = np.zeros((96, 4), np.int32)
    good = r.track_config()

    def call(state=st.c, cfg=good, joints=j, n=None, out=recs):
        n = len(j) if n is None else n
        return lib.rtp_track_update(C.byref(state) if state is not None else None, C.byref(cfg) if cfg is not None else None,
                                    joints.ctypes.data_as(_lib.fp) if joints is not None else None, n, out.ctypes.data_as(_lib.ip) if out is not None else None)
    bad_cfgs = [dict(min_score=-0.1), dict(min_score=float("nan")), dict(min_score=float("inf")), dict(min_parts=0), dict(min_common=0), dict(max_cost=0.0),
                dict(max_cost=-1.0), dict(max_cost=float("inf")), dict(max_cost=float("nan")), dict(max_misses=-1)]
    for kw in bad_cfgs:
        assert call(cfg=r.track_config(**kw)) == r.RTP_EINVAL, kw
        assert st.tobytes() == before, kw
    wrong = r.track_config()
    wrong.struct_size -= 4
    assert call(cfg=wrong) == r.RTP_EINVAL
    assert call(state=None) == call(cfg=None) == call(out=None) == call(joints=None) == r.RTP_EINVAL
    assert call(joints=None, n=0) == 0    # nobody is read: the frame counts (undone below)
    st2 = r.TrackState(18)
    for field, v in (("struct_size", 8), ("num_parts", 0), ("num_parts", 71)):
        bad = st2.copy()
        setattr(bad.c, field, v)
        keep = bad.tobytes()
        assert call(state=bad.c) == r.RTP_EINVAL and bad.tobytes() == keep, (field, v)
    assert _lib.lib.rtp_track_state_init(C.byref(st2.c), 0) == r.RTP_EINVAL and _lib.lib.rtp_track_state_init(C.byref(st2.c), 71) == r.RTP_EINVAL
    assert _lib.lib.rtp_track_state_init(None, 18) == r.RTP_EINVAL and _lib.lib.rtp_track_config_default(None) == r.RTP_EINVAL


def test_next_id_wraps_past_zero():
    import caffe_rtpose_amd as r
    st, ref = r.TrackState(18), tr.State(18)
    st.next_id = ref.next_id = 0xFFFFFFFF
    frame = np.stack([tc.body(18, 100 + 300 * i, 100) for i in range(3)])
    recs = r.track_update(st, frame)
    want = tr.update(ref, frame)
    assert tr.same_recs(want, recs) and tr.same_state(ref, st) is None
    assert [int(x) for x in recs[:, 0]] == [-1, 1, 2] and st.next_id == 3


def test_format_json_tracked():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    rng = np.random.default_rng(5)
    for people, parts in ((0, 18), (1, 15), (3, 18), (7, 70)):
        j = rng.uniform(0, 700, (people, parts, 3)).astype(np.float32)
        plain = C.create_string_buffer(1 << 20)
        n = _lib.lib.rtp_format_json(plain, len(plain), j.ctypes.data_as(_lib.fp) if people else None, people, parts, 0.5)
        assert n > 0
        assert r.format_json_tracked(j, parts, 0.5, None) == plain.raw[:n], "NULL recs: byte for byte rtp_format_json"
        recs = np.zeros((max(people, 1), 4), np.int32)
        recs[:, 0] = [0, 7, 2147483647, -5, 12, 1, 3][:max(people, 1)]
        recs[:, 1:] = 99
        text = r.format_json_tracked(j, parts, 0.5, recs)
        doc = json.loads(text)
        assert [b["id"] for b in doc["bodies"]] == [int(x) for x in recs[:people, 0]]
        assert re.sub(rb'"id":-?\d+,', b"", text) == plain.raw[:n], "only the id members differ"
        assert text.count(b'"id":') == people and all(list(b)[0] == "id" for b in doc["bodies"])
    small = C.create_string_buffer(40)
    j = np.zeros((1, 18, 3), np.float32)
    assert _lib.lib.rtp_format_json_tracked(small, len(small), j.ctypes.data_as(_lib.fp), 1, 18, 1.0, np.zeros(4, np.int32).ctypes.data_as(_lib.ip)) == r.RTP_ERANGE


DRY = ["--video", "synthetic:64x48:24", "--dry_engine", "400", "--dry_people", "4", "--model", "coco", "--resolution", "64x48", "--net_resolution", "64x48", "--no_display",
       "--no_frame_drops"]


def _cli(out, *extra):
    os.makedirs(out, exist_ok=True)
    p = subprocess.run([BIN] + DRY + ["--write_json", out] + list(extra), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    files = sorted(glob.glob(os.path.join(out, "*.json")))
    assert len(files) == 24
    return {os.path.basename(f): open(f, "rb").read() for f in files}


def test_cli_dry_engine_tracks_in_the_reorderer(tmp_path):
    one = _cli(str(tmp_path / "one"), "--track", "--num_gpu", "1")
    four = _cli(str(tmp_path / "four"), "--track", "--num_gpu", "4")
    assert one == four, "the re-orderer tracks in frame order whatever the number of workers"
    seen = []
    for name, text in one.items():
        bodies = json.loads(text)["bodies"]
        assert len(bodies) == 4 and all(isinstance(b["id"], int) for b in bodies), name
        ids = [b["id"] for b in bodies if b["id"]]
        assert len(set(ids)) == len(ids), f"{name}: ids {ids}"
        seen += ids
    assert seen, "somebody is tracked"
    plain = _cli(str(tmp_path / "plain"), "--num_gpu", "1")
    assert all(b'"id"' not in t for t in plain.values()), "without --track the files carry no ids"
    assert {k: re.sub(rb'"id":-?\d+,', b"", v) for k, v in one.items()} == plain, "--track adds the id members and nothing else"
    p = subprocess.run([BIN] + DRY + ["--write_json", str(tmp_path / "bad"), "--track", "--track_max_cost", "0"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--track_max_cost" in p.stderr
    h = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--track" in h and "--track_max_cost" in h and "--track_max_misses" in h and "--track_min_parts" in h and "rtp_track_update" in h


def _case_file(path, cases):
    """the cases and rtp_track_update's own records as the replay program reads them (tests/helpers/track_check.cpp)"""
    import caffe_rtpose_amd as r
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for case in cases:
            c = tr.config(**case["cfg"])
            f.write(struct.pack("<ifiifii", case["P"], c["min_score"], c["min_parts"], c["min_common"], c["max_cost"], c["max_misses"], len(case["frames"])))
            st = r.TrackState(case["P"])
            for joints, num_people in case["frames"]:
                j = np.ascontiguousarray(joints, np.float32).reshape(-1, case["P"], 3)
                people = len(j) if num_people is None else num_people
                recs = r.track_update(st, j, num_people, r.track_config(**case["cfg"]))
                f.write(struct.pack("<ii", people, len(j)) + j.tobytes() + struct.pack("<i", len(recs)) + np.ascontiguousarray(recs, np.int32).tobytes())


def test_host_definition_is_clean_under_sanitizers(tmp_path):
    """tests/helpers/track_check.cpp (its own main) replays every case through rtp_track_update on exactly-sized heap blocks and compares
    with the records this process got: an element read or written outside a block is an AddressSanitizer report.  Built with the
    host-only sources; nothing is loaded into python."""
    csrc = os.path.join(ROOT, "caffe_rtpose_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "helpers", "track_check.cpp")] + [os.path.join(csrc, f) for f in ("codecs.cpp", "preprocess.cpp", "host_util.cpp")]
    exe = str(tmp_path / "track_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-o", exe] + src + ["-lpthread", "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    data = str(tmp_path / "cases.bin")
    _case_file(data, ALL_CASES)
    q = subprocess.run([exe, data], capture_output=True, text=True, timeout=300, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert q.returncode == 0, q.stdout[-2000:] + q.stderr[-3000:]
    assert not [ln for ln in q.stderr.splitlines() if "Sanitizer" in ln or "runtime error:" in ln], q.stderr[-3000:]
    assert f"track_check OK: {len(ALL_CASES)} cases" in q.stdout

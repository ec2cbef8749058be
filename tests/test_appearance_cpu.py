"""Appearance-aided tracking without a GPU: rtp_appearance_describe and rtp_track_update_appearance against the numpy restatement of the
header's text (tests/_appearref.py) on every case of tests/_appearcases.py, neutrality against rtp_track_update on every sequence of
tests/_trackcases.py, the crossing, every refusal, the ABI, and the two host definitions under the address / undefined sanitizers in
a program of their own."""
import ctypes as C
import glob
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import _appearcases as ac
import _appearref as ar
import _trackcases as tc
import _trackref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESCRIBE_CASES = [c for P in (18, 15) for c in ac.describe_cases(P)]
UPDATE_CASES = [c for P in (18, 15) for c in ac.update_cases(P)]
TRACK_CASES = [c for P in (15, 18, 70) for c in tc.cases(P)]
_REF = {}


def ref_of(case):
    """the restatement's result of an update case, computed once and shared"""
    if case["name"] not in _REF:
        _REF[case["name"]] = ac.run_ref(case)
    return _REF[case["name"]]


def test_the_abi_declares_and_exports_appearance():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    for name in ("rtp_appearance_config_default", "rtp_appearance_state_init", "rtp_appearance_torso_parts", "rtp_appearance_describe", "rtp_track_update_appearance"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    assert C.sizeof(_lib.rtp_appearance_state) == 16 + 128 * 4 + 128 * 128 * 2 and C.sizeof(_lib.rtp_appearance_config) == 48
    assert _lib.rtp_appearance_state.desc.offset % 16 == 0
    assert C.sizeof(_lib.rtp_track_state) == 16 + 3 * 128 * 4 + 128 * 70 * 3 * 4 and C.sizeof(_lib.rtp_track_config) == 24, "the tracker's structures keep their sizes"
    d = r.appearance_config()
    assert (d.struct_size, bool(d.parts), d.min_score, d.min_parts, d.margin, d.weight, d.max_dist, d.unknown, d.rate) == (48, False, 0.0, 3, 0.0, 0.125, 1.0, 0.25, 32)
    assert {k: v for k, v in ar.DEFAULTS.items() if k != "parts"} == dict(min_score=0.0, min_parts=3, margin=0.0, weight=0.125, max_dist=1.0, unknown=0.25, rate=32)
    st = r.AppearanceState()
    assert st.c.struct_size == C.sizeof(_lib.rtp_appearance_state) and not st.owner.any() and not st.desc.any()
    assert r.appearance_torso_parts(r.MODEL_COCO_18) == ar.TORSO[18] == [1, 2, 5, 8, 11] and r.appearance_torso_parts(r.MODEL_MPI_15) == ar.TORSO[15] == [1, 2, 5, 8, 11, 14]
    assert _lib.lib.rtp_appearance_torso_parts(2, (C.c_int * 8)()) == r.RTP_EINVAL


@pytest.mark.parametrize("case", DESCRIBE_CASES, ids=lambda c: c["name"])
def test_describe_equals_the_restatement_and_reaches_its_target(case):
    import caffe_rtpose_amd as r
    bins, valid = ar.describe(case["image"], case["joints"], case["P"], **case["cfg"])
    assert case["pred"](bins, valid), f"{case['name']} does not reach its target: valid {valid.tolist()}, bins {bins[:2].tolist()}"
    got_bins, got_valid = r.appearance_describe(case["image"], case["joints"], case["P"], r.appearance_config(**case["cfg"]))
    assert np.array_equal(valid, got_valid), (valid.tolist(), got_valid.tolist())
    assert np.array_equal(bins, got_bins), f"people {np.flatnonzero((bins != got_bins).any(1)).tolist()} differ"
    assert (got_bins.sum(1) == 1024 * got_valid.astype(np.int64)).all()


def test_describe_clamps_the_number_of_people():
    import caffe_rtpose_amd as r
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (ac.H, ac.W, 3), dtype=np.uint8)
    crowd = np.stack([tc.body(18, 3 * (i % 40), 2 * (i // 3)) for i in range(120)])
    bins, valid = r.appearance_describe(img, crowd, 18)
    assert bins.shape == (96, 128) and valid.all()
    want = ar.describe(img, crowd, 18)
    assert np.array_equal(bins, want[0]) and np.array_equal(valid, want[1])
    none = r.appearance_describe(img, np.zeros((0, 18, 3), np.float32), 18)
    assert none[0].shape == (0, 128) and none[1].shape == (0,)


def replay_host(case):
    """the two host definitions over an update case, as ac.run_ref runs the restatement"""
    import caffe_rtpose_amd as r
    ts, ap = r.TrackState(case["P"]), r.AppearanceState()
    acfg, tcfg = r.appearance_config(**case["cfg"]), r.track_config(**case["track"])
    out = []
    for joints, num_people, image in case["frames"]:
        b, v = r.appearance_describe(image, joints, case["P"], acfg) if image is not None else (None, None)
        recs = r.track_update_appearance(ts, ap, joints, num_people, b, v, tcfg, acfg)
        out.append((recs, ts.copy(), ap.copy(), (b, v)))
    return out


@pytest.mark.parametrize("case", UPDATE_CASES, ids=lambda c: c["name"])
def test_update_equals_the_restatement(case):
    ref_recs, ref_ts, ref_ap, ref_d = ref_of(case)
    ac.check_predicates(case, ref_recs, ref_ts, ref_ap, ref_d)   # the restatement alone reaches the case's target ...
    host = replay_host(case)
    ac.check_predicates(case, *[[h[i] for h in host] for i in range(4)])   # ... and so do the host definitions
    for i, (recs, ts, ap, (b, v)) in enumerate(host):
        if b is not None:
            assert np.array_equal(b, ref_d[i][0]) and np.array_equal(v, ref_d[i][1]), f"{case['name']} frame {i}: descriptors"
        assert tr.same_recs(ref_recs[i], recs), f"{case['name']} frame {i}: records\n{recs}\nexpected\n{ref_recs[i]}"
        diff = tr.same_state(ref_ts[i], ts) or ar.same_state(ref_ap[i], ap)
        assert diff is None, f"{case['name']} frame {i}: {diff}"


def test_the_crossing_swaps_the_ids_without_the_descriptors_and_keeps_them_with():
    import caffe_rtpose_amd as r
    case = ac.crossing(18)
    assert case["cfg"] == dict(weight=4.0) and case["track"] == dict(max_cost=2.0)
    tcfg = r.track_config(**case["track"])
    st = r.TrackState(18)
    plain = [r.track_update(st, joints, num_people, tcfg) for joints, num_people, _ in case["frames"]]
    assert tc.ids(plain[0]) == [1, 2] and tc.ids(plain[1]) == [2, 1], "displacement alone swaps the ids: the failure the mode exists for"
    assert tc.rec(plain[1], 0)[3] == 0 and tc.rec(plain[1], 1)[3] == 0
    aided = [x[0] for x in replay_host(case)]
    assert tc.ids(aided[0]) == [1, 2] and tc.ids(aided[1]) == [1, 2], "the person in red keeps id 1"
    assert tc.rec(aided[1], 0) == [1, 0, 2, tr.bits(1.0)] and tc.rec(aided[1], 1) == [2, 1, 2, tr.bits(1.0)]


@pytest.mark.parametrize("case", TRACK_CASES, ids=lambda c: c["name"])
def test_weight_zero_is_rtp_track_update_bit_for_bit(case):
    """weight 0, max_dist 1, unknown 0: whatever the descriptors are (random ones, some invalid, and a table that fills with them),
    records and track table are rtp_track_update's."""
    import caffe_rtpose_amd as r
    rng = np.random.default_rng(len(case["name"]))
    tcfg, acfg = r.track_config(**case["cfg"]), r.appearance_config(weight=0.0, max_dist=1.0, unknown=0.0, rate=77)
    plain, aided, ap = r.TrackState(case["P"]), r.TrackState(case["P"]), r.AppearanceState()
    for i, (joints, num_people) in enumerate(case["frames"]):
        want = r.track_update(plain, joints, num_people, tcfg)
        rows = np.asarray(joints).reshape(-1, case["P"], 3).shape[0]
        bins = np.zeros((rows, 128), np.uint16)
        for k in range(rows):
            bins[k] = np.bincount(rng.integers(0, 128, 1024), minlength=128)
        valid = (rng.integers(0, 4, rows) > 0).astype(np.uint8)
        got = r.track_update_appearance(aided, ap, joints, num_people, bins if i % 3 != 2 else None, valid, tcfg, acfg)
        assert np.array_equal(want, got), f"{case['name']} frame {i}"
        assert plain == aided, f"{case['name']} frame {i}: the track tables differ"


def test_every_refusal_leaves_both_states_untouched():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    lib = _lib.lib
    case = ac.crossing(18)
    joints, _, image = case["frames"][0]
    ts, ap = r.TrackState(18), r.AppearanceState()
    bins, valid = r.appearance_describe(image, joints, 18)
    r.track_update_appearance(ts, ap, joints, None, bins, valid)
    before = ts.tobytes(), ap.tobytes()
    assert ap.owner[:2].tolist() == [1, 2]
    j = np.ascontiguousarray(joints, np.float32)
    recs = np.zeros((96, 4), np.int32)
    u16p, u8p = C.POINTER(C.c_uint16), C.POINTER(C.c_ubyte)

    def call(t=ts.c, a=ap.c, tcfg=r.track_config(), acfg=r.appearance_config(), jj=j, n=None, b=bins, v=valid, out=recs):
        n = len(j) if n is None else n
        ref = lambda x: C.byref(x) if x is not None else None
        return lib.rtp_track_update_appearance(ref(t), ref(a), ref(tcfg), ref(acfg), jj.ctypes.data_as(_lib.fp) if jj is not None else None, n,
                                               b.ctypes.data_as(u16p) if b is not None else None, v.ctypes.data_as(u8p) if v is not None else None,
                                               out.ctypes.data_as(_lib.ip) if out is not None else None)
    bad_acfgs = [dict(min_score=-1.0), dict(min_score=float("nan")), dict(min_score=float("inf")), dict(min_parts=0), dict(margin=-0.5), dict(margin=16.5), dict(margin=float("nan")),
                 dict(weight=-0.1), dict(weight=float("inf")), dict(weight=float("nan")), dict(max_dist=0.0), dict(max_dist=1.5), dict(max_dist=float("nan")),
                 dict(unknown=-0.1), dict(unknown=1.5), dict(unknown=float("nan")), dict(rate=0), dict(rate=257)]
    for kw in bad_acfgs:
        assert call(acfg=r.appearance_config(**kw)) == r.RTP_EINVAL, kw
        assert (ts.tobytes(), ap.tobytes()) == before, kw
    for kw in (dict(max_cost=0.0), dict(min_parts=0), dict(min_common=0), dict(max_misses=-1), dict(min_score=float("nan"))):
        assert call(tcfg=r.track_config(**kw)) == r.RTP_EINVAL, kw
    wrong_a, wrong_t = r.appearance_config(), r.track_config()
    wrong_a.struct_size -= 4
    wrong_t.struct_size += 4
    assert call(acfg=wrong_a) == call(tcfg=wrong_t) == r.RTP_EINVAL
    assert call(t=None) == call(a=None) == call(tcfg=None) == call(acfg=None) == call(out=None) == call(jj=None) == call(v=None) == r.RTP_EINVAL
    for st2, field, val in ((r.TrackState(18), "struct_size", 8), (r.TrackState(18), "num_parts", 0), (r.TrackState(18), "num_parts", 71)):
        setattr(st2.c, field, val)
        keep = st2.tobytes()
        assert call(t=st2.c) == r.RTP_EINVAL and st2.tobytes() == keep
    ap2 = r.AppearanceState()
    ap2.c.struct_size = 12
    keep = ap2.tobytes()
    assert call(a=ap2.c) == r.RTP_EINVAL and ap2.tobytes() == keep
    assert (ts.tobytes(), ap.tobytes()) == before
    assert lib.rtp_appearance_state_init(None) == lib.rtp_appearance_config_default(None) == r.RTP_EINVAL
    # the describe call: nothing is written by a refused call
    img = np.ascontiguousarray(image)
    out_b, out_v = np.full((2, 128), 7, np.uint16), np.full(2, 7, np.uint8)

    def desc(image=img, w=ac.W, h=ac.H, jj=j, n=2, P=18, acfg=r.appearance_config(), b=out_b, v=out_v):
        return lib.rtp_appearance_describe(image.ctypes.data_as(u8p) if image is not None else None, w, h, jj.ctypes.data_as(_lib.fp) if jj is not None else None, n, P,
                                           C.byref(acfg) if acfg is not None else None, b.ctypes.data_as(u16p) if b is not None else None,
                                           v.ctypes.data_as(u8p) if v is not None else None)
    for kw in bad_acfgs + [dict(parts=[18]), dict(parts=[-1]), dict(parts=[])]:
        assert desc(acfg=r.appearance_config(**kw)) == r.RTP_EINVAL, kw
    assert desc(acfg=wrong_a) == desc(acfg=None) == desc(image=None) == desc(jj=None) == desc(b=None) == desc(v=None) == r.RTP_EINVAL
    assert desc(w=0) == desc(h=0) == desc(w=32769) == desc(h=32769) == desc(n=-1) == desc(P=0) == desc(P=71) == r.RTP_EINVAL
    assert (out_b == 7).all() and (out_v == 7).all()
    assert desc(image=None, jj=None, n=0) == 0 and desc() == 2 and out_v.tolist() == [1, 1]


BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
DRY_W, DRY_H, DRY_FRAMES, DRY_PEOPLE = 64, 48, 24, 4
DRY = ["--video", f"synthetic:{DRY_W}x{DRY_H}:{DRY_FRAMES}", "--dry_engine", "400", "--dry_people", str(DRY_PEOPLE), "--model", "coco", "--resolution", f"{DRY_W}x{DRY_H}",
       "--net_resolution", f"{DRY_W}x{DRY_H}", "--no_display", "--no_frame_drops"]


def _dry_joints(index, people=DRY_PEOPLE, P=18):
    """the people rtpose.bin's dry workers hand out for the frame of this index (rtpose_main.cpp dry_collect)"""
    M = (1 << 64) - 1
    x = (0x9E3779B97F4A7C15 * (index + 1)) & M
    j = np.zeros((people * P, 3), np.float32)
    for i in range(people * P):
        x ^= (x << 13) & M
        x ^= x >> 7
        x ^= (x << 17) & M
        j[i] = (np.float32(x % 1280000) / np.float32(1000), np.float32((x >> 20) % 720000) / np.float32(1000), np.float32((x >> 40) % 1000) / np.float32(1000))
    return j.reshape(people, P, 3)


def _cli_ids(out, *extra):
    os.makedirs(out, exist_ok=True)
    p = subprocess.run([BIN] + DRY + ["--write_json", out] + list(extra), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    files = sorted(glob.glob(os.path.join(out, "*.json")))
    assert len(files) == DRY_FRAMES
    return [[b["id"] for b in json.load(open(f))["bodies"]] for f in files]


def test_cli_dry_engine_tracks_with_appearance_in_the_reorderer(tmp_path):
    """The re-orderer describes every frame's people on the display image it was handed and runs rtp_track_update_appearance in frame
    order: the ids of the JSON files equal a replay of the two host definitions over the dry workers' people and the synthetic frames,
    whatever the number of workers, with --host_preprocess too, and they are not the ids of --track alone."""
    import caffe_rtpose_amd as r
    flags = ["--track", "--track_max_cost", "4", "--track_min_parts", "2", "--track_appearance", "--appearance_weight", "64", "--appearance_rate", "128",
             "--appearance_parts", "all"]
    tcfg = r.track_config(max_cost=4.0, min_parts=2)
    acfg = r.appearance_config(parts=list(range(18)), weight=64.0, rate=128)
    ts, ap, plain = r.TrackState(18), r.AppearanceState(), r.TrackState(18)
    want, alone = [], []
    for i in range(DRY_FRAMES):
        joints = _dry_joints(i + 1)     # (frame indices start at 1)
        disp, _ = r.warp_display(r.synth_frame(DRY_W, DRY_H, i, seed=2), DRY_W, DRY_H)
        b, v = r.appearance_describe(disp, joints, 18, acfg)
        want.append([int(x) for x in r.track_update_appearance(ts, ap, joints, None, b, v, tcfg, acfg)[:, 0]])
        alone.append([int(x) for x in r.track_update(plain, joints, None, tcfg)[:, 0]])
    assert _cli_ids(str(tmp_path / "alone"), *flags[:5], "--num_gpu", "1") == alone, "--track alone: the replay of rtp_track_update (the dry people are what this test takes them to be)"
    assert want != alone, "the appearance term must decide at least one assignment, or this test shows nothing"
    assert any(len(set(a) & set(b)) for a, b in zip(want, want[1:])), "somebody must be matched across two frames"
    one = _cli_ids(str(tmp_path / "one"), *flags, "--num_gpu", "1")
    assert one == want, "the ids are the replay's"
    assert _cli_ids(str(tmp_path / "four"), *flags, "--num_gpu", "4") == want, "the re-orderer works in frame order whatever the number of workers"
    assert _cli_ids(str(tmp_path / "hostpre"), *flags, "--num_gpu", "2", "--host_preprocess") == want, "with --host_preprocess the producer keeps the display image"
    for bad in (["--track_appearance"], ["--track", "--track_appearance", "--appearance_max_dist", "0"], ["--track", "--track_appearance", "--appearance_rate", "300"],
                ["--track", "--track_appearance", "--appearance_weight", "-1"], ["--track", "--track_appearance", "--appearance_parts", "nose"]):
        p = subprocess.run([BIN] + DRY + ["--write_json", str(tmp_path / "bad")] + bad, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and "--track_appearance" in p.stderr, bad
    h = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(w in h for w in ("--track_appearance", "--appearance_weight", "--appearance_max_dist", "--appearance_rate", "--appearance_parts", "rtp_track_update_appearance"))


def test_cli_video_files_reach_the_reorderer_as_bgr_frames(tmp_path):
    """A Y4M and an MJPEG file under --num_gpu 2 --track --track_appearance: the producer hands the workers BGR frames (not planes or
    JPEG bytes), the re-orderer warps each to the display image and describes the people on it: the ids equal the host replay over the
    frames Video.read returns.  A part list outside the model's parts is refused, not tracked as unknown."""
    import caffe_rtpose_amd as r
    W, H, N = 96, 64, 10          # (not the display size: the warp matters)
    src = [r.synth_frame(W, H, i, seed=7) for i in range(N)]
    flags = ["--dry_engine", "400", "--dry_people", str(DRY_PEOPLE), "--model", "coco", "--resolution", f"{DRY_W}x{DRY_H}", "--net_resolution", f"{DRY_W}x{DRY_H}", "--no_display",
             "--no_frame_drops", "--num_gpu", "2", "--track", "--track_max_cost", "4", "--track_min_parts", "2", "--track_appearance", "--appearance_weight", "64",
             "--appearance_rate", "128", "--appearance_parts", "all"]
    tcfg = r.track_config(max_cost=4.0, min_parts=2)
    acfg = r.appearance_config(parts=list(range(18)), weight=64.0, rate=128)
    for name in ("clip.y4m", "clip.mjpeg"):
        path = str(tmp_path / name)
        wr = r.VideoWriter(path, W, H)
        for f in src:
            wr.write_bgr(f)
        wr.close()
        v = r.Video(path)
        ts, ap, plain = r.TrackState(18), r.AppearanceState(), r.TrackState(18)
        want, alone = [], []
        for i in range(N):
            disp, _ = r.warp_display(v.read(), DRY_W, DRY_H)
            joints = _dry_joints(i + 1)
            b, vv = r.appearance_describe(disp, joints, 18, acfg)
            want.append([int(x) for x in r.track_update_appearance(ts, ap, joints, None, b, vv, tcfg, acfg)[:, 0]])
            alone.append([int(x) for x in r.track_update(plain, joints, None, tcfg)[:, 0]])
        v.close()
        assert want != alone, "the appearance term must decide at least one assignment, or this test shows nothing"
        out = str(tmp_path / (name + ".json"))
        os.makedirs(out)
        p = subprocess.run([BIN, "--video", path, "--write_json", out] + flags, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        files = sorted(glob.glob(os.path.join(out, "*.json")))
        assert len(files) == N
        assert [[b["id"] for b in json.load(open(f))["bodies"]] for f in files] == want, name
    p = subprocess.run([BIN] + DRY + ["--write_json", str(tmp_path / "bad"), "--num_gpu", "2", "--track", "--track_appearance", "--appearance_parts", "1,2,40"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--appearance_parts" in p.stderr and "18 parts" in p.stderr, p.stderr[-500:]


def _case_file(path):
    """the cases and the host definitions' own results as the replay program reads them (tests/helpers/appear_check.cpp)"""
    import caffe_rtpose_amd as r

    def head(f, P, cfg, track, frames):
        a, t = ar.config(**cfg), tr.config(**track)
        plist = a["parts"]
        f.write(struct.pack("<ii", P, -1 if plist is None else len(plist)) + (np.asarray(plist, np.int32).tobytes() if plist else b""))
        f.write(struct.pack("<fiffffi", a["min_score"], a["min_parts"], a["margin"], a["weight"], a["max_dist"], a["unknown"], a["rate"]))
        f.write(struct.pack("<fiifii", t["min_score"], t["min_parts"], t["min_common"], t["max_cost"], t["max_misses"], frames))

    def frame(f, P, joints, num_people, image, desc, recs):
        j = np.ascontiguousarray(joints, np.float32).reshape(-1, P, 3)
        f.write(struct.pack("<ii", len(j) if num_people is None else num_people, len(j)) + j.tobytes())
        if image is None:
            f.write(struct.pack("<iii", 0, 0, 0))
        else:
            img = np.ascontiguousarray(image, np.uint8)
            f.write(struct.pack("<ii", img.shape[1], img.shape[0]) + img.tobytes() + struct.pack("<i", len(desc[1])) + desc[0].tobytes() + desc[1].tobytes())
        f.write(struct.pack("<i", -1) if recs is None else struct.pack("<i", len(recs)) + np.ascontiguousarray(recs, np.int32).tobytes())

    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(DESCRIBE_CASES) + len(UPDATE_CASES)))
        for case in DESCRIBE_CASES:
            head(f, case["P"], case["cfg"], {}, 1)
            frame(f, case["P"], case["joints"], None, case["image"], r.appearance_describe(case["image"], case["joints"], case["P"], r.appearance_config(**case["cfg"])), None)
        for case in UPDATE_CASES:
            head(f, case["P"], case["cfg"], case["track"], len(case["frames"]))
            for (joints, num_people, image), (recs, _, _, desc) in zip(case["frames"], replay_host(case)):
                frame(f, case["P"], joints, num_people, image, desc, recs)


def test_host_definitions_are_clean_under_sanitizers(tmp_path):
    """tests/helpers/appear_check.cpp (its own main) replays every case through rtp_appearance_describe and rtp_track_update_appearance
    on exactly-sized heap blocks and compares with the results this process got: an element read or written outside a block is an
    AddressSanitizer report.  Built with the host-only sources; nothing is loaded into python."""
    csrc = os.path.join(ROOT, "caffe_rtpose_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "helpers", "appear_check.cpp")] + [os.path.join(csrc, f) for f in ("codecs.cpp", "preprocess.cpp", "host_util.cpp")]
    exe = str(tmp_path / "appear_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-o", exe] + src + ["-lpthread", "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    data = str(tmp_path / "cases.bin")
    _case_file(data)
    q = subprocess.run([exe, data], capture_output=True, text=True, timeout=300, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert q.returncode == 0, q.stdout[-2000:] + q.stderr[-3000:]
    assert not [ln for ln in q.stderr.splitlines() if "Sanitizer" in ln or "runtime error:" in ln], q.stderr[-3000:]
    assert f"appear_check OK: {len(DESCRIBE_CASES) + len(UPDATE_CASES)} cases" in q.stdout

"""The matrix of tests/test_postproc_sizes.py (tests/_postcases.py) on the CPU: what it reaches, and that its inputs are what they claim to be.

The post-processing kernels (csrc/postproc.hip) have branches that depend on max_peaks and on the thresholds and that the built-in sizes
(max_peaks 64 / 20, default thresholds) never take:

  B1  launch_connect_impl: more than 64 KiB of sort keys (max_peaks >= 91)
  B2  connect_match_limb: the bitonic sort over 8192 and over 16384 keys (a limb with more than 4096 / 8192 surviving pairs)
  B3  greedy scan: the second occupancy word, key fields above 64
  B4  the assemble kernel without its LDS copy (COCO, max_peaks >= 121)
  B5  blk_off up to index 64 (a limb with more than 16128 pairs: 127 x 127)
  B6  conn_of / matched above 64; a limb with more than 64 peaks at one end only (COCO: "not yet held"; MPI: appends all)
  B7  the pair kernel's early exit with allowed_fail other than 0 and 1: 2..9, and negative (inter_min_above >= 10)
  B8  emission: the max_people cap in a later 256-row chunk than the first
  B9  max_peaks 1 and 2
  B10 fused NMS: a strip skipped whole, a strip with skipped AND evaluated columns, thresholds <= 0

1. Every one of them is reached by at least one (engine, input, threshold set) of the matrix, by its predicate in _postcases.py — a Python
   restatement of the kernel's condition on the oracle's decision trace.  Taking an engine out of the matrix fails this test for the branch
   the engine was there for.
2. No input is silently empty, and the oracle accepts every case (so the GPU file needs no `try`), including the 17 cases of
   test_gpu_parity.test_fused_postproc_from_lowres_bit_exact.
3. The premise of the NMS skip, |resized| <= 1.95 * max|low-res|, on adversarial sign patterns: a statement about the reference's
   arithmetic, not about the kernel.
4. The plan's contract for max_peaks: [1, 127], anything else is RTP_EINVAL."""
import numpy as np
import pytest

import _oracle as orc
import _postcases as pc


def _r():
    import caffe_rtpose_amd as r
    return r


@pytest.fixture(scope="module")
def all_facts():
    return [pc.facts(engine, name, thr) for engine, name, sets in pc.CASES for thr in sets]


def test_matrix_has_the_engines_display_sizes_and_threshold_sets_it_documents():
    coco = sorted(mp for m, mp, _, N, _ in pc.ENGINES.values() if m == 0 and N == 1)
    mpi = sorted(mp for m, mp, _, N, _ in pc.ENGINES.values() if m == 1)
    assert coco == [1, 2, 63, 65, 90, 91, 120, 121, 127] and mpi == [1, 19, 64, 127]
    assert [(mp, N, gap) for m, mp, _, N, gap in pc.ENGINES.values() if N > 1] == [(127, 3, 0.15)]
    assert {d for _, _, d, _, _ in pc.ENGINES.values()} == {(1280, 720), (333, 201), (640, 360), (1920, 1080)}
    assert len({(c[0], c[1]) for c in pc.CASES}) == len(pc.CASES) and {c[0] for c in pc.CASES} == set(pc.ENGINES)
    used = {t for c in pc.CASES for t in c[2]}
    assert used == set(pc.THRESHOLDS), set(pc.THRESHOLDS) - used       # every threshold set runs somewhere
    assert all(c[2][0] == "default" or c[1].startswith("straddle") for c in pc.CASES)
    for engine, name, _ in pc.CASES:                                   # P = 40 only where 40 people fit under the cap
        assert name != "people40" or pc.ENGINES[engine][1] >= 63


def test_every_branch_is_reached(all_facts):
    def who(pred):
        return [(f["engine"], f["input"], f["thr"]) for f in all_facts if pred(f)]

    own = {"straddle05": "nms005", "straddle20": "nms02", "straddle50": "nms05"}
    reached = {
        "B1": who(pc.b1),
        "B2 8192 keys": who(lambda f: pc.b2(f, 8192)),
        "B2 16384 keys": who(lambda f: pc.b2(f, 16384)),
        "B3": who(pc.b3),
        "B3 ties above 64": who(lambda f: f["tied_above_64"] and pc.b3(f)),
        "B4": who(pc.b4),
        "B4 with the cap in a later chunk": who(lambda f: pc.b4(f) and pc.b8(f)),
        "B5": who(pc.b5),
        "B6 COCO": who(lambda f: f["model"] == 0 and pc.b6(f)),
        "B6 MPI": who(lambda f: f["model"] == 1 and pc.b6(f)),
        "B8": who(pc.b8),
        "B9 max_peaks 1": who(lambda f: f["max_peaks"] == 1 and pc.b9(f)),
        "B9 max_peaks 2": who(lambda f: f["max_peaks"] == 2 and pc.b9(f)),
        "B10 strip skipped": who(lambda f: pc.b10(f)[0]),
        "B10 columns skipped and evaluated": who(lambda f: pc.b10(f)[1]),
        "B10 threshold <= 0": who(lambda f: pc.b10(f)[2]),
        "B10 straddle at its own threshold": who(lambda f: own.get(f["input"]) == f["thr"] and pc.b10(f)[1]),
    }
    for v in (9, 5, 2, -1, -3):                                        # inter_min_above 0, 4, 7, 10, 12
        reached[f"B7 allowed_fail {v}"] = who(lambda f: pc.b7(f) == v)
    for name, cases in reached.items():
        print(f"{name}: {len(cases)} runs, e.g. {cases[:2]}")
    missing = [name for name, cases in reached.items() if not cases]
    assert not missing, missing
    # B1 / B4 sit between the engines that were chosen for them
    assert not any(pc.b1(f) for f in all_facts if f["max_peaks"] <= 90) and all(pc.b1(f) for f in all_facts if f["max_peaks"] >= 91)
    assert not any(pc.b4(f) for f in all_facts if f["max_peaks"] <= 120) and not any(pc.b4(f) for f in all_facts if f["model"] == 1)
    assert all(pc.b4(f) for f in all_facts if f["model"] == 0 and f["max_peaks"] >= 121)
    # the figures of the largest case, re-derived at this net size: almost every pair of a limb survives, every limb connects all its peaks
    big = [f for f in all_facts if (f["engine"], f["input"], f["thr"]) == ("coco127", "noise", "above0")][0]
    assert big["survivors"].max() > 15000 and len(big["conn"]) == 19 * 127 and (big["conn"][:, 1] > 64).sum() > 1000 and big["n"] == pc.MAX_PEOPLE
    # early exit and no connection at all: inter_min_above >= 10
    for f in all_facts:
        if pc.b7(f) is not None and pc.b7(f) < 0:
            assert len(f["conn"]) == 0 and f["survivors"].sum() == 0


def test_no_case_is_silently_empty(all_facts):
    for f in all_facts:
        key = (f["engine"], f["input"], f["thr"])
        if f["input"].startswith("people"):
            assert f["n"] >= 1, key
        if f["input"] == "noise":
            assert (f["counts"] >= max(f["max_peaks"], 128)).all(), (key, f["counts"].min())
        if f["input"] == "late_cap":
            assert len(f["rows"]) > 256 and not f["rows"][:256, f["num_parts"] + 2].any() and len(f["kept"]) > pc.MAX_PEOPLE, key
            assert f["kept"][pc.MAX_PEOPLE - 1] >= 256 and f["n"] == pc.MAX_PEOPLE, key
        if f["input"] == "ties":
            assert f["tied_above_64"] or f["max_peaks"] <= 64, key
            assert f["n"] >= 1 and f["counts"].max() == f["max_peaks"], key
        if f["input"] == "single_sided":
            chains = [c for c in pc.one_sided_chains(f) if c["n"] > 1]
            assert len(chains) >= (3 if f["model"] == 0 else 1), key                     # COCO: parts 2 and 5, and part 1 (all held)
            assert len(f["rows"]) <= pc.MAX_PEOPLE, key                                   # the cap never hides a row
            if f["thr"] == "sub1_0":                                                     # every row is kept: the one-part rows come out
                assert f["n"] == len(f["rows"]), key
                far = [c for c in chains if c["n"] >= min(f["max_peaks"], 70)]
                assert len(far) == (2 if f["model"] == 0 else 1), key
                for c in far:
                    assert c["emitted"] == c["appended"], (key, c)
                    if f["model"] == 0:
                        assert len(c["appended"]) == c["n"] - len(c["held"]) > 0, (key, c)
                    else:   # MPI appends all n; the single peaks of parts 5 and 14 may each extend one of these rows, which then has two parts
                        assert c["n"] - 2 <= len(c["appended"]) <= c["n"] and len(c["held"]) + len(c["appended"]) > c["n"], (key, c)
                    if f["max_peaks"] > 64:
                        assert any(o > 64 for o in c["emitted"]), (key, c)
                    if f["model"] == 0:                                                  # the filter had ordinals on both sides of 64 to filter and to pass
                        assert min(c["held"]) < 64 and min(c["emitted"]) < 64 and not set(c["held"]) & set(c["appended"]), (key, c)
                    if f["model"] == 0 and f["max_peaks"] >= 70:
                        assert sum(o > 64 for o in c["held"]) == 4 and sum(o > 64 for o in c["emitted"]) == 2, (key, c)
                if f["model"] == 0:   # every held ordinal above 64, appended by mistake, would be emitted as well
                    assert len(f["rows"]) + sum(sum(o > 64 for o in c["held"]) for c in far) <= pc.MAX_PEOPLE, key
        if f["input"].startswith("straddle"):
            assert f["n"] >= 1 or f["thresholds"]["nms_threshold"] < pc.thresholds(f["engine"], "default")["nms_threshold"], key
    # every case has people under at least one of its threshold sets (inter_min_above >= 10 is meant to give none)
    for engine, name, sets in pc.CASES:
        ns = {f["thr"]: f["n"] for f in all_facts if (f["engine"], f["input"]) == (engine, name)}
        assert max(ns.values()) >= 1, (engine, name, ns)
        assert all(n == 0 for t, n in ns.items() if t in ("above10", "above12")), (engine, name, ns)


def test_oracle_accepts_every_case():
    for engine, name, sets in pc.CASES:
        for thr in sets:
            assert pc.reference(engine, name, thr)[2] >= 0, (engine, name, thr)       # (orc.connect itself asserts that the oracle did not refuse)
    inp = pc.inputs("mpi127", "ties")                                   # MPI does not clamp: no PAF sample may leave the map
    assert inp["peaks"][:, 1:, 0].max() < pc.NET_W - 1 and inp["peaks"][:, 1:, 1].max() < pc.NET_H - 1


def test_oracle_accepts_the_existing_fused_cases():
    """test_fused_postproc_from_lowres_bit_exact used to drop its connect comparison wherever orc.connect raised: it raises for none of the 17."""
    import test_gpu_parity as g
    refused = []
    for case in g.FUSED_CASES:
        model, W, H, N, start, gap, kind = case
        num_parts, num_limbs, _, _ = orc.model_tables(model)
        mp = 64 if model == 0 else 20
        low = pc.fused_case_input(model, W, H, N, start, gap, kind)      # the function the GPU test builds its input with
        res = orc.imresize(low, W, H, start, gap)[0]
        thr = orc.default_thresholds(model)
        peaks = orc.nms(res, num_parts, mp, thr["nms_threshold"])
        try:
            orc.connect(model, res, peaks, mp, W, H, 1280, 720, thr)
        except AssertionError:                                          # orc.connect: "oracle connect failed"
            refused.append(case)
    assert len(g.FUSED_CASES) == 17 and refused == []


def _sign_patterns(h, w, nrandom=23):
    """80 low-res planes of +-1: checkerboards of period 1 and 2 in every phase, separable (49, the constant plane among them) and diagonal (8), and random signs"""
    y, x = np.mgrid[0:h, 0:w]
    axis = lambda t: [np.ones_like(t)] + [1 - 2 * ((t + p) % 2) for p in range(2)] + [1 - 2 * (((t + p) // 2) % 2) for p in range(4)]
    pats = [a * b for a in axis(y) for b in axis(x)]
    pats += [1 - 2 * (((x + y + p) // 2) % 2) for p in range(4)] + [1 - 2 * (((x - y + p) // 2) % 2) for p in range(4)]
    rs = np.random.RandomState(1)
    pats += [rs.choice([-1, 1], (h, w)) for _ in range(nrandom)]
    return np.stack(pats).astype(np.float32)


def test_premise_of_the_nms_skip_holds_for_the_reference_resize():
    """nms_fused_strip_kernel does not evaluate what NMS_BOUND (1.95) * max|low-res neighbourhood| says cannot exceed the threshold.  The bound
    is 1.375^2 = 1.89 in exact arithmetic; here the reference's own ImResize on the sign patterns that maximise a bicubic overshoot, for every
    start scale / gap / size of test_resize_bit_exact (per scale a different phase of the pattern set): measured worst ratio 1.71."""
    import test_gpu_parity as g
    worst = 0.0
    for _, W, H, N, start, gap in sorted(set((0,) + c[1:] for c in g.RESIZE_CASES)):
        h, w = H // 8, W // 8
        pats = _sign_patterns(h, w)
        for c0 in range(0, len(pats), 20):                              # 20 planes a call: the 1312x736 output stays small
            chunk = pats[c0:c0 + 20]
            low = np.ascontiguousarray(np.stack([np.roll(chunk, n, axis=2) for n in range(N)]))   # [N][C][h][w]
            res = orc.imresize(low, W, H, start, gap)[0]
            ratio = np.abs(res).reshape(len(chunk), -1).max(axis=1) / np.abs(low).max(axis=(0, 2, 3))
            worst = max(worst, float(ratio.max()))
    print(f"worst |resized| / max|low-res| = {worst:.4f}")
    assert worst <= 1.95
    assert worst > 1.25                                                  # the patterns do overshoot: the test is about something


def test_plan_accepts_max_peaks_1_to_127_only(tmp_path):
    r = _r()
    for model, parts in ((0, 18), (1, 15)):
        for mp in (1, 127):
            line0 = r.plan_summary(r.Config(model=model, proto_path=pc.proto_file(model, mp), net_w=pc.NET_W, net_h=pc.NET_H, precision=r.PREC_FP16,
                                            frames_in_flight=1)).split("\n")[0]
            assert f"parts {parts} max_peaks {mp} " in line0, line0
            assert r.prototxt_summary(pc.proto_file(model, mp))["max_peaks"] == mp
        for mp in (0, 128, 1000, -1):
            with pytest.raises(r.RtpError) as ei:
                r.plan_summary(r.Config(model=model, proto_path=pc.proto_file(model, mp), net_w=pc.NET_W, net_h=pc.NET_H, precision=r.PREC_FP16, frames_in_flight=1))
            assert ei.value.code == r.RTP_EINVAL, (model, mp)
    # the engines of the matrix plan the cheapest way and report their own max_peaks
    for name, (model, mp, disp, N, gap) in pc.ENGINES.items():
        assert f" max_peaks {mp} " in r.plan_summary(pc.config(name)).split("\n")[0]


def test_lds_formulas_of_the_predicates_match_the_boundaries_of_the_issue():
    assert [mp for mp in range(1, 128) if pc.sort_keys(mp) * 8 > 64 * 1024][0] == 91
    assert [mp for mp in range(1, 128) if not pc.assemble_preload(0, mp)][0] == 121
    assert all(pc.assemble_preload(1, mp) for mp in range(1, 128))
    assert pc.sort_keys(127) == 16384 and pc.sort_keys(1) == 64 and pc.sort_keys(90) * 8 == 64 * 1024
    assert pc.sort_keys(127) * 8 <= pc.K_POST_DYN_LDS_MAX

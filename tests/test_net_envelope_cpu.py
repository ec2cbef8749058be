"""The smallest and the widest nets the plan accepts, on the CPU (tests/_edgecases.py; the GPU half is tests/test_net_envelope.py).

1. The envelope itself: 16x16 is accepted, sizes that are no positive multiple of 16 are RTP_EINVAL, width 2736 is accepted and 2752 refused with
   a message that names the width — for one and for three scales, for both models.
2. The strip rule.  rtp_plan_summary's `postproc strip_rows R nstrips S max_rows M` line says what Builder::postproc_sizes chose; it must equal
   the rule restated in _edgecases.strip_rows on both sides of every halving (1360 | 1376, 1920 | 1936, 2400 | 2416) and at the ends.
3. The arithmetic of nms_fused_strip_kernel's LDS carve over EVERY accepted width: the dynamic LDS within 150 KiB, the rows of a strip within
   ytab[24], the ballots and their prefix within the eight rows of T they reuse.
4. The convolution machinery on the extreme plans: the tile walks of tests/_convcheck.py match every launch's workgroup count, and the four
   kernel classes that only these plans run are reached by CONV_EDGE and by none of the four older matrices (a plan_keys difference).
5. The inputs of the GPU file are what they claim to be: the oracle accepts all but the portrait 16x32, the wide noise maps exercise the
   max_peaks cap and hold people, the tiny ones hold what maps of 2x2 to 6x2 can, and the two straddle inputs reach all three kinds of strip
   (skipped whole, some columns skipped, evaluated in full) at the strip height of their plan.  Conditions on inputs, not measurements."""
import numpy as np
import pytest

import _convcheck as cc
import _edgecases as ec
import _manycases as mc
import _oracle as orc
import _postcases as pc

BOUNDARY_WIDTHS = (16, 656, 1312, 1360, 1376, 1920, 1936, 2400, 2416, 2736)
# the issue's table, literally: scales class -> [(first width, last width, strip rows)]
STRIP_TABLE = {1: [(16, 1920, 8), (1936, 2400, 4), (2416, 2736, 2)],
               2: [(16, 1360, 16), (1376, 1920, 8), (1936, 2400, 4), (2416, 2736, 2)]}


def _r():
    import caffe_rtpose_amd as r
    return r


@pytest.fixture(scope="module")
def graphs():
    return {m: cc.builtin_graph(m) for m in (0, 1)}


def _summary(W, H, N=1, model=0, **kw):
    r = _r()
    return r.plan_summary(r.Config(model=model, net_w=W, net_h=H, num_scales=N, scale_gap=0.3 if N < 3 else 0.15, **kw))


# ------------------------------------------------------------------------------------------
# 1. the envelope
# ------------------------------------------------------------------------------------------
def test_smallest_net_is_accepted_and_sizes_off_the_grid_are_refused():
    r = _r()
    lines = _summary(16, 16).splitlines()
    assert [ln for ln in lines if ln.startswith("level ")] == ["level 0 H 16 W 16 halo 1", "level 1 H 8 W 8 halo 1", "level 2 H 4 W 4 halo 1", "level 3 H 2 W 2 halo 3"]
    assert len([ln for ln in lines if ln.startswith("step pool ")]) == 3          # narrower than 128 at every level: no pooling epilogue
    for bad in (0, 8, 24, -16, -1):
        for w, h in ((bad, 16), (16, bad), (bad, bad)):
            with pytest.raises(r.RtpError) as ei:
                _summary(w, h)
            assert ei.value.code == r.RTP_EINVAL, (w, h)
            assert f"{w}x{h}" in str(ei.value), ei.value


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("N", [1, 3])
def test_widest_net_is_2736_and_the_refusal_names_the_width(model, N):
    r = _r()
    assert ec.summary_postproc(_summary(ec.MAX_W, 16, N, model))[0] == 2
    with pytest.raises(r.RtpError) as ei:
        _summary(ec.MAX_W + 16, 16, N, model)
    assert ei.value.code == r.RTP_EINVAL
    assert "2752" in str(ei.value) and "strip kernel" in str(ei.value), ei.value
    assert ec.strip_rows(ec.MAX_W, N) == 2 and ec.strip_rows(ec.MAX_W + 16, N) is None
    assert _summary(ec.MAX_W, 16, N, model, precision=r.PREC_FP32)                # (the arenas and tiles of the widest fp32 plan exist too)


# ------------------------------------------------------------------------------------------
# 2. the strip rule
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("W", BOUNDARY_WIDTHS)
def test_postproc_line_equals_the_strip_rule(W, N):
    summary = _summary(W, 32, N)
    lines = summary.splitlines()
    post = [i for i, ln in enumerate(lines) if ln.startswith("postproc ")]
    levels = [i for i, ln in enumerate(lines) if ln.startswith("level ")]
    assert len(post) == 1 and post[0] > max(levels) and post[0] > 0, "one `postproc` line, behind the `level` lines, never the first line"
    assert lines[post[0]] == ec.postproc_line(W, 32, N)
    rows, nstrips, max_rows = ec.summary_postproc(summary)
    assert rows == [r_ for lo, hi, r_ in STRIP_TABLE[N] if lo <= W <= hi][0]
    assert nstrips * rows == 32 and max_rows == 19 * 64                           # H / strip_rows with no remainder
    # other heights: the last strip may be short
    for H in (16, 48, 80):
        r2, n2, _ = ec.summary_postproc(_summary(W, H, N))
        assert r2 == rows and n2 == -(-H // rows)
    # the model's own limb count and cap
    assert ec.summary_postproc(_summary(W, 32, N, model=1))[2] == 14 * 20
    assert lines[post[0]].replace("1216", "280") == ec.postproc_line(W, 32, N, model=1)


def test_strip_rule_has_the_boundaries_of_the_table():
    for N, table in STRIP_TABLE.items():
        for W in range(ec.MIN_W, ec.MAX_W + 16, 16):
            assert ec.strip_rows(W, N) == [r_ for lo, hi, r_ in table if lo <= W <= hi][0], (W, N)
    assert ec.strip_rows(1360, 3) == 16 and ec.strip_rows(1376, 16) == 8          # "several scales" is one class


# ------------------------------------------------------------------------------------------
# 3. whole-envelope arithmetic of the strip kernel's LDS carve
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2])
def test_strip_kernel_lds_carve_fits_at_every_accepted_width(N):
    seen = set()
    for W in range(ec.MIN_W, ec.MAX_W + 16, 16):
        rows, nstrips, _ = ec.summary_postproc(_summary(W, 16, N))
        assert rows == ec.strip_rows(W, N) and nstrips == -(-16 // rows)
        seen.add(rows)
        assert ec.strip_lds(rows, W) <= ec.STRIP_LDS_CAP, W                     # the dynamic LDS of the launch
        assert ec.strip_lds(rows, W) <= pc.K_POST_DYN_LDS_MAX, W                # launch_nms_fused refuses above this
        assert rows + 2 <= ec.YTAB_ROWS, W                                      # ytab[24]: one entry per row held (strip rows + one above + one below)
        assert ec.ballot_bytes(rows, W) <= 4 * ec.NMSF_TROWS * W, W             # bals [nr][NG] + gbase [nr * NG + 1] reuse T's 32 * W bytes
    assert seen == ({8, 4, 2} if N == 1 else {16, 8, 4, 2})
    assert ec.strip_lds(2, ec.MAX_W + 16) > ec.STRIP_LDS_CAP                     # what the refusal is for


# ------------------------------------------------------------------------------------------
# 4. the convolution machinery on the extreme plans
# ------------------------------------------------------------------------------------------
def _edge_plans(graphs):
    r = _r()
    plans = [(name, graphs[c[1]], c[4], c[6], r.plan_summary(cc.matrix_config(name, ec.CONV_EDGE))) for name, c in ec.CONV_EDGE.items()]
    plans += [(name + " (batch)", graphs[c[1]], c[4], c[6], r.plan_summary(cc.batch_config(name, matrix=ec.BATCH_EDGE))) for name, c in ec.BATCH_EDGE.items()]
    return plans


def test_edge_matrices_have_the_entries_of_the_issue():
    want = [("mixed", 0, 16, 16, 1, 1), ("mixed", 1, 16, 16, 3, 3), ("fp32", 0, 16, 16, 1, 1), ("f16x3", 0, 32, 16, 1, 1), ("fp16", 0, 16, 32, 1, 2),
            ("mixed", 0, 16, 512, 1, 1), ("mixed", 0, 2736, 16, 1, 1), ("mixed", 0, 1936, 16, 1, 1), ("mixed", 0, 1376, 16, 2, 1), ("fp32", 0, 2736, 16, 1, 1)]
    assert [(m, mdl, w, h, n, b) for m, mdl, w, h, n, gap, b, seed in ec.CONV_EDGE.values()] == want
    batched = [c for c in ec.CONV_EDGE.values() if c[6] > 1]
    assert list(ec.BATCH_EDGE.values())[:len(batched)] == batched
    assert [(m, mdl, w, h, n, b) for m, mdl, w, h, n, gap, b, seed in list(ec.BATCH_EDGE.values())[len(batched):]] == [("mixed", 0, 16, 16, 1, 5)]
    assert len(set(ec.POST_EDGE)) == len(ec.POST_EDGE) == 13 and ec.POST_ERANGE in ec.POST_EDGE
    assert [(c[1], c[2]) for c in ec.STRADDLE_EDGE] == [(1936, 48), (2416, 48)]


def test_tile_walks_match_the_workgroup_counts_of_the_edge_plans(graphs):
    """the body of test_conv_launches_cpu.test_tile_walks_match_the_workgroup_counts_of_the_plan over CONV_EDGE and BATCH_EDGE: the float64 checker
    samples the first and last pixel of every workgroup's tile from these walks"""
    pools = {}
    for name, g, n, b, summary in _edge_plans(graphs):
        levels, launches = cc.parse_plan(summary)
        pools[name] = len([L for L in launches if L.kind == "pool"])
        for L in launches:
            if L.kind == "pool":
                continue
            hh, ww, halo = levels[g.level[g.convs[L.layers[0]]["bottom"]]]
            if L.kind == "first":
                assert L.wgs == hh * n * b
                continue
            ends, nt = cc.pool_tile_ends(hh, ww, L.k, L.tile[0]) if L.pool else cc.plain_tile_ends(hh, ww, halo, L.tile[0])
            assert L.wgs == nt * n * b * (L.coutp // L.tile[1]) * len(L.layers), (name, L)
            lim = (hh // 2, ww // 2) if L.pool else (hh, ww)
            assert ends and all(0 <= y < lim[0] and 0 <= x < lim[1] for y, x in ends), (name, L)
    # nets narrower than 128 at a level pool in a step of their own (three of them at 16x16), the wide ones fuse two pools
    assert pools["mixed_coco_16x16"] == pools["fp32_coco_16x16"] == pools["mixed_coco_16x16_b5 (batch)"] == 3
    assert pools["mixed_coco_2736x16"] == pools["mixed_coco_1936x16"] == 1


def test_edge_plans_reach_four_kernel_classes_that_no_older_matrix_reaches(graphs):
    r = _r()
    old = set()
    for name, c in cc.MATRIX.items():
        old |= cc.plan_keys(r.plan_summary(cc.matrix_config(name)), graphs[c[1]])
    for name, c in cc.BATCH_MATRIX.items():
        old |= cc.plan_keys(r.plan_summary(cc.batch_config(name)), graphs[c[1]])
    for name, c in mc.CONV_MATRIX.items():
        old |= cc.plan_keys(r.plan_summary(cc.matrix_config(name, mc.CONV_MATRIX)), graphs[c[1]])
    for name, c in mc.BATCH_MATRIX.items():
        old |= cc.plan_keys(r.plan_summary(cc.batch_config(name, matrix=mc.BATCH_MATRIX)), graphs[c[1]])
    new = {}
    for name, c in ec.CONV_EDGE.items():
        for k in cc.plan_keys(r.plan_summary(cc.matrix_config(name, ec.CONV_EDGE)), graphs[c[1]]) - old:
            new.setdefault(cc.key_str(k), []).append(name)
    for cls, names in new.items():
        print(f"{cls}: {names}")
    assert new == dict(ec.EDGE_ONLY_CLASSES)
    assert not any(cc.key_str(k) in ec.EDGE_ONLY_CLASSES for k in old)


# ------------------------------------------------------------------------------------------
# 5. the inputs of the GPU file
# ------------------------------------------------------------------------------------------
def test_oracle_accepts_every_post_edge_input_but_the_portrait_one():
    for case in ec.POST_EDGE + ec.STRADDLE_EDGE:
        res, peaks, n, joints = ec.post_reference(case)
        model, W, H = case[:3]
        assert res.shape == (pc._dims(model)[2], H, W) and ec.post_input(case).shape == (case[3], pc._dims(model)[2], H // 8, W // 8)
        assert (n is None) == (case == ec.POST_ERANGE), (case, n)                # 16x32: the oracle's connect fails its range check
        assert not np.array_equal(peaks, ec.stale_peaks(model))


def test_wide_noise_inputs_exercise_the_cap_and_hold_people():
    for case in ec.POST_WIDE_NOISE + ec.POST_LAST_BEFORE_HALVING + ec.POST_MPI:
        _, peaks, n, _ = ec.post_reference(case)
        assert peaks[:, 0, 0].max() >= ec.max_peaks(case[0]), (case, peaks[:, 0, 0].max())
        assert n >= 1, case
    for case in ec.POST_WIDE_NOISE:                                               # every part has more maxima than the cap
        assert ec.post_reference(case)[1][:, 0, 0].min() > ec.max_peaks(case[0]), case


def test_tiny_inputs_hold_what_such_maps_can():
    by_size = {(c[1], c[2]): ec.post_reference(c) for c in ec.POST_TINY_NOISE}
    assert by_size[(32, 16)][2] >= 1 and by_size[(48, 16)][2] >= 1               # at least one person
    assert by_size[(16, 16)][1][:, 0, 0].max() >= 1                               # at least one part with a peak
    assert ec.post_reference(ec.POST_ERANGE)[1][:, 0, 0].max() >= 1


@pytest.mark.parametrize("case", ec.STRADDLE_EDGE, ids=ec.post_id)
def test_straddle_inputs_reach_every_kind_of_strip_at_their_plans_strip_height(case):
    model, W, H, N, start, gap, _ = case
    rows, nstrips, _ = ec.summary_postproc(_summary(W, H, N, model))
    assert rows == {1936: 4, 2416: 2}[W] and nstrips * rows == H
    thr = orc.default_thresholds(model)["nms_threshold"]
    whole, mixed, full = pc.nms_skip_stats(ec.post_input(case), pc._dims(model)[0], thr, strip_rows=rows)
    print(f"{ec.post_id(case)}: {rows}-row strips: {whole} skipped whole, {mixed} with skipped and evaluated columns, {full} evaluated in full")
    assert whole > 0 and mixed > 0 and full > 0
    assert whole + mixed + full <= pc._dims(model)[0] * nstrips
    assert ec.post_reference(case)[1][:, 0, 0].max() >= 1                         # the Gaussians across the seam are peaks

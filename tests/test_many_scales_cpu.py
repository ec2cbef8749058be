"""The cases of tests/test_many_scales.py (tests/_manycases.py) on the CPU: what they reach, and that the references accept them.

1. Pre-processing.  launch_area_pad runs one launch per group of four scales.  From the host's level geometry: 5, 9 and 16 scales are the group
   shapes 4 + 1, 4 + 4 + 1 and 4 x 4; identity, integer-fast, fractional-area and enlarging (`linear`) levels each occur in a group OTHER than
   the first; one display equals the net, one is smaller, one is a plain down-scale.  rtp_preprocess_frame — the reference of the GPU test —
   writes levels of exactly that geometry: the padded region is zero, the interior is not constant, and it equals the independent OpenCV
   restatement (tests/_cvref.py) on every case.
2. Post-processing.  The oracle accepts every ImResize and every fused case; people cases emit people; the scale counts, a start scale below 1,
   the MPI model and the 2x2-crop geometry are among them; at that geometry EVERY output pixel has an active neighbour clamp in axis_nb; some case
   has a peak whose 7x7 window overlaps the clamp region of the smallest crop and an accepted connection with a summed PAF sample there
   (predicates on the oracle's trace).
3. The premise of the fused NMS kernel's strip skip, |resized| <= 1.95 * max|low-res|, at these geometries on adversarial sign patterns — a
   statement about the reference's arithmetic.  Measured worst ratio 1.56 (1.71 at the geometries of test_resize_bit_exact,
   tests/test_postproc_sizes_cpu.py): averaging over up to 16 differently phased scales overshoots less than one scale does.
4. Configuration: 16 scales and batch_frames 16 are planned, 17 of either are refused."""
import numpy as np
import pytest

import _manycases as mc
import _oracle as orc


def _r():
    import caffe_rtpose_amd as r
    return r


# ------------------------------------------------------------------------------------------
# 1. pre-processing
# ------------------------------------------------------------------------------------------
def test_preprocess_cases_put_every_level_kind_into_a_later_group():
    assert mc.PREP_SCALES == (5, 9, 16) and mc.PREP_NET == (160, 96)
    assert [-(-N // 4) for N in mc.PREP_SCALES] == [2, 3, 4] and [N % 4 for N in mc.PREP_SCALES] == [1, 1, 0]       # 4 + 1, 4 + 4 + 1 (partial last groups), 4 x 4
    d = mc.PREP_DISPLAYS
    assert d["display_is_net"] == mc.PREP_NET and d["display_below_net"][0] < 160 and d["display_below_net"][1] < 96
    assert d["downscale"][0] > 160 and d["downscale"][1] > 96
    assert len(mc.PREP_CASES) == 9 and {c[1] for c in mc.PREP_CASES} == set(mc.PREP_SCALES)
    later = {}
    for case in mc.PREP_CASES:
        for group, kind in mc.prep_kinds(case):
            if group >= 1:
                later.setdefault(kind, set()).add(case)
    assert set(later) == {"identity", "fast", "area", "linear"}, later.keys()
    # ... and in the partial last group of 5 = 4 + 1 and 9 = 4 + 4 + 1 something other than one kind
    assert {mc.prep_kinds(c)[-1][1] for c in mc.PREP_CASES if c[1] in (5, 9)} >= {"fast", "area"}
    # per display: what the case module says about it
    kinds = lambda name, N: [k for _, k in mc.prep_kinds((name, N))]
    assert kinds("display_is_net", 16)[:2] == ["identity", "identity"] and "identity" not in kinds("display_is_net", 16)[2:]
    assert set(kinds("downscale", 16)) == {"area"}
    below = mc.prep_kinds(("display_below_net", 16))
    assert {g for g, k in below if k == "linear"} == {0, 1} and {g for g, k in below if k == "identity"} == {1, 2} and {g for g, k in below if k == "fast"} == {3}
    assert ("display_below_net", 9) in later["identity"]          # the pipeline case of the GPU file
    # the smallest level is 16x16, the first 160x96
    for case in mc.PREP_CASES:
        sizes = mc.level_sizes(*mc.prep_geom(case)[4:])
        assert sizes[0] == (160, 96) and sizes[-1] == (16, 16) and all(a[0] >= b[0] and a[1] >= b[1] for a, b in zip(sizes, sizes[1:]))


def test_level_kind_restates_the_hosts_choice():
    """engine.cpp build_prep_tables takes identity / linear / rtp_internal_area_fast / the table path in this order; the fast path is cv::resize's
    is_area_fast: integer factors on both axes.  Checked here through the host resize: a `fast` level is the rounded block mean."""
    r = _r()
    rs = np.random.RandomState(4)
    for (dw, dh), (tw, th) in (((160, 96), (80, 48)), ((96, 64), (32, 16)), ((160, 96), (16, 16)), ((96, 64), (48, 32))):
        assert mc.level_kind(dw, dh, tw, th) == "fast"
        img = rs.randint(0, 256, (dh, dw, 3)).astype(np.uint8)
        fx, fy = dw // tw, dh // th
        blk = img.astype(np.int64).reshape(th, fy, tw, fx, 3).sum(axis=(1, 3))
        want = (blk + 2) >> 2 if (fx, fy) == (2, 2) else np.rint(blk.astype(np.float32) * np.float32(1.0 / (fx * fy))).astype(np.int64)
        assert np.array_equal(r.resize_area(img, tw, th), want.astype(np.uint8)), (dw, dh, tw, th)
    assert mc.level_kind(96, 64, 96, 64) == "identity" and mc.level_kind(96, 64, 112, 64) == "linear" and mc.level_kind(96, 64, 96, 80) == "linear"
    assert mc.level_kind(160, 96, 96, 64) == "area" and mc.level_kind(320, 180, 160, 96) == "area"


@pytest.mark.parametrize("case", mc.PREP_CASES, ids=lambda c: f"{c[0]}-{c[1]}s")
def test_host_preprocess_of_the_cases_has_the_level_geometry_and_equals_the_opencv_restatement(case):
    r = _r()
    import _cvref
    fw, fh, dw, dh, W, H, N, start, gap = mc.prep_geom(case)
    sizes = mc.level_sizes(W, H, N, start, gap)
    frames = mc.prep_frames(case)
    assert len(frames) == 2 and not np.array_equal(frames[0], frames[1])
    for img in frames:
        x, disp, fs = r.preprocess_frame(img, dw, dh, W, H, N, start, gap)
        want_x, want_disp, want_fs = _cvref.producer_frame(img, dw, dh, W, H, N, start, gap, orc.process_and_pad_image)
        assert fs == want_fs and np.array_equal(disp, want_disp) and np.array_equal(x, want_x)
        assert x.shape == (N, 3, H, W)
        for i, (tw, th) in enumerate(sizes):
            pw, ph = (W - tw) // 2, (H - th) // 2
            inside = np.zeros((H, W), bool)
            inside[ph:ph + th, pw:pw + tw] = True
            assert not x[i][:, ~inside].any(), (case, i)                              # the padded region is zero
            inner = x[i][:, ph:ph + th, pw:pw + tw]
            assert all(np.unique(inner[c]).size > 4 for c in range(3)), (case, i)     # the interior is not constant
        # no two levels of a group are equal where their sizes differ: a launch that wrote level i's pixels to slot j would show
        for i in range(N):
            for j in range(i):
                assert sizes[i] == sizes[j] or not np.array_equal(x[i], x[j])


# ------------------------------------------------------------------------------------------
# 2. post-processing
# ------------------------------------------------------------------------------------------
def test_resize_cases_cover_the_scale_counts_and_geometries():
    cases = mc.RESIZE_CASES
    assert {c[3] for c in cases} >= {4, 5, 7, 11, 13, 16}
    assert any(c[4] < 1.0 for c in cases) and any(c[0] == 1 for c in cases)
    assert (0, 160, 96, 16, 1.0, 0.06) in cases and (0, 64, 48, 16, 1.0, 0.06) in cases
    for model, W, H, N, start, gap in cases:
        assert start - (N - 1) * gap > 0.09
        sizes = mc.level_sizes(W, H, N, start, gap)
        assert all(tw <= W and th <= H for tw, th in sizes)                   # what rtp_set_scales / the producer accept
    # the 2x2-crop geometry: the last scale of 160x96 and of 64x48 at 16 scales keeps 2x2 of 20x12 / 8x6 low-res cells
    for W, H in ((160, 96), (64, 48)):
        padw, padh, ow, oh = mc.scale_geo(W // 8, H // 8, W, H, 1.0, 0.06, 15)[:4]
        assert (ow, oh) == (2, 2) and (padw, padh) == ((W // 8 - 2) // 2, (H // 8 - 2) // 2)
        assert mc.clamp_mask(W, H, 1.0, 0.06, 15).all()                        # every neighbour clamp of axis_nb is active at every output pixel
        assert not mc.clamp_mask(W, H, 1.0, 0.06, 0).all()                     # (the full-size scale clamps at the borders only)


def test_oracle_accepts_the_resize_cases():
    import _synth
    for model, W, H, N, start, gap in mc.RESIZE_CASES:
        C = 57 if model == 0 else 44
        low = _synth.smooth_field(N * C, H // 8, W // 8, seed=3).reshape(N, C, H // 8, W // 8)
        res = orc.imresize(low, W, H, start, gap)[0]
        assert res.shape == (C, H, W) and np.isfinite(res).all() and np.abs(res).max() > 0


def test_fused_cases_are_accepted_by_the_oracle_and_reach_the_clamp_region():
    cases = mc.FUSED_CASES
    assert {c[3] for c in cases} == {5, 9, 16}
    for kind in ("people5", "speople5", "noise"):
        assert {c[3] for c in cases if c[6] == kind} == {5, 9, 16}, kind
    assert {(c[1], c[2]) for c in cases} == {(160, 96), (320, 176), (64, 48)} and any(c[0] == 1 for c in cases)
    peak_hits, paf_hits = {}, {}
    for case in cases:
        ref = mc.fused_reference(case)                                        # (orc.connect_trace asserts that the oracle did not refuse)
        assert ref["n"] >= 0 and ref["res"].shape[1:] == (case[2], case[1])
        if case[6] != "noise":
            assert ref["n"] >= 1, case
        assert ref["peaks"][:, 0, 0].max() >= 1, case
        peak_hits[case] = mc.peaks_in_clamp_region(case)
        if case[0] == 0:
            paf_hits[case] = mc.kept_paf_samples_in_clamp_region(case)
    print({k: v for k, v in peak_hits.items() if v}, {k: v for k, v in paf_hits.items() if v})
    # At the 2x2 geometry the mask is all True, so the predicate is trivially met there: `two` only says that peaks and accepted connections EXIST where
    # every clamp is active.  The case that carries the weight is `wide` (320x176, a 4x4 crop at the end): the mask covers part of the map, and
    # peaks and summed PAF samples fall inside that part.
    two = (0, 160, 96, 16, 1.0, mc.gap(16), "speople5")
    assert peak_hits[two] > 0 and paf_hits[two] > 0 and mc.fused_reference(two)["n"] >= 1
    wide = (0, 320, 176, 16, 1.0, mc.gap(16), "people5")
    m = mc.clamp_mask(320, 176, 1.0, mc.gap(16), 15)
    assert 0.0 < m.mean() < 1.0 and peak_hits[wide] > 0 and paf_hits[wide] > 0
    assert len(mc.fused_reference(two)["conn"]) > 0


# ------------------------------------------------------------------------------------------
# 3. the premise of the strip skip at these geometries
# ------------------------------------------------------------------------------------------
def test_premise_of_the_nms_skip_holds_at_many_scales():
    """nms_fused_strip_kernel skips what NMS_BOUND (1.95) * max|low-res neighbourhood| says cannot exceed the threshold; 1.375^2 = 1.89 in exact
    arithmetic per scale, and the mean over scales cannot exceed the largest.  Here the reference's own ImResize on the sign patterns of
    tests/test_postproc_sizes_cpu.py (per scale another phase), at every geometry of RESIZE_CASES — crops of 2x2 cells included, where both
    neighbours on either side are clamped."""
    from test_postproc_sizes_cpu import _sign_patterns
    worst, per_case = 0.0, {}
    for _, W, H, N, start, gap in sorted(set((0,) + c[1:] for c in mc.RESIZE_CASES)):
        h, w = H // 8, W // 8
        pats = _sign_patterns(h, w)
        wc = 0.0
        for c0 in range(0, len(pats), 20):
            chunk = pats[c0:c0 + 20]
            for same in (False, True):      # another phase per scale, and the same pattern at every scale (each scale crops another part of it)
                low = np.ascontiguousarray(np.stack([chunk if same else np.roll(chunk, n, axis=2) for n in range(N)]))   # [N][C][h][w]
                res = orc.imresize(low, W, H, start, gap)[0]
                ratio = np.abs(res).reshape(len(chunk), -1).max(axis=1) / np.abs(low).max(axis=(0, 2, 3))
                wc = max(wc, float(ratio.max()))
        per_case[(W, H, N, start, gap)] = round(wc, 4)
        worst = max(worst, wc)
    print(f"worst |resized| / max|low-res| = {worst:.4f}", per_case)
    assert worst <= 1.95
    assert worst > 1.25                                                  # the patterns do overshoot: the test is about something


# ------------------------------------------------------------------------------------------
# 4. the accepted range
# ------------------------------------------------------------------------------------------
def test_plan_accepts_16_scales_and_batches_of_16_and_refuses_17():
    r = _r()
    ok = r.plan_summary(r.Config(net_w=64, net_h=48, num_scales=16, scale_gap=mc.gap(16), frames_in_flight=16, batch_frames=16))
    first = [ln for ln in ok.splitlines() if ln.startswith("step ") and " wgs " in ln][0].split()
    assert int(first[first.index("wgs") + 1]) % 256 == 0                     # 256 images in every launch
    for kw in (dict(num_scales=17, scale_gap=0.05), dict(batch_frames=17, frames_in_flight=17)):      # rtp_engine_create: argument errors come before the device is looked for
        with pytest.raises(r.RtpError) as ei:
            r.Engine(r.Config(**{**dict(net_w=64, net_h=48, num_scales=16, scale_gap=mc.gap(16), frames_in_flight=16, batch_frames=16), **kw}))
        assert ei.value.code == r.RTP_EINVAL, kw

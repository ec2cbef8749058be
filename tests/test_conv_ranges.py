"""Convolution launches at the edges of the fp8 and fp16 value ranges, each launch ALONE against float64 (tests/_convcheck.py, saturating=True).

Per case: one engine, the weight set of a range case (tests/_rangecases.py) written with rtp_set_conv_weights for every layer, one
rtp_forward_heatmaps, every launch checked element by element on the engine's own blobs — the body of tests/test_conv_launches.py with other weights.
tests/test_conv_ranges_cpu.py holds the same cases on the CPU: what they must reach, that the bound is sound on them, which defects it catches.

Plans: mixed coco 144x80 (every case); mixed mpi 96x64 (stand-alone q pooling steps, cout-28 tails); the custom graph `odd` under mixed @all (tensors
with a lo AND a q block, concat slices at odd channel offsets: the 8-aligned, 4-byte and single-byte q stores of conv_store_dst); a mixed plan whose
conv2_ / conv3_ groups run as `:x` (fp16 correction passes, "no e4m3 range limits": its launches are bounded as 3aw, with no saturation allowance,
at every gain); fp16 and F16X3 at 144x80 for the cases named for fp16 subnormals.

Asserted per case: every map finite; the reach conditions of the case on the engine's own blobs (built-in mixed plans; on the other plans that
saturation is reached at all); every tensor below 32768; for zero_launch the stored outputs equal relu(b) rounded.  Printed: the worst |err|/tol
per kernel instantiation (profiles/conv_range_check.txt has the table)."""
import time

import numpy as np
import pytest

import _convcheck as cc
import _customnets as cn
import _rangecases as rg
import _synth

pytestmark = pytest.mark.gpu

INTERIOR = 128
X_RULES = "conv2_:x,conv3_:x,conv4_,*_stage4_,*_stage5_,*_stage6_,@1x1"      # the default split set with the first two groups on fp16 correction passes
X_GROUPS = ("conv2_", "conv3_")
PLANS = {   # name -> (graph: built-in model or custom net, mode, W, H, split_layers)
    "coco": (0, "mixed", 144, 80, None),
    "mpi": (1, "mixed", 96, 64, None),
    "odd": ("odd", "mixed", 256, 64, "@all"),
    "coco_x": (0, "mixed", 144, 80, X_RULES),
    "coco_fp16": (0, "fp16", 144, 80, None),
    "coco_f16x3": (0, "f16x3", 144, 80, None),
}
MATRIX = ([("coco", c) for c in rg.CASES] +
          [("mpi", c) for c in ("gain_256_ss", "gain_2048", "gain_tiny", "pair_mismatch")] +
          [("odd", c) for c in ("gain_192", "gain_2048_ss", "channel_spread", "pair_mismatch")] +
          [("coco_x", c) for c in ("gain_192", "gain_256_ss", "gain_2048")] +
          [(p, c) for p in ("coco_fp16", "coco_f16x3") for c in ("subnormal_weights", "gain_tiny")])
_graphs = {}


def plan_graph(plan):
    g = PLANS[plan][0]
    if g not in _graphs:
        _graphs[g] = cn.net(g)[1] if isinstance(g, str) else cc.builtin_graph(g)
    return _graphs[g]


def plan_config(plan):
    import caffe_rtpose_amd as r
    g, mode, W, H, split = PLANS[plan]
    if isinstance(g, str):
        return cn.config(g, mode, W, H)
    prec = {"fp16": r.PREC_FP16, "mixed": r.PREC_MIXED, "f16x3": r.PREC_F16X3}[mode]
    kw = dict(split_layers=split) if split else {}
    return r.Config(model=g, net_w=W, net_h=H, num_scales=1, scale_gap=0.3, precision=prec, frames_in_flight=1, batch_frames=1, synthetic_seed=1, **kw)


def saturating_for(plan):
    """which launches get the saturation terms: every 2q launch — the `:x` groups run no 2q launch and get none"""
    if plan != "coco_x":
        return True
    return lambda L: not any(n.startswith(X_GROUPS) for n in L.layers)


def expected_relu_b(b, part):
    """what rtp_get_blob returns of a tensor that holds relu(b) in every pixel: the fp16 value plus the lo block, else the q block, that the tensor carries"""
    v = np.maximum(np.asarray(b, np.float32), np.float32(0))
    hi = cc._round16(v)
    if "lo" in part:
        return hi + cc._round16(v - hi)
    if "q" in part:
        return hi + cc._e4m3((v - hi) * np.float32(4096)) * np.float32(1.0 / 4096)
    return hi


def check_case(plan, case, summary, graph, wts, blob, heat, images_per_launch=1):
    """everything that is asserted of one case, on the blobs `blob` returns (the engine's; tests/test_conv_ranges_cpu.py's emulation for a dry run)"""
    mode = PLANS[plan][1]
    _, launches = cc.parse_plan(summary)
    assert np.isfinite(heat).all(), f"{plan} {case}: {int((~np.isfinite(heat)).sum())} non-finite map values"
    seen = {}

    def blob(nm, inner=blob):      # every blob the check reads goes into the range assertion below
        if nm not in seen:
            seen[nm] = inner(nm)
        return seen[nm]

    if mode == "mixed":
        if plan in ("coco", "mpi"):
            rc = rg.check_reach(case, graph, launches, wts, blob)
        else:
            rc = rg.reach(graph, launches, wts, blob)
            if case.startswith("gain_"):
                assert max(d["share112"] for _, d in rc) > 0.05 and max(d["amax"] for _, d in rc) >= 224.0, [d for _, d in rc]
        print(f"\n[rangecheck] {plan} | {case} | 2q inputs: |a_hi| >= 112 in {min(d['share112'] for _, d in rc):.3f}..{max(d['share112'] for _, d in rc):.3f}, "
              f"largest |a| {min(d['amax'] for _, d in rc):.4g}..{max(d['amax'] for _, d in rc):.4g}, weight exponents {sorted({d['t'] for _, d in rc})}")
    if plan == "coco_x":
        assert all("q" not in L.passes and L.passes == "3aw" for L in launches if L.kind == "conv" and any(n.startswith(X_GROUPS) for n in L.layers))
        ins = [np.abs(blob(graph.convs[n]["bottom"])) for L in launches if L.kind == "conv" for n in L.layers if n.startswith(X_GROUPS)]
        assert max(float(a.max()) for a in ins) >= 224.0      # the :x launches do read values beyond both e4m3 ranges
    reps = cc.check_plan(summary, graph, wts, blob, n_interior=INTERIOR, seed=11, images_per_launch=images_per_launch, saturating=saturating_for(plan))
    nl = len([ln for ln in summary.splitlines() if ln.startswith("step ") and not ln.startswith("step pack")])
    assert len(reps) == nl and all(rep.nchecked > 0 for rep in reps)
    for key, worst in sorted(cc.summarize(reps).items(), key=lambda kv: cc.key_str(kv[0])):
        print(f"[rangecheck] {plan} | {case} | {cc.key_str(key)} | worst |err|/tol {worst:.4f}")
    mx = max(float(np.abs(v).max()) for n, v in seen.items() if n != graph.input)
    print(f"[rangecheck] {plan} | {case} | largest |value| of a blob {mx:.5g}")
    bad = [rep for rep in reps if rep.nfail]
    for rep in bad:
        print(f"[rangecheck] FAIL {plan} {case} {rep.launch!r}: {rep.nfail} of {rep.nchecked} elements, worst |err|/tol {rep.worst:.3g}")
        for (dest, cls), (n, nf, worst) in rep.by_class.items():
            print(f"    -> {dest} {cls}: {nf} of {n} elements, worst {worst:.3g}")
        for f in rep.failures[:8]:
            print(f"    {f}")
    assert not bad, f"{len(bad)} launches outside their bound, first: {bad[0].failures[0]}"
    assert np.isfinite(mx) and mx < rg.LIMIT, (plan, case, mx)
    if case == "zero_launch":
        parts = cc.tensor_parts(graph, launches)
        for n in rg.named_launch(case, launches).layers:
            got = blob(n)
            want = expected_relu_b(wts[n][1], parts.get(n, ""))
            assert np.array_equal(got, np.broadcast_to(want[None, :, None, None], got.shape)), n
    return reps


@pytest.mark.parametrize("plan,case", MATRIX, ids=[f"{p}-{c}" for p, c in MATRIX])
def test_every_launch_at_the_range_edges_against_float64(plan, case):
    import caffe_rtpose_amd as r
    graph, cfg = plan_graph(plan), plan_config(plan)
    W, H = cfg.c.net_w, cfg.c.net_h
    t0 = time.time()
    e = r.Engine(cfg)
    try:
        layers = e.conv_layers()
        assert [n for n, *_ in layers] == list(graph.convs)
        summary = r.plan_summary(e.cfg)
        base = {n: e.get_conv_weights(i) for i, (n, *_rest) in enumerate(layers)}
        wts = rg.apply_case(case, graph, cc.parse_plan(summary)[1], base)
        for i, (n, *_rest) in enumerate(layers):
            e.set_conv_weights(i, *wts[n])
        for i, (n, *_rest) in enumerate(layers):      # what the launches are checked against is what the engine holds
            w, b = e.get_conv_weights(i)
            assert np.array_equal(w, wts[n][0]) and np.array_equal(b, wts[n][1]), n
        assert r.plan_summary(e.cfg) == summary
        x = _synth.random_frame(1, H, W, seed=3)
        t1 = time.time()
        heat = e.forward_heatmaps(x)
        t2 = time.time()
        assert np.array_equal(heat, e.get_blob(graph.lowres), equal_nan=True)
        cache = {}

        def blob(nm):
            if nm not in cache:
                cache[nm] = x if nm == graph.input else heat if nm == graph.lowres else e.get_blob(nm)
            return cache[nm]

        check_case(plan, case, summary, graph, wts, blob, heat)
        print(f"[rangecheck] {plan} | {case} | engine build + weights {t1 - t0:.2f} s, forward {t2 - t1:.2f} s, taps + float64 reference {time.time() - t2:.2f} s")
    finally:
        e.close()

"""The range cases of tests/_rangecases.py on the CPU: what they reach, that the bound of tests/_convcheck.py (saturating=True) is sound on them, and
that it catches what it is for.

A correct kernel is emulated (_convcheck.Emulation) on the full-depth mixed plan of coco 64x48, on stage 1 of mpi 96x64 and — for the cases named
for fp16 subnormals — on the trunk of the fp16 and F16X3 plans of coco 64x48 (labels 1, 2w, 3aw: the tight fp16 bound).

1. Reach conditions, per 2q launch (conditions, not measurements; _rangecases.check_reach): the share of input elements with |a_hi| >= 112 is in
   [0.5 %, 60 %] at gains 192 and 256 and >= 40 % at 2048; some input element is >= 224 at 256 and 2048; gain_tiny has fp16-subnormal inputs in every 2q
   launch; channel_spread has an output channel whose fp8 weights are all e4m3 subnormals or 0; the weight exponent is 40 in wq_clamp and 0 in
   zero_launch; every tensor stays below 32768.
2. Soundness: the correct emulation passes check_plan(saturating=True) on every case.  The saturation terms are exactly 0 on the synthetic weights
   (every older case keeps its bound bit for bit), and the same-sign case at gain 256 FAILS without them: they are necessary.
3. Planted defects, each in the case named for it: no clamp in front of the e4m3 conversion (gain_256), a per-branch weight exponent on the packing
   side (pair_mismatch), the W_lo8 scale off by 11 (channel_spread), fp16 operands flushed to zero when subnormal (subnormal_weights under fp16 and
   F16X3, gain_tiny under mixed), the stand-alone q pooling choosing by the hi value alone (gain_tiny), a clamp at 240 instead of 448 (band_100_112)."""
import numpy as np
import pytest

import _convcheck as cc
import _rangecases as rg
import _synth

NETS = {   # name -> (model, mode, W, H, the emulation stops after)
    "coco": (0, "mixed", 64, 48, None),
    "mpi": (1, "mixed", 96, 64, "conv5_5_CPM_L2"),
    "coco_fp16": (0, "fp16", 64, 48, "conv4_4_CPM"),
    "coco_f16x3": (0, "f16x3", 64, 48, "conv4_4_CPM"),
}
MPI_CASES = [c for c in rg.CASES if c not in ("pair_mismatch", "zero_branch", "zero_launch")]     # stage 1 of the mpi plan has no paired 2q launch
MATRIX = [("coco", c) for c in rg.CASES] + [("mpi", c) for c in MPI_CASES] + [(n, c) for n in ("coco_fp16", "coco_f16x3") for c in ("subnormal_weights", "gain_tiny")]


class _Net:
    def __init__(self, name):
        import caffe_rtpose_amd as r
        model, mode, self.W, self.H, self.stop = NETS[name]
        self.graph = cc.builtin_graph(model)
        prec = {"fp16": r.PREC_FP16, "mixed": r.PREC_MIXED, "f16x3": r.PREC_F16X3}[mode]
        self.summary = r.plan_summary(r.Config(model=model, net_w=self.W, net_h=self.H, precision=prec))
        names = list(self.graph.convs)
        if self.stop:
            names = names[:names.index(self.stop) + 1]
        self.base = {n: r.synth_weights(1, n, self.graph.convs[n]["cout"], self.graph.channels[self.graph.convs[n]["bottom"]], self.graph.convs[n]["k"]) for n in names}
        _, launches = cc.parse_plan(self.summary)
        if self.stop:
            launches = launches[:next(i for i, L in enumerate(launches) if self.stop in L.layers + L.layers2) + 1]
        self.launches = launches
        self.frame = _synth.random_frame(1, self.H, self.W, seed=3)
        self.runs = {}

    def run(self, case, emulation=cc.Emulation, stop=None):
        """(weights, emulation) of a case; the correct emulation of a case is kept"""
        key = (case, emulation, stop)
        if key not in self.runs:
            wts = self.base if case == "base" else rg.apply_case(case, self.graph, self.launches, self.base)
            em = emulation(self.summary, self.graph, wts, self.frame, stop_after=stop or self.stop)
            if emulation is not cc.Emulation:
                return wts, em
            self.runs[key] = (wts, em)
        return self.runs[key]

    def check(self, wts, em, saturating=True, only=None):
        """the launches of the emulated part of the plan (`only`: those of these layers / pooled blobs)"""
        have = [n for L in self.launches for n in L.layers + L.layers2 if n in em.pre] + [L.pool_out for L in self.launches if L.kind == "pool" and L.pool_out in em.hi]
        names = [n for n in have if only is None or n in only]
        return cc.check_plan(self.summary, self.graph, wts, em.blob, n_interior=10 ** 9, only=names, saturating=saturating)


class _Lazy(dict):
    def __missing__(self, name):
        self[name] = _Net(name)
        return self[name]


@pytest.fixture(scope="module")
def nets():
    return _Lazy()


def _worst(reps, q):
    return max((rep.worst for rep in reps if ("q" in rep.launch.passes) == q), default=0.0)


@pytest.mark.parametrize("net,case", MATRIX, ids=[f"{n}-{c}" for n, c in MATRIX])
def test_case_reaches_its_range_and_the_correct_emulation_stays_inside_the_bound(nets, net, case):
    t = nets[net]
    wts, em = t.run(case)
    mx = max(float(np.abs(v).max()) for v in list(em.hi.values()) + list(em.pre.values()))
    assert np.isfinite(mx) and mx < rg.LIMIT, mx
    if NETS[net][1] == "mixed":
        rc = rg.check_reach(case, t.graph, t.launches, wts, em.blob)
        print(f"\n[{net} {case}] max |v| {mx:.4g}; per 2q launch: |a_hi| >= 112 in {min(d['share112'] for _, d in rc):.3f}..{max(d['share112'] for _, d in rc):.3f} of the input, "
              f"largest |a| {min(d['amax'] for _, d in rc):.4g}..{max(d['amax'] for _, d in rc):.4g}, weight exponents {sorted({d['t'] for _, d in rc})}, "
              f"{sum(d['small_channels'] for _, d in rc)} output channels with fp8 weights all subnormal or 0")
    else:
        assert {L.passes for L in t.launches if L.kind == "conv"} <= {"1", "2w", "3aw"}
        w_sub = wts[rg.SUBNORMAL_LAYER][0]
        if case == "subnormal_weights":
            assert (np.abs(w_sub) < 2.0 ** -14).mean() > 0.5 and float(np.abs(em.hi[rg.SUBNORMAL_LAYER]).max()) > 0.25      # most weights subnormal, the output normal
        else:
            a = np.abs(em.hi["pool1_stage1"])
            assert ((a > 0) & (a < 2.0 ** -14)).any()
    reps = t.check(wts, em)
    assert reps and all(rep.nchecked > 0 for rep in reps)
    print(f"[rangecheck-cpu] {net} | {case} | worst |err|/tol: 2q launches {_worst(reps, True):.4f}, other launches {_worst(reps, False):.4f}")
    bad = [str(f) for rep in reps for f in rep.failures]
    assert not bad, bad[:5]
    if case in ("zero_branch", "zero_launch"):      # relu(b) exactly: the accumulators hold nothing but the bias
        L = rg.named_launch(case, t.launches)
        for n in L.layers[:1 if case == "zero_branch" else 2]:
            b = np.maximum(wts[n][1], 0)
            assert np.array_equal(em.pre[n], np.broadcast_to(wts[n][1][None, :, None, None], em.pre[n].shape))
            assert np.array_equal(em.hi[n], np.broadcast_to(cc._round16(b)[None, :, None, None], em.hi[n].shape))


def test_saturation_terms_are_zero_inside_the_ranges_and_needed_beyond(nets):
    """On the synthetic weights the two saturation terms and the W_lo8 term of _convcheck._Saturation are exactly 0, and the fourth is non-zero only at
    weights below 2^-14, of which a He set holds a few (it moves the worst ratio of their launches by 2 parts in 10^6; with it switched off the ratios
    are the same bit for bit).  The default, saturating=False, is the unchanged code path.  On same-sign residuals at gain 256 the correct emulation leaves the OLD bound (assert taken out = saturating
    with the terms zeroed) in most 2q launches and stays inside the new one."""
    t = nets["coco"]
    wts, em = t.run("base")
    plain, sat = t.check(wts, em, saturating=False), t.check(wts, em, saturating=True)
    print("\nlargest relative change of a launch's worst ratio: %.3g" % max(abs(p.worst - s.worst) / p.worst for p, s in zip(plain, sat) if p.worst))
    assert all(abs(p.worst - s.worst) <= 1e-5 * p.worst for p, s in zip(plain, sat))      # the few synthetic weights below 2^-14
    cc._Saturation.SUBNORMAL_W = False
    try:
        rest = t.check(wts, em, saturating=True)
    finally:
        cc._Saturation.SUBNORMAL_W = True
    assert [rep.worst for rep in plain] == [rep.worst for rep in rest] and [rep.by_class for rep in plain] == [rep.by_class for rep in rest]      # bit for bit
    for L in rg.q_launches(t.launches):
        for n in L.layers:
            g = t.graph.convs[n]
            a64, w64 = cc._operands(L.passes, False, em.blob(g["bottom"]), wts[n][0])
            s = cc._Saturation(a64, w64, [wts[m][0] for m in L.layers], "lo+q", g["k"] // 2)
            assert not s.sat_a.any() and not s.sat_w.any() and not s.sat_l.any(), n
            assert not s.sub_w[s.wabs >= 2.0 ** -14].any(), n      # only weights below the fp16 normal range have a term
    wts, em = t.run("gain_256_ss")
    new = t.check(wts, em)
    keep = cc._Saturation.tol
    cc._Saturation.tol = lambda self, n, ys, xs: 0.0
    try:
        old = t.check(wts, em)
    finally:
        cc._Saturation.tol = keep
    nq = len([rep for rep in old if "q" in rep.launch.passes])
    failing = len([rep for rep in old if "q" in rep.launch.passes and rep.nfail])
    print(f"\nsame-sign residuals, gain 256: worst 2q |err|/tol {_worst(old, True):.3f} without the saturation terms ({failing} of {nq} 2q launches fail), {_worst(new, True):.3f} with them")
    assert failing >= nq // 4 and _worst(old, True) > 1.2
    assert not any(rep.nfail for rep in new) and _worst(new, True) > 0.25      # ... and the new terms are not loose


# ------------------------------------------------------------------------------------------------------------
# planted defects
# ------------------------------------------------------------------------------------------------------------
def _e4m3_clamped(x32, lim):
    import torch
    x = np.ascontiguousarray(x32, np.float32)
    if lim is not None:
        x = np.clip(x, -lim, lim)
    return torch.from_numpy(x).to(torch.float8_e4m3fn).float().numpy()      # NaN beyond 464, like v_cvt_pk_fp8_f32


class NoClamp(cc.Emulation):
    def e4m3(self, x32):
        return _e4m3_clamped(x32, None)


class Clamp240(cc.Emulation):
    """the FNUZ e4m3 maximum instead of the OCP one"""
    def e4m3(self, x32):
        return _e4m3_clamped(x32, 240.0)


class PerBranchExponent(cc.Emulation):
    """the host packs each branch's fp8 weights with that branch's own exponent, the kernel descales both with the launch's"""
    def wq_pack(self, name):
        return cc._wq_t([self.weights[name][0]])


class WloScaleFromWhi(cc.Emulation):
    """E8M0 sb_odd taken from sb_even: W_lo8 descaled by 2^-t instead of 2^-(t + 11)"""
    WLO_EXP = 0


class FlushSubnormals(cc.Emulation):
    """an MFMA that reads fp16 subnormals as 0"""
    def mfma_in(self, x16):
        return np.where(np.abs(x16) < np.float32(2.0 ** -14), np.float32(0), x16)


class PoolByHi(cc.Emulation):
    """the stand-alone q pooling orders by hi alone: among equal hi values the first wins, with ITS q byte"""
    def pool_value(self, hi, part):
        return hi


def _fails(t, case, emulation, stop=None, only=None):
    wts, em = t.run(case, emulation, stop=stop)
    reps = t.check(wts, em, only=only)
    bad = [rep for rep in reps if rep.nfail]
    print(f"\n{emulation.__name__} on {case}: {len(bad)} of {len(reps)} launches fail, worst |err|/tol {max(rep.worst for rep in reps):.3g}")
    return bad, reps


def test_planted_missing_clamp_in_front_of_the_e4m3_conversion(nets):
    t = nets["mpi"]
    bad, reps = _fails(t, "gain_256", NoClamp)
    assert {rep.launch.passes for rep in bad} >= {"2q"} and any(not np.isfinite(f.got) for rep in bad for f in rep.failures)


def test_planted_per_branch_weight_exponent(nets):
    t = nets["coco"]
    bad, reps = _fails(t, "pair_mismatch", PerBranchExponent, stop="Mconv2_stage4_L2")
    assert bad and all(len(rep.launch.layers) == 2 and "q" in rep.launch.passes for rep in bad)


def test_planted_w_lo8_scale_off_by_11(nets):
    t = nets["mpi"]
    bad, reps = _fails(t, "channel_spread", WloScaleFromWhi, stop="conv4_4_CPM")
    assert len(bad) == len([rep for rep in reps if "q" in rep.launch.passes]) and all("q" in rep.launch.passes for rep in bad)


@pytest.mark.parametrize("net,case", [("coco_fp16", "subnormal_weights"), ("coco_f16x3", "subnormal_weights"), ("mpi", "gain_tiny")])
def test_planted_flush_of_subnormal_fp16_operands(nets, net, case):
    t = nets[net]
    bad, reps = _fails(t, case, FlushSubnormals, stop="conv3_1")
    assert bad
    if case == "subnormal_weights":
        assert rg.SUBNORMAL_LAYER in {f.layer for rep in bad for f in rep.failures}


def test_planted_q_pooling_by_the_hi_value_alone(nets):
    t = nets["mpi"]
    pools = [L for L in t.launches if L.kind == "pool" and "q" in cc.tensor_parts(t.graph, t.launches).get(L.pool_in, "")]
    assert pools
    bad, reps = _fails(t, "gain_2048", PoolByHi, stop="conv3_1", only=[L.pool_out for L in pools])
    assert bad and all(rep.launch.kind == "pool" for rep in bad)


def test_planted_clamp_at_240_instead_of_448(nets):
    """Not caught by the gain cases: with He-distributed activations the part of a_hi * W_lo that a clamp at 240 drops (Qa ends at 60 instead of 112)
    stays below the 2^-13.4 |a||W| that the bound grants the fp8 roundings — worst 2q ratios 0.59 / 0.87 at gains 64 / 256 in the trial behind this
    test.  band_100_112 makes the dropped parts as large and as coherent as the correct range allows: every input element in (100, 112), every W_lo
    positive and 2^-11 (2^-11 / 1.5) of |W|."""
    t = nets["coco"]
    wts, em = t.run("band_100_112", stop=rg.BAND_LAYER)
    a = em.blob(t.graph.convs[rg.BAND_LAYER]["bottom"])
    assert 100.0 < float(a.min()) and float(a.max()) < 112.0
    good = t.check(wts, em, only=[rg.BAND_LAYER])
    assert len(good) == 1 and good[0].nfail == 0
    bad, reps = _fails(t, "band_100_112", Clamp240, stop=rg.BAND_LAYER, only=[rg.BAND_LAYER])
    print(f"band_100_112: correct emulation worst |err|/tol {good[0].worst:.3f}, clamp at 240 {reps[0].worst:.3f}")
    assert bad and bad[0].launch.layers == [rg.BAND_LAYER]
    for case in ("gain_192", "gain_256"):      # what the gain cases see of it (printed, for the record)
        wts, em = nets["mpi"].run(case, Clamp240, stop="conv4_4_CPM")
        print(f"clamp at 240 on {case}: worst 2q |err|/tol {_worst(nets['mpi'].check(wts, em), True):.3f}")

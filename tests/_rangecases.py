"""Weight sets that drive single convolution launches to the edges of the fp8 and fp16 value ranges — TEST INFRASTRUCTURE (numpy only).

Every case is a transformation of a weight set {layer: (w, b)} (the engine's synthetic He weights: caffe_rtpose_amd.synth_weights on the CPU,
rtp_get_conv_weights on the GPU, written back with rtp_set_conv_weights) for a graph (_convcheck.Graph) and the launches of one plan
(_convcheck.parse_plan).  ReLU, max pooling and concat are positively homogeneous: scale a producer's weights and every bias behind it by g > 0 and
every blob behind it scales by g; scale the output channels of a layer and divide its consumers' input channels by the same numbers and nothing
behind the consumers changes.  All scales are powers of two, so the transformed network is the same function in exact arithmetic.

  gain_192 / gain_256 / gain_2048     the first layer's weights and every bias times g: activations up to 4g.  fp8(a_hi * 4) saturates at |a| = 112, fp8(lo * 2^12)
                                      from |a| = 256 on (tests/_convcheck.py, `Beyond the e4m3 ranges`).  The smallest gain is 192, not 64: the synthetic
                                      network's activations shrink towards the late stages (largest input of a 2q launch 0.96 to 3.8), and only gains of 176 to 503
                                      put 0.5 % to 60 % of EVERY 2q launch's input at or beyond 112; 2048 is the smallest power of two with 40 % everywhere
  ..._ss                              the same on same-sign-residual weights: every weight f16(w) + 3/8 of its fp16 step, so that W_lo = W - f16(W) > 0 everywhere and
                                      the parts of the a_hi * W_lo correction that saturation drops add up over the K terms instead of cancelling
  gain_tiny                           gain 2^-14: activations in and below the fp16 subnormal range, the lo and q blocks at their small end
  subnormal_weights                   one layer's weights times 2^-13 (most |W| < 2^-14: W_hi subnormal, W_lo subnormal or 0), its input gained up by 2^12 so that its
                                      output stays in the normal range (half the synthetic network's from there on)
  channel_spread                      per-output-channel scales 2^e, e integer in [-10, 4], on every layer of a 2q launch, undone on the consumers' input channels.
                                      The channel with the smallest largest weight takes -10 and the one with the largest +4, the rest are drawn: the weight
                                      exponent of the launch drops, and small channels' fp8 weights are e4m3 subnormals or 0
  pair_mismatch                       in every paired 2q launch the first branch times 2^8, the second times 2^-8, undone in the consumers: the branches share ONE
                                      fp8 weight exponent, a per-branch one on either side is off by 2^16
  zero_branch / zero_launch           the first branch / both branches of the first paired 2q launch all-zero with positive biases (both: max|W| = 0, exponent 0):
                                      the output is relu(b) exactly
  wq_clamp                            the first 2q launch with every weight below 448 * 2^-41: the exponent clamps at 40
  band_100_112                        (CPU only, run up to BAND_LAYER; made for a planted e4m3 clamp at 240 instead of 448, which turns Qa's end from 112 into 60)
                                      the producer of one 2q layer gets the bias 106 and weights small enough that its output stays in (100, 112): every input
                                      element of the 2q layer is as far beyond 60 as the correct range allows.  That layer's weights become 2^k (w >= 0) or
                                      -1.5 * 2^(k-1) (w < 0) plus 31/64 of the fp16 step there: the largest same-sign W_lo there is

Scope: every tensor stays below half the fp16 range, max |v| < 32768 (asserted where the cases are used).  What the engine does with values beyond the
fp16 maximum 65504 — they are stored as infinity — is not covered by these cases or by the bound they are checked with."""
from collections import OrderedDict

import numpy as np

import _convcheck as cc

LIMIT = 32768.0
GAIN_CASES = OrderedDict([("gain_192", (192.0, False)), ("gain_256", (256.0, False)), ("gain_2048", (2048.0, False)),
                          ("gain_192_ss", (192.0, True)), ("gain_256_ss", (256.0, True)), ("gain_2048_ss", (2048.0, True))])
CASES = list(GAIN_CASES) + ["gain_tiny", "subnormal_weights", "channel_spread", "pair_mismatch", "zero_branch", "zero_launch", "wq_clamp"]
SUBNORMAL_LAYER = "conv2_1"     # of the built-in graphs: reads pool1_stage1
SUB_IN, SUB_W = 2.0 ** 12, 2.0 ** -13
BAND_LAYER, BAND_BIAS, BAND_SPREAD = "conv2_2", 106.0, 1.0     # conv2_1's synthetic pre-activation stays within +-6: its output in (100, 112)


def f32(x):
    return np.ascontiguousarray(x, np.float32)


def fp16_step(h):
    """the spacing of fp16 at h (2^-24 below the normal range)"""
    a = np.abs(np.asarray(h, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def same_sign(w):
    """f16(w) + 3/8 of the fp16 step there: exact in float32, W_lo > 0"""
    h = cc.f16(w)
    step = np.where((h < 0) & (np.abs(h) == 2.0 ** np.floor(np.log2(np.maximum(np.abs(h), 2.0 ** -30)))), 0.5, 1.0) * fp16_step(h)   # (towards 0 from -2^k the spacing halves)
    out = f32(h + 0.375 * step)
    assert np.array_equal(cc.f16(out), h)
    return out


def largest_residual(w):
    """|w| -> 2^k (w >= 0) or 1.5 * 2^(k-1) (w < 0), k = round(log2|w|), plus 31/64 of the fp16 step: W_lo > 0 and 2^-11 (2^-11 / 1.5) of |W|"""
    a = np.maximum(np.abs(np.asarray(w, np.float64)), 2.0 ** -12)
    k = np.round(np.log2(a))
    h = np.where(np.asarray(w) >= 0, 2.0 ** k, -0.75 * 2.0 ** k)      # (smaller negative weights: the layer's outputs stay positive, ReLU hides none)
    out = f32(h + (31.0 / 64.0) * fp16_step(h))
    assert np.array_equal(cc.f16(out), h)
    return out


def first_conv(graph):
    return next(n for n, c in graph.convs.items() if c["bottom"] == graph.input)


def consumers(graph, blob, off=0):
    """[(convolution, first input channel)] that read `blob`'s channels, through pooling layers and concats"""
    out = [(n, off) for n, c in graph.convs.items() if c["bottom"] == blob]
    for top, bot in graph.pools.items():
        if bot == blob:
            out += consumers(graph, top, off)
    for top, bots in graph.concats.items():
        o = 0
        for b in bots:
            if b == blob and top != graph.lowres:
                out += consumers(graph, top, off + o)
            o += graph.channels[b]
    return out


def ancestors(graph, conv):
    """the convolutions `conv`'s input depends on"""
    out, todo = set(), [graph.convs[conv]["bottom"]]
    while todo:
        b = todo.pop()
        if b in graph.convs and b not in out:
            out.add(b)
            todo.append(graph.convs[b]["bottom"])
        elif b in graph.pools:
            todo.append(graph.pools[b])
        elif b in graph.concats:
            todo += graph.concats[b]
    return out


def q_launches(launches):
    return [L for L in launches if L.kind == "conv" and "q" in L.passes]


def _gain(graph, wts, g):
    first = first_conv(graph)
    return {n: (f32(w * np.float32(g)) if n == first else w, f32(b * np.float32(g))) for n, (w, b) in wts.items()}


def _scale_out(graph, wts, name, s):
    """output channels of `name` times s[c] (powers of two), its consumers' input channels divided by them"""
    s = np.asarray(s, np.float32)
    if s.ndim == 0:
        s = np.full(graph.convs[name]["cout"], s, np.float32)
    users = consumers(graph, name)
    assert users, f"{name} has no convolution behind it"
    w, b = wts[name]
    wts[name] = (f32(w * s[:, None, None, None]), f32(b * s))
    for u, off in users:
        if u not in wts:      # a weight set that ends before the consumer (an emulation of the first stages): nothing behind it is run
            continue
        wu, bu = wts[u]
        wu = wu.copy()
        wu[:, off:off + len(s)] /= s[None, :, None, None]
        wts[u] = (wu, bu)


def apply_case(case, graph, launches, weights, seed=0):
    """the weight set of `case`: {layer: (w float32, b float32)}; `weights` is not modified"""
    wts = {n: (f32(w).copy(), f32(b).copy()) for n, (w, b) in weights.items()}
    ql = q_launches(launches)
    if case in GAIN_CASES:
        g, ss = GAIN_CASES[case]
        if ss:
            wts = {n: (same_sign(w), b) for n, (w, b) in wts.items()}
        return _gain(graph, wts, g)
    if case == "gain_tiny":
        return _gain(graph, wts, 2.0 ** -14)
    if case == "band_100_112":
        tgt = BAND_LAYER
        prod = graph.convs[tgt]["bottom"]
        assert prod in graph.convs and any(tgt in L.layers for L in ql)
        w, b = wts[prod]
        wts[prod] = (f32(w * np.float32(BAND_SPREAD)), np.full_like(b, BAND_BIAS))
        wts[tgt] = (largest_residual(wts[tgt][0]), wts[tgt][1])
        return wts
    if case == "subnormal_weights":
        up = ancestors(graph, SUBNORMAL_LAYER)
        first = first_conv(graph)
        out = {}
        for n, (w, b) in wts.items():
            ws = SUB_IN if n == first else SUB_W if n == SUBNORMAL_LAYER else 1.0
            bs = SUB_IN if n in up else SUB_IN * SUB_W
            out[n] = (f32(w * np.float32(ws)), f32(b * np.float32(bs)))
        return out
    if case == "channel_spread":
        rs = np.random.RandomState(seed + 17)
        for L in ql:
            for n in L.layers:
                if not consumers(graph, n):
                    continue
                rowmax = np.abs(weights[n][0]).reshape(len(weights[n][0]), -1).max(axis=1)
                e = rs.randint(-10, 5, size=len(rowmax))
                e[int(rowmax.argmin())], e[int(rowmax.argmax())] = -10, 4
                _scale_out(graph, wts, n, 2.0 ** e.astype(np.float64))
        return wts
    if case == "pair_mismatch":
        pairs = [L for L in ql if len(L.layers) == 2]
        assert pairs
        for L in pairs:
            _scale_out(graph, wts, L.layers[0], 2.0 ** 8)
            _scale_out(graph, wts, L.layers[1], 2.0 ** -8)
        return wts
    if case in ("zero_branch", "zero_launch"):
        L = next(L for L in ql if len(L.layers) == 2)
        for n in L.layers[:1 if case == "zero_branch" else 2]:
            w, b = wts[n]
            wts[n] = (np.zeros_like(w), f32(np.abs(b) + np.float32(0.25)))
        return wts
    if case == "wq_clamp":
        L = ql[0]
        mx = max(float(np.abs(wts[n][0]).max()) for n in L.layers)
        s = 2.0 ** -(int(np.ceil(np.log2(mx / (448.0 * 2.0 ** -41)))) + 1)
        for n in L.layers:
            wts[n] = (f32(wts[n][0] * np.float32(s)), wts[n][1])
        assert max(float(np.abs(wts[n][0]).max()) for n in L.layers) < 448.0 * 2.0 ** -41
        return wts
    raise KeyError(case)


def named_launch(case, launches):
    """the launch a zero_* / wq_clamp case changes"""
    ql = q_launches(launches)
    return next(L for L in ql if len(L.layers) == 2) if case.startswith("zero_") else ql[0]


def e4m3_small(w, t):
    """where a weight's fp8 copy e4m3(W_hi * 2^t) is an e4m3 subnormal or 0 (below the smallest normal 2^-6)"""
    return np.abs(cc.f16(w)) * 2.0 ** t < 2.0 ** -6


def reach(graph, launches, weights, blob):
    """what the inputs and weights of every 2q launch reach: [(launch, dict)] with the share of input elements whose |a_hi| >= 112, the largest |a|,
    whether an input element is a non-zero fp16 subnormal, the fp8 weight exponent and the output channels whose fp8 weights are all subnormal or 0"""
    out = []
    for L in q_launches(launches):
        ah = np.concatenate([np.abs(cc.f16(blob(graph.convs[n]["bottom"]))).reshape(-1) for n in L.layers])
        t = cc._wq_t([weights[n][0] for n in L.layers])
        small = [e4m3_small(weights[n][0], t).reshape(len(weights[n][0]), -1) for n in L.layers]
        out.append((L, dict(share112=float((ah >= 112.0).mean()), amax=float(ah.max()), subnormal_in=bool(((ah > 0) & (ah < 2.0 ** -14)).any()), t=t,
                            small_channels=int(sum(s.all(axis=1).sum() for s in small)), small_share=float(np.concatenate([s.reshape(-1) for s in small]).mean()))))
    return out


def check_reach(case, graph, launches, weights, blob):
    """the reach conditions of `case` (tests/test_conv_ranges_cpu.py states them), asserted on the blobs `blob` returns; returns the reach list"""
    rc = reach(graph, launches, weights, blob)
    assert rc
    base = case[:-3] if case.endswith("_ss") else case
    for L, d in rc:
        if base in ("gain_192", "gain_256"):
            assert 0.005 <= d["share112"] <= 0.60, (case, L, d)
        if base == "gain_2048":
            assert d["share112"] >= 0.40, (case, L, d)
        if base in ("gain_256", "gain_2048"):
            assert d["amax"] >= 224.0, (case, L, d)
        if case == "gain_tiny":
            assert d["subnormal_in"], (case, L, d)
    tl = {id(L): d for L, d in rc}
    if case == "channel_spread":
        assert sum(d["small_channels"] for _, d in rc) >= 1, [d for _, d in rc]
    if case == "wq_clamp":
        assert tl[id(named_launch(case, launches))]["t"] == 40
    if case == "zero_launch":
        assert tl[id(named_launch(case, launches))]["t"] == 0
    return rc

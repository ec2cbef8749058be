"""The per-launch convolution checker (tests/_convcheck.py) on the CPU: which kernel instantiations its GPU matrix reaches, and that it
catches what it is for.

1. Coverage.  rtp_plan_summary needs no device: the instantiation keys (step kind, single / paired, +pool, k, cin_p, tile, rowb, pass label,
   ring / reg, several destinations, low-res output) of every plan bench.py times — test_precision.CONFIGS in the default mixed mode — must be
   among the keys of _convcheck.MATRIX, the configurations tests/test_conv_launches.py runs on the GPU.  A new tile or pass variant in a
   benchmarked plan fails here until the matrix reaches it.
2. The checker on a correct kernel and on planted defects.  A correct kernel is emulated on the CPU (operands rounded to fp16, float32
   accumulation, outputs rounded to fp16 + lo part or + the e4m3 operands of the fp8-compensated launches; _convcheck.Emulation) for the
   first two stages of the 128x32 plans in F16X3, pure fp16 and mixed — the smallest resolution that still has a pooling epilogue, stand-alone pooling steps, the im2col and the direct input layer,
   64x64 / 128x64 / 128x32 tiles, six concat destinations and both branch-tail shapes.  Every pixel is sampled there.  It must pass;
   each planted defect must fail, in the right layer and the right pixel class."""
import numpy as np
import pytest

import _convcheck as cc
import _synth
import test_precision as tp

W, H = 128, 32
STOP = "Mconv7_stage2_L2"      # the emulation runs the trunk, stage 1 and stage 2


def _r():
    import caffe_rtpose_amd as r
    return r


@pytest.fixture(scope="module")
def graphs():
    return {m: cc.builtin_graph(m) for m in (0, 1)}


def test_graph_of_the_builtin_model_matches_the_engine_layer_list(graphs):
    import _oracle as orc
    for model, g in graphs.items():
        net = orc.Net(model)
        assert [(n, g.channels[c["bottom"]], c["cout"], c["k"]) for n, c in g.convs.items()] == net.convs
        assert g.lowres == "concat_stage7" and g.concats["concat_stage7"] == ["Mconv7_stage6_L2", "Mconv7_stage6_L1"]
        assert g.dests("conv4_4_CPM") == [("conv4_4_CPM", 0)] + [(f"concat_stage{s}", g.channels["conv5_5_CPM_L1"] + g.channels["conv5_5_CPM_L2"]) for s in range(2, 7)]
        assert [g.level[b] for b in ("image", "conv1_2", "pool1_stage1", "conv3_4", "pool3_stage1", "concat_stage7")] == [0, 0, 1, 2, 3, 3]


def test_matrix_reaches_every_instantiation_of_the_benchmarked_plans(graphs):
    r = _r()
    have = {}
    for name in cc.MATRIX:
        for k in cc.plan_keys(r.plan_summary(cc.matrix_config(name)), graphs[cc.MATRIX[name][1]]):
            have.setdefault(k, name)
    print(f"\n{len(have)} instantiations in {len(cc.MATRIX)} configurations")
    missing = []
    for cfg, (model, w, h, n, gap, b) in tp.CONFIGS.items():
        c = r.Config(model=model, net_w=w, net_h=h, num_scales=n, start_scale=tp.START.get(cfg, 1.0), scale_gap=gap, precision=r.PREC_MIXED,
                     frames_in_flight=b, batch_frames=b, synthetic_seed=tp.SEEDS.get(cfg, 1))
        missing += [(cfg, cc.key_str(k)) for k in cc.plan_keys(r.plan_summary(c), graphs[model]) if k not in have]
    assert not missing, missing
    # what the issue names as unchecked so far is in the matrix
    keys = [cc.key_str(k) for k in have]
    for needle in ("tile 128x128 rowb 128 passes 2q ring", "+pool", "pair k 7 cin_p 192", "tile 128x32 rowb 256 passes 2q ring dsts>1", "mid 512", "mid 128",
                   "passes 3aw ring", "passes 2w reg", "passes 3aw/3aw", "first k 3", "lowres"):
        assert any(needle in k for k in keys), needle


def test_tile_walks_match_the_workgroup_counts_of_the_plan(graphs):
    """plain_tile_ends / pool_tile_ends restate plan.h: tiles per image x images x N tiles x branches == `wgs` of every launch of every matrix plan,
    and every tile end is an interior pixel"""
    r = _r()
    for name, (mode, model, w, h, n, gap, b, seed) in cc.MATRIX.items():
        levels, launches = cc.parse_plan(r.plan_summary(cc.matrix_config(name)))
        g = graphs[model]
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
            assert ends and all(0 <= y < lim[0] and 0 <= x < lim[1] for y, x in ends)


class _Toy:
    def __init__(self, mode, graph):
        r = _r()
        self.graph = graph
        self.summary = r.plan_summary(r.Config(net_w=W, net_h=H, precision={"f16x3": r.PREC_F16X3, "fp16": r.PREC_FP16, "mixed": r.PREC_MIXED}[mode]))
        stop = list(graph.convs).index(STOP)
        self.weights = {n: r.synth_weights(1, n, c["cout"], graph.channels[c["bottom"]], c["k"]) for n, c in list(graph.convs.items())[:stop + 1]}
        self.em = cc.Emulation(self.summary, graph, self.weights, _synth.random_frame(1, H, W, seed=3), stop_after=STOP)
        self.launch = {n: L for L in self.em.launches for n in L.layers + L.layers2}

    def check(self, only=None):
        names = list(self.weights) + list(self.graph.pools) if only is None else only
        return cc.check_plan(self.summary, self.graph, self.weights, self.em.blob, n_interior=10 ** 9, only=names)

    def plant(self, name, v, **kw):
        """store the fp32 values v as layer `name`'s output, check its launch alone, put the correct output back"""
        L = self.launch[name]
        finish = (lambda x, **k: self.em.store(name, x)) if L.kind == "pw2" else (lambda x, **k: self.em.finish(L, name, x, **k))
        finish(v, **kw)
        rep = self.check([name])
        finish(self.em.pre[name])
        assert len(rep) == 1
        return rep[0]


class _Lazy(dict):
    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, mode):
        self[mode] = self.make(mode)
        return self[mode]


@pytest.fixture(scope="module")
def toy(graphs):
    return _Lazy(lambda mode: _Toy(mode, graphs[0]))


@pytest.mark.parametrize("mode", ["f16x3", "fp16", "mixed"])
def test_emulated_correct_kernel_passes_every_launch(toy, mode):
    t = toy[mode]
    reps = t.check()
    kinds = {cc.key_str(rep.launch.key) for rep in reps}
    assert len(reps) == 24 and any("+pool" in k for k in kinds) and any(k.startswith("pool") for k in kinds) and any("mid 512" in k for k in kinds)
    for rep in reps:
        print(f"  {rep.launch!r:90.90s} worst |err|/tol {rep.worst:.3f} over {rep.nchecked} elements, {rep.tiles} tiles")
    print(f"[{mode}] worst |err|/tol {max(rep.worst for rep in reps):.3f}")
    bad = [str(f) for rep in reps for f in rep.failures]
    assert not bad, bad[:5]
    assert all(rep.nchecked > 0 for rep in reps)
    # the same launches stay clean after a plant + restore cycle (the defects below do not leak into each other)
    rep = t.plant("conv2_1", t.em.pre["conv2_1"])
    assert rep.nfail == 0


def _classes(rep):
    return {f.cls for f in rep.failures}


def test_planted_last_column_tap_read_from_the_next_row(toy):
    """flat addressing without the zero gap: the right-most tap of the last column reads the first pixel of the next row"""
    t = toy["f16x3"]
    name = "conv2_1"
    a_hi, _ = t.em.operand(t.graph.convs[name]["bottom"])
    w = np.asarray(t.weights[name][0], np.float32)
    v = t.em.pre[name].copy()
    for rr in range(3):   # tap (rr, 2) of output (y, W-1) is zero padding; the defect reads input (y + rr - 1 + 1, 0)
        src = np.zeros_like(a_hi[:, :, :, 0])
        yy = np.arange(a_hi.shape[2]) + rr
        ok = yy < a_hi.shape[2]
        src[:, :, ok] = a_hi[:, :, yy[ok], 0]
        v[:, :, :, -1] += np.einsum("oc,nch->noh", w[:, :, rr, 2], src)
    rep = t.plant(name, v)
    assert rep.nfail > 0 and _classes(rep) == {"border"} and all(f.layer == name and f.x == v.shape[3] - 1 for f in rep.failures), [str(f) for f in rep.failures]


def test_planted_stale_last_pixel_of_one_tile(toy):
    t = toy["f16x3"]
    name = "conv2_1"
    L = t.launch[name]
    levels, _ = cc.parse_plan(t.summary)
    hh, ww, halo = levels[1]
    ends, _ = cc.plain_tile_ends(hh, ww, halo, L.tile[0])
    y, x = next((y, x) for y, x in ends[1::2] if cc.BORDER <= y < hh - cc.BORDER and cc.BORDER <= x < ww - cc.BORDER)
    v = t.em.pre[name].copy()
    v[:, :, y, x] = v[:, :, y, x - 1]          # what an earlier launch left there
    rep = t.plant(name, v)
    assert rep.nfail > 0 and _classes(rep) == {"tile end"} and all((f.layer, f.y, f.x) == (name, y, x) for f in rep.failures), [str(f) for f in rep.failures]


def test_planted_swap_of_two_concat_channels(toy):
    t = toy["f16x3"]
    g = t.graph
    off = dict(g.dests("conv4_4_CPM"))["concat_stage2"]
    real = t.em.operand

    def swapped(name):
        hi, lo = real(name)
        if name == "concat_stage2":
            hi, lo = hi.copy(), lo.copy()
            for part in (hi, lo):
                part[:, [off + 5, off + 6]] = part[:, [off + 6, off + 5]]
        return hi, lo
    t.em.operand = swapped
    try:
        rep = t.check(["conv4_4_CPM"])[0]
    finally:
        t.em.operand = real
    assert rep.nfail > 0 and {(f.layer, f.dest) for f in rep.failures} == {("conv4_4_CPM", "concat_stage2")} and {f.ch for f in rep.failures} <= {5, 6}, [str(f) for f in rep.failures]


def test_planted_missing_relu_at_one_pixel(toy):
    t = toy["fp16"]
    name = "conv2_2"
    L, v = t.launch[name], t.em.pre[name]
    y, x = 7, 17
    assert (v[0, :, y, x] < 0).any()
    t.em.finish(L, name, v)
    t.em.hi[name][0, :, y, x] = cc._round16(v[0, :, y, x])          # stored without the ReLU
    rep = t.check([name])[0]
    t.em.finish(L, name, v)
    assert rep.nfail > 0 and all((f.layer, f.y, f.x, f.cls) == (name, y, x, "interior") and f.got < 0 for f in rep.failures), [str(f) for f in rep.failures]
    assert t.check([name])[0].nfail == 0


def test_planted_missing_bias_of_one_output_channel(toy):
    t = toy["fp16"]
    name = "Mconv3_stage2_L1"
    v = t.em.pre[name].copy()
    v[:, 77] -= np.float32(t.weights[name][1][77])
    rep = t.plant(name, v)
    assert rep.nfail > 0 and {(f.layer, f.ch) for f in rep.failures} == {(name, 77)}, [str(f) for f in rep.failures]
    assert t.check([name])[0].nfail == 0


def test_planted_pool_over_three_of_four_pixels(toy):
    t = toy["f16x3"]
    rep = t.plant("conv1_2", t.em.pre["conv1_2"], pool3=True)       # the pooling epilogue
    assert rep.launch.pool and rep.nfail > 0 and all(f.dest == "pool1_stage1" for f in rep.failures), [str(f) for f in rep.failures]
    L = next(L for L in t.em.launches if L.kind == "pool")           # a stand-alone pooling step: must be equal
    keep = t.em.hi[L.pool_out].copy()
    a = t.em.hi[L.pool_in]
    t.em.hi[L.pool_out] = np.maximum(np.maximum(a[:, :, 0::2, 0::2], a[:, :, 0::2, 1::2]), a[:, :, 1::2, 0::2])
    rep = t.check([L.pool_out])[0]
    t.em.hi[L.pool_out] = keep
    assert rep.launch.kind == "pool" and rep.nfail > 0 and rep.failures[0].dest == L.pool_out
    assert t.check([L.pool_out])[0].nfail == 0


@pytest.mark.parametrize("name", ["conv2_1", "conv5_1_CPM_L1"])
@pytest.mark.parametrize("skip", ["a", "w"])
def test_planted_missing_correction_pass_of_a_3aw_layer(toy, name, skip):
    """a 3aw launch that leaves out a_lo x W_hi (a) or a_hi x W_lo (w): a 2^-12-relative error per term, far below the fp16 rounding that hides it in
    every check on hi-only values — the bound that tells it apart is the 2^-22 of a tensor with a lo part.

    Where this stops: the omitted products add up like sqrt(K), the worst-case accumulation term c_acc * 2^-24 * S of the bound grows like K.  Measured
    here: 3x3 layers on 64 / 128 channels (K = 576 / 1152) 17x / 7x the bound; a 7x7 layer on 128 channels (K = 6272, Mconv2_stage2_L2) reaches 0.93-0.95
    of it and is NOT caught launch by launch — for those layers a missing pass is what the 1e-4 end-to-end bound of tests/test_precision.py (f16x3) sees."""
    t = toy["f16x3"]
    L = t.launch[name]
    assert L.passes == "3aw"
    a_hi, a_lo = t.em.operand(t.graph.convs[name]["bottom"])
    rep = t.plant(name, t.em.gemm(name, "3aw", a_hi, a_lo, skip=(skip,)))
    print(f"\n{name} without the {skip} correction: worst |err|/tol {rep.worst:.2f}, {rep.nfail} of {rep.nchecked} elements")
    assert rep.nfail > 0 and all(f.layer == name for f in rep.failures)

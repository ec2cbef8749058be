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
   each planted defect must fail, in the right layer and the right pixel class.
3. Graphs other than the built-in one (tests/_customnets.py, CUSTOM_MATRIX): the shape-dependent branches of the planner and of the epilogues
   that the built-in plans never take are reached (asserted feature by feature), the tile walks match the plans, a correct kernel emulated
   over every custom graph passes (which proves, among others, that no activation reaches the 112 at which the 2q bound ends), and the
   defects planted on the new paths fail in the right layer.
4. Plans of 7 to 13 images per launch (tests/_manycases.py CONV_MATRIX): the seven kernel classes that only such plans run are reached, each by
   the case named for it and by no plan of the three older matrices; the image counts 7, 10, 13, 16 and 32 occur; grids that are and are not
   a multiple of 8 per kernel; the tile walks match the plans."""
import numpy as np
import pytest

import _convcheck as cc
import _customnets as cn
import _manycases as mc
import _synth
import test_precision as tp

CUSTOM_MATRIX = cn.CUSTOM_MATRIX

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
    """plain_tile_ends / pool_tile_ends restate plan.h: tiles per image x images x N tiles x branches == `wgs` of every launch of every matrix plan (the batch matrix of tests/test_batch_launches.py included),
    and every tile end is an interior pixel"""
    r = _r()
    plans = [(name, graphs[model], n, b, r.plan_summary(cc.matrix_config(name))) for name, (mode, model, w, h, n, gap, b, seed) in cc.MATRIX.items()]
    plans += [(cn.case_id(c), cn.net(c[0])[1], c[4], c[5], r.plan_summary(cn.config(*c))) for c in CUSTOM_MATRIX]
    plans += [(name, graphs[model], n, b, r.plan_summary(cc.batch_config(name))) for name, (mode, model, w, h, n, gap, b, seed) in cc.BATCH_MATRIX.items()]   # tests/test_batch_launches.py: full batches
    plans += [(name, graphs[model], n, b, r.plan_summary(cc.matrix_config(name, mc.CONV_MATRIX))) for name, (mode, model, w, h, n, gap, b, seed) in mc.CONV_MATRIX.items()]   # tests/_manycases.py: 7 to 32 images
    plans += [(name, graphs[model], n, b, r.plan_summary(cc.batch_config(name, matrix=mc.BATCH_MATRIX))) for name, (mode, model, w, h, n, gap, b, seed) in mc.BATCH_MATRIX.items()]
    halos = set()
    for name, g, n, b, summary in plans:
        levels, launches = cc.parse_plan(summary)
        halos |= {(lvl, lv[2]) for lvl, lv in enumerate(levels)}
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
    assert {(0, 3), (1, 3), (2, 3)} <= halos       # levels whose halo is 3 below 1/8 resolution: custom plans only


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


# ------------------------------------------------------------------------------------------------------------
# graphs other than the built-in one
# ------------------------------------------------------------------------------------------------------------
def test_bound_of_the_builtin_launches_is_on_the_unchanged_code_path(graphs):
    """What the custom graphs added to the bound (a tensor with a lo AND a q block; a 3x3 ring layer on 32 fp32 channels, which the rule for the packed input
    layer used to match) is selected by conditions no built-in plan meets: their tolerance is computed by the same expressions as before."""
    r = _r()
    for name in cc.MATRIX:
        g = graphs[cc.MATRIX[name][1]]
        _, launches = cc.parse_plan(r.plan_summary(cc.matrix_config(name)))
        assert set(cc.tensor_parts(g, launches).values()) <= {"lo", "q"}, name
        assert not [L for L in launches if L.kind == "conv" and L.cin_p == 32 and L.k == 3 and L.impl != "reg"], name
        parts = cc.tensor_parts(g, launches)      # ... and no pair of theirs reads tensors with different blocks: the planner's un-pairing rule leaves them alone
        assert all(len({parts.get(g.convs[n]["bottom"], "") for n in L.layers}) == 1 for L in launches if len(L.layers) == 2), name
    a = np.linspace(-300.0, 300.0, 13)
    for part in ("", "lo", "q", "f32"):
        assert np.array_equal(cc.out_rounding(part, False, a), cc.out_rounding(part, False, a.copy()))
    assert np.array_equal(cc.out_rounding("lo+q", False, a), cc.out_rounding("lo", False, a))
    assert cc.e_op_of("2q", False) == cc.e_op_of("2q", False, "q") == (3 * 2.0 ** -15 + 2.0 ** -19 + 2.0 ** -22) * (1 + 2.0 ** -10)
    assert cc.e_op_of("2q", False, "lo+q") > cc.e_op_of("2q", False) and cc.e_op_of("3aw", False, "lo+q") == cc.e_op_of("3aw", False)


def test_accumulation_counts_of_1x1_layers_on_the_register_staged_kernel():
    """conv_igemm.hip launch_cfg<T, 1, 128>: one tap, cin_p * elem / 128 chunks, (128 / 32) / KSPLIT instructions per chunk and wave with KSPLIT 1 / 2 / 4 on
    128x128 / 64x128 / 64x64, + 15 roundings inside the fp16 instructions (+ 2 for fp32, four 32x32x2 per k-group), + KSPLIT - 1 for the reduction, + 1 bias"""
    mk = lambda tile, cin_p, passes: cc.Launch(kind="conv", layers=["x"], k=1, cin_p=cin_p, tile=tile, rowb=128, passes=passes, impl="reg")
    assert [cc.c_acc_conv(mk(t, 192, "3aw"), False) for t in ((128, 128), (64, 128), (64, 64))] == [3 * 3 * 4 + 15 + 0 + 1, 3 * 3 * 2 + 15 + 1 + 1, 3 * 3 * 1 + 15 + 3 + 1]
    assert [cc.c_acc_conv(mk(t, 128, "1"), False) for t in ((128, 128), (64, 128), (64, 64))] == [2 * 4 + 16, 2 * 2 + 17, 2 * 1 + 19]
    assert [cc.c_acc_conv(mk(t, 96, "1"), True) for t in ((128, 128), (64, 128), (64, 64))] == [3 * 4 * 4 + 2 + 0 + 1, 3 * 2 * 4 + 2 + 1 + 1, 3 * 1 * 4 + 2 + 3 + 1]
    # a 3x3 layer on a 32-channel fp32 tensor is a ring launch of nine taps, not the packed input layer (a 1x1 layer on 32 channels of the register-staged kernel)
    ring = cc.Launch(kind="conv", layers=["x"], k=3, cin_p=32, tile=(128, 64), rowb=128, passes="1", impl="ring")
    pack = cc.Launch(kind="conv", layers=["x"], k=3, cin_p=32, tile=(128, 64), rowb=128, passes="1", impl="reg")
    assert cc.c_acc_conv(ring, True) == 9 * 2 * 4 + 2 + 1 + 1 and cc.c_acc_conv(pack, True) == 2 * 4 + 2 + 1 + 1


def _custom_features(graph, summary, mode):
    """the shape-dependent paths a custom plan takes"""
    levels, launches = cc.parse_plan(summary)
    f = set()
    for L in launches:
        if L.kind == "pool":
            if levels[graph.level[L.pool_in]][2] == 3:
                f.add("pool step reads a tensor with halo 3")
            continue
        couts = [graph.convs[n]["cout"] for n in L.layers]
        lvl = graph.level[graph.convs[L.layers[0]]["bottom"]]
        if L.k == 7 and lvl < 3:
            f.add("k 7 below level 3")
        if L.pool and couts[0] % 16:
            f.add("+pool with a partial 16-channel chunk, passes " + L.passes)
        if L.kind == "conv" and L.coutp - min(couts) >= 64 and L.coutp > -(-min(couts) // 64) * 64:
            f.add("whole 64-channel groups past cout, past the output tensor's padded channels")
        if len(set(couts)) == 2:
            f.add("pair with different cout")
        if L.kind == "conv" and L.cin_p == 32 and L.impl == "reg" and couts[0] != 64 and mode != "fp32":
            f.add("first layer with cout != 64 through pack + 1x1")
        for n in L.layers:
            b = graph.convs[n]["bottom"]
            if b in graph.concats and mode != "fp32":
                for _, off in cn.concat_offsets(graph, b):
                    if off % 2 and "q" in L.passes:
                        f.add("odd slice offset, q block")
                    if off % 2 and "a" in L.passes[1:]:
                        f.add("odd slice offset, lo block")
                    if off % 4 == 0 and off % 8 and off % 64 > 48 and "q" in L.passes:
                        f.add("4-aligned slice across a q group boundary")
    if "lo+q" in cc.tensor_parts(graph, launches).values():
        f.add("tensor with lo and q")
    return f


def test_concat_offsets_restate_the_planner():
    """the 8-aligned layout where it costs no padded channels (the built-in concats: 0 / 128 / 168), packed offsets — odd ones — where it would"""
    g = cc.builtin_graph(0)
    assert cn.concat_offsets(g, "concat_stage2") == [("conv5_5_CPM_L1", 128), ("conv5_5_CPM_L2", 168), ("conv4_4_CPM", 0)]
    assert cn.concat_offsets(cn.net("odd")[1], "cat1") == [("a1", 128), ("a2", 147), ("f", 0)]
    assert cn.concat_offsets(cn.net("single")[1], "cat2") == [("s", 40), ("t", 60), ("u", 0)]


def test_custom_matrix_reaches_the_shape_dependent_paths(graphs):
    r = _r()
    base = set()
    for name in cc.MATRIX:
        base |= cc.plan_keys(r.plan_summary(cc.matrix_config(name)), graphs[cc.MATRIX[name][1]])
    new, feats, every = {}, set(), set()
    for case in CUSTOM_MATRIX:
        graph = cn.net(case[0])[1]
        summary = r.plan_summary(cn.config(*case))
        every |= cc.plan_keys(summary, graph)
        for k in cc.plan_keys(summary, graph) - base:
            new.setdefault(k, cn.case_id(case))
        feats |= _custom_features(graph, summary, case[1])
    print(f"\n{len(new)} instantiations in {len(CUSTOM_MATRIX)} custom configurations that the {len(base)} of the built-in matrix do not have")
    for k, c in sorted(new.items(), key=lambda kv: cc.key_str(kv[0])):
        print(f"  {cc.key_str(k)}  ({c})")
    assert len(new) >= 42
    import re
    keys = [cc.key_str(k) for k in every]
    for needle in (r"k 1 .* tile 128x128 .* reg", r"k 1 .* tile 64x128 .* reg", r"k 1 .* tile 64x64 .* reg", r"^conv pair k 1 .* reg",
                   r"^conv (pair )?k 1 .* reg lowres", r"^conv k 3 .* ring lowres", r"\+pool .* passes 2q", r"\+pool .* passes 3aw", r"k 7 cin_p 224", r"k 7 cin_p 256", r"k 7 cin_p 320",
                   r"^pw2 .* mid 256", r"^pw2 pair .* mid 384 .* lowres"):
        assert any(re.search(needle, k) for k in keys), needle
    # (coutp = round_up(largest cout of the launch, BN) and the branches of a pair have the same round_up(cout, 64): coutp - cout < BN always; what
    #  does occur is whole 64-channel groups of 16-channel chunks past cout — cout 300 on 128-wide tiles, coutp 384, in a tensor padded to 320)
    want = {"+pool with a partial 16-channel chunk, passes 2q", "+pool with a partial 16-channel chunk, passes 3aw", "pool step reads a tensor with halo 3", "k 7 below level 3", "whole 64-channel groups past cout, past the output tensor's padded channels",
            "pair with different cout", "first layer with cout != 64 through pack + 1x1", "odd slice offset, q block", "odd slice offset, lo block",
            "4-aligned slice across a q group boundary", "tensor with lo and q"}
    assert want <= feats, want - feats
    assert {c[1:4] for c in CUSTOM_MATRIX} >= {("mixed", 64, 256)} and len([c for c in CUSTOM_MATRIX if c[4:] == (2, 2)]) == 1
    assert {cn.net(c[0])[2] for c in CUSTOM_MATRIX} == {15, 18}      # an MPI-shaped tail among them


def test_pair_whose_inputs_carry_different_blocks_runs_as_two_launches():
    """odd, mixed @all: b1 is read by d1 (1x1, register-staged kernel, 3aw: a lo block) and by b1k3 (3x3 ring, 2q: a q block), b2 by d2 alone — the tensors
    have different pixel pitches, and a pair has ONE input pitch in its kernel arguments.  Where every layer runs the same passes the pair stays."""
    r = _r()
    steps = lambda mode: [ln.split()[2:5] for ln in r.plan_summary(cn.config("odd", mode, 256, 64)).splitlines() if ln.startswith("step conv d")]
    assert steps("mixed") == [["d1", "k", "1"], ["d2", "k", "1"]]
    for mode in ("f16x3", "fp16", "fp32"):
        assert steps(mode) == [["d1", "+", "d2"]], mode
    g = cn.net("odd")[1]
    _, launches = cc.parse_plan(r.plan_summary(cn.config("odd", "mixed", 256, 64)))
    parts = cc.tensor_parts(g, launches)
    assert (parts["b1"], parts["b2"]) == ("lo+q", "lo")
    for L in launches:      # every remaining pair reads tensors with the same blocks
        if len(L.layers) == 2:
            assert len({parts.get(g.convs[n]["bottom"], "") for n in L.layers}) == 1, L


SMALL_W, SMALL_H = 64, 48


class _Custom:
    """a custom graph at the smallest size, emulated launch by launch"""
    def __init__(self, gname, mode):
        r = _r()
        self.graph = cn.net(gname)[1]
        self.summary = r.plan_summary(cn.config(gname, mode, SMALL_W, SMALL_H))
        self.weights = {n: r.synth_weights(1, n, c["cout"], self.graph.channels[c["bottom"]], c["k"]) for n, c in self.graph.convs.items()}
        self.em = cc.Emulation(self.summary, self.graph, self.weights, _synth.random_frame(1, SMALL_H, SMALL_W, seed=3))
        self.launch = {n: L for L in self.em.launches for n in L.layers + L.layers2}
        self.blob = self.em.blob

    def check(self, only=None):
        names = list(self.weights) + list(self.graph.pools) if only is None else only
        return cc.check_plan(self.summary, self.graph, self.weights, lambda n: self.blob(n), n_interior=10 ** 9, only=names)


@pytest.fixture(scope="module")
def custom():
    return _Lazy(lambda key: _Custom(*key))


@pytest.mark.parametrize("mode", ["fp16", "f16x3", "mixed"])
@pytest.mark.parametrize("gname", list(cn.NETS))
def test_emulated_correct_kernel_passes_every_launch_of_the_custom_graphs(custom, gname, mode):
    t = custom[gname, mode]
    reps = t.check()
    nl = len([ln for ln in t.summary.splitlines() if ln.startswith("step ") and not ln.startswith("step pack")])
    for rep in reps:
        print(f"  {rep.launch!r:60.60s} {cc.key_str(rep.launch.key):100.100s} worst |err|/tol {rep.worst:.3f} over {rep.nchecked} elements")
    print(f"[{gname} {mode}] worst |err|/tol {max(rep.worst for rep in reps):.3f}")
    bad = [str(f) for rep in reps for f in rep.failures]
    assert not bad, bad[:5]
    assert len(reps) == nl and all(rep.nchecked > 0 for rep in reps)
    assert np.array_equal(t.em.blob(t.graph.lowres).shape, (1, 57 if cn.net(gname)[2] == 18 else 44, SMALL_H // 8, SMALL_W // 8))


def _only(rep, layer_dest):
    return rep.nfail > 0 and {(f.layer, f.dest) for f in rep.failures} == layer_dest


def test_planted_stale_last_channels_of_a_130_channel_layer(custom):
    """the 16-channel chunk at channel 128 of b1 (two valid channels) left unwritten: what was in the tensor before stays"""
    t = custom["odd", "mixed"]
    keep = t.em.hi["b1"].copy()
    t.em.hi["b1"][:, 128:] = np.float32(0.25)
    rep = t.check(["b1"])[0]
    t.em.hi["b1"] = keep
    assert _only(rep, {("b1", "b1")}) and {f.ch for f in rep.failures} <= {128, 129}, [str(f) for f in rep.failures]
    assert t.check(["b1"])[0].nfail == 0


@pytest.mark.parametrize("mode", ["f16x3", "mixed"])
def test_planted_odd_offset_slice_one_channel_too_low(custom, mode):
    """a2's slice of cat1 (tensor channel 147, reference channels 19..63) written at 146: every channel of the slice holds its neighbour's value and a1's last channel is overwritten"""
    t = custom["odd", mode]
    off = dict(t.graph.dests("a2"))["cat1"]
    assert off == 19 and dict(cn.concat_offsets(t.graph, "cat1"))["a2"] % 2 == 1

    def shifted(name):
        b = t.em.blob(name)
        if name == "cat1":
            b = b.copy()
            b[:, off - 1:off + 44] = b[:, off:off + 45]
        return b
    t.blob = shifted
    try:
        rep = t.check(["a2"])[0]
    finally:
        t.blob = t.em.blob
    assert rep.nfail > 0 and {f.dest for f in rep.failures} == {"cat1"} and ("a2", "cat1") in {(f.layer, f.dest) for f in rep.failures}, [str(f) for f in rep.failures]
    assert {f.ch for f in rep.failures if f.layer == "a1"} <= {18}
    assert t.check(["a2"])[0].nfail == 0


def test_planted_wrong_channel_offset_of_the_low_res_maps_of_a_single_convolution(custom):
    t = custom["single", "fp16"]
    assert t.graph.lowres == "low" and "low" in t.graph.convs
    t.blob = lambda name: np.roll(t.em.blob(name), 1, axis=1) if name == "low" else t.em.blob(name)
    try:
        rep = t.check(["low"])[0]
    finally:
        t.blob = t.em.blob
    assert rep.launch.lowres and _only(rep, {("low", "low")}), [str(f) for f in rep.failures]
    assert t.check(["low"])[0].nfail == 0


def test_planted_swapped_branches_of_a_1x1_pair_on_the_register_staged_kernel(custom):
    t = custom["odd", "f16x3"]
    L = t.launch["d1"]
    assert L.layers == ["d1", "d2"] and L.k == 1 and L.impl == "reg"
    t.em.store("d1", t.em.pre["d2"]); t.em.store("d2", t.em.pre["d1"])
    rep = t.check(["d1"])[0]
    t.em.store("d1", t.em.pre["d1"]); t.em.store("d2", t.em.pre["d2"])
    assert _only(rep, {("d1", "d1"), ("d2", "d2")}), [str(f) for f in rep.failures]
    assert t.check(["d1"])[0].nfail == 0


def test_planted_dropped_lo_part_of_the_tensor_with_lo_and_q(custom):
    """f's own tensor carries lo (read by the 1x1 layer fk1, 3aw) and q (read by a1 + a2, 2q): without the lo block its export is 2^-12 off, against a bound
    of 2^-22; its slice of cat1 carries a q block only and stays inside its bound"""
    t = custom["odd", "mixed"]
    assert t.em.parts["f"] == "lo+q" and t.em.parts["cat1"] == "q" and t.launch["fk1"].passes == "3aw" and t.launch["a1"].passes == "2q"
    keep = t.em.lo["f"]
    t.em.lo["f"] = np.zeros_like(keep)
    rep = t.check(["f"])[0]
    t.em.lo["f"] = keep
    assert _only(rep, {("f", "f")}), [str(f) for f in rep.failures]
    assert t.check(["f"])[0].nfail == 0


# ------------------------------------------------------------------------------------------------------------
# plans of many images per launch (tests/_manycases.py)
# ------------------------------------------------------------------------------------------------------------
def _old_classes(graphs):
    """kernel classes of every plan of the three older matrices"""
    r = _r()
    old = set()
    for name, t in cc.MATRIX.items():
        old |= mc.classes(t[0], cc.parse_plan(r.plan_summary(cc.matrix_config(name)))[1])
    for name, t in cc.BATCH_MATRIX.items():
        old |= mc.classes(t[0], cc.parse_plan(r.plan_summary(cc.batch_config(name)))[1])
    for c in CUSTOM_MATRIX:
        old |= mc.classes(c[1], cc.parse_plan(r.plan_summary(cn.config(*c)))[1])
    return old


def test_many_image_cases_reach_the_seven_classes_no_older_case_runs(graphs):
    r = _r()
    old = _old_classes(graphs)
    assert len(old) == 55
    plans = {name: cc.parse_plan(r.plan_summary(cc.matrix_config(name, mc.CONV_MATRIX)))[1] for name in mc.CONV_MATRIX}
    new = {name: mc.classes(mc.CONV_MATRIX[name][0], la) - old for name, la in plans.items()}
    for cls, case in mc.NEW_CLASSES.items():      # first: a case taken out of CONV_MATRIX fails HERE, with the class it was added for in the message
        assert cls not in old, f"{cls} is run by an older case"
        reached_by = {name for name, cl in new.items() if cls in cl}
        assert reached_by == {case}, f"class {cls} (added for: {case}) is reached by {sorted(reached_by) or 'no case'}"
    assert len(mc.NEW_CLASSES) == 7 and set(mc.NEW_CLASSES.values()) == set(mc.CONV_MATRIX)
    assert set().union(*new.values()) == set(mc.NEW_CLASSES)          # ... and the cases add nothing that is not on the list
    # the ring kernel's 64x128 tile in every mode and pass label
    assert {(c[0], c[5]) for c in mc.NEW_CLASSES if c[2:4] == ("ring", "64x128")} == {("fp16", "1"), ("fp32", "1"), ("mixed", "1"), ("mixed", "2q"), ("f16x3", "3aw")}
    # its k-split is on record in the bound: KSPLIT 2, the reduction of one more partial
    for la in plans.values():
        for L in la:
            if L.kind == "conv" and L.tile == (64, 128):
                assert cc.ksplit_of(L) == 2
    # the same plan runs the full batches of tests/test_batch_launches.py
    assert mc.BATCH_MATRIX["fp16_coco_96x64_5s_b2"] == mc.CONV_MATRIX["fp16_coco_96x64_5s_b2"]
    both = cc.parse_plan(r.plan_summary(cc.batch_config("fp16_coco_96x64_5s_b2", matrix=mc.BATCH_MATRIX)))[1]
    assert ("fp16", "conv", "ring", "64x128", 128, "1", False) in mc.classes("fp16", both)


def test_many_image_cases_reach_the_image_counts_and_grid_remainders(graphs):
    r = _r()
    entries = [(t, r.plan_summary(cc.matrix_config(n, mc.CONV_MATRIX))) for n, t in mc.CONV_MATRIX.items()]
    entries += [(t, r.plan_summary(cc.batch_config(n, matrix=mc.BATCH_MATRIX))) for n, t in mc.BATCH_MATRIX.items()]
    counts = {t[4] * t[6] for t, _ in entries}
    assert mc.IMAGE_COUNTS <= counts, mc.IMAGE_COUNTS - counts
    older = {t[4] * t[6] for t in list(cc.MATRIX.values()) + list(cc.BATCH_MATRIX.values())} | {c[4] * c[5] for c in CUSTOM_MATRIX}
    assert max(older) == 6                                              # what the suite stopped at
    assert max(t[4] for t, _ in entries) == 16 and max(t[6] for t, _ in entries) == 16     # the accepted limits of num_scales and batch_frames
    for impl in ("ring", "reg", "pw2"):      # grids that are and are not a multiple of 8 workgroups, per kernel: the q / r split of the XCD remap
        rem = {L.wgs % 8 == 0 for _, s in entries for L in cc.parse_plan(s)[1] if L.impl == impl}
        assert rem == {True, False}, (impl, rem)
    for t, s in entries:                      # conv_first: one workgroup per image row of every image
        first = [L for L in cc.parse_plan(s)[1] if L.kind == "first"]
        assert all(L.wgs == t[3] * t[4] * t[6] for L in first)
    assert any(L.kind == "first" and L.wgs == 48 * 32 for t, s in entries for L in cc.parse_plan(s)[1])       # 32 images of 48 rows

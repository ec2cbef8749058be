"""Every convolution launch ALONE against float64, element by element (tests/_convcheck.py has the method and the derivation of the bound).

One case per configuration of _convcheck.MATRIX; a case checks EVERY launch of its plan: the production library, the built-in graphs, the
default plan (no keep_blobs, no experiment knobs).  The input of a launch is the engine's own blob after one rtp_forward_heatmaps, so the
tolerance of a launch holds no upstream error:  tol = u_out*|r| + (c_acc*2^-24 + e_op)*S + a_min  per element, nothing fitted.  Sampled per
image and launch: the first and last 4 rows and columns in full, the first and last pixel of every workgroup's tile, a seeded interior set.
tests/test_conv_launches_cpu.py keeps the matrix a superset of the kernel instantiations bench.py's plans run.

The tapped forward runs ONE frame: a batch_frames 2 case runs that plan's tiles (chosen for 2 x N images per launch) on half the grid.
Full batches — every image of every frame, through rtp_submit / rtp_collect and the captured graphs — are checked blob by blob in
tests/test_batch_launches.py.

Time: a case costs the engine build + one forward (what a tests/test_precision.py case pays too) plus the float64 reference of the
sampled pixels; both are printed, profiles/conv_launch_check.txt has them for every case.

A second set of cases (tests/_customnets.py CUSTOM_MATRIX) runs graphs other than the built-in one through proto_path, at sizes of a few
thousand pixels: 1x1 layers on the register-staged kernel, concat slices at odd channel offsets, output-channel tails other than 19 / 38 / 28,
7x7 layers below 1/8 resolution, one convolution writing the low-res maps, a tensor with a lo and a q block (tests/test_conv_launches_cpu.py
asserts what they reach).

A third set (tests/_manycases.py CONV_MATRIX) runs plans of 7, 10 and 13 images per launch — 5 to 13 scales on nets of 64x48 to 160x96 — for
the seven kernel classes the planner picks only there, the ring kernel's 64x128 tile in every mode among them; same body, same bound."""
import time

import numpy as np
import pytest

import _convcheck as cc
import _customnets as cn
import _manycases as mc
import _synth

pytestmark = pytest.mark.gpu

INTERIOR = 128        # random interior pixels per image and launch (borders and tile ends are never cut)
_graphs = {}


def _check_every_launch(name, cfg, graph, mode, N, B, frame_seed):
    """one engine, one forward, every launch of its plan alone against float64"""
    import caffe_rtpose_amd as r
    W, H = cfg.c.net_w, cfg.c.net_h
    t0 = time.time()
    e = r.Engine(cfg)
    t1 = time.time()
    layers = e.conv_layers()
    assert [(n, ci, co, k) for n, ci, co, k in layers] == [(n, graph.channels[c["bottom"]], c["cout"], c["k"]) for n, c in graph.convs.items()]
    weights = {n: e.get_conv_weights(i) for i, (n, *_rest) in enumerate(layers)}
    x = _synth.random_frame(N, H, W, seed=frame_seed)
    t2 = time.time()
    heat = e.forward_heatmaps(x)
    t3 = time.time()
    assert np.array_equal(heat, e.get_blob(graph.lowres))

    def blob(nm):
        return x if nm == graph.input else heat if nm == graph.lowres else e.get_blob(nm)

    summary = r.plan_summary(e.cfg)
    reps = cc.check_plan(summary, graph, weights, blob, fp32=(mode == "fp32"), n_interior=INTERIOR // N, seed=11, images_per_launch=N * B)
    t4 = time.time()
    e.close()
    nl = len([ln for ln in summary.splitlines() if ln.startswith("step ") and not ln.startswith("step pack")])
    assert len(reps) == nl and all(rep.nchecked > 0 for rep in reps)       # every launch of the plan was checked
    print(f"\n[convcheck] case {name}: {nl} launches, {sum(rep.npixels for rep in reps)} pixels, {sum(rep.nchecked for rep in reps)} elements; "
          f"engine build {t1 - t0:.2f} s, forward {t3 - t2:.2f} s, taps + float64 reference {t4 - t3:.2f} s")
    for key, worst in sorted(cc.summarize(reps).items(), key=lambda kv: cc.key_str(kv[0])):
        print(f"[convcheck] {name} | {cc.key_str(key)} | worst |err|/tol {worst:.4f}")
    bad = [rep for rep in reps if rep.nfail]
    for rep in bad:
        print(f"[convcheck] FAIL {rep.launch!r}: {rep.nfail} of {rep.nchecked} elements, worst |err|/tol {rep.worst:.3g}")
        for (dest, cls), (n, nf, worst) in rep.by_class.items():
            print(f"    -> {dest} {cls}: {nf} of {n} elements, worst {worst:.3g}")
        for f in rep.failures[:8]:
            print(f"    {f}")
    assert not bad, f"{len(bad)} launches outside their bound, first: {bad[0].failures[0]}"


@pytest.mark.parametrize("name", list(cc.MATRIX))
def test_every_launch_alone_against_float64(name):
    mode, model, W, H, N, gap, B, wseed = cc.MATRIX[name]
    if model not in _graphs:
        _graphs[model] = cc.builtin_graph(model)
    _check_every_launch(name, cc.matrix_config(name), _graphs[model], mode, N, B, 3 if wseed == 1 else 100 + wseed)


@pytest.mark.parametrize("case", cn.CUSTOM_MATRIX, ids=cn.case_id)
def test_every_launch_of_a_custom_graph_alone_against_float64(case):
    gname, mode, W, H, N, B = case
    _check_every_launch(cn.case_id(case), cn.config(*case), cn.net(gname)[1], mode, N, B, 3)


@pytest.mark.parametrize("name", list(mc.CONV_MATRIX))
def test_every_launch_of_a_many_image_plan_alone_against_float64(name):
    mode, model, W, H, N, gap, B, wseed = mc.CONV_MATRIX[name]
    if model not in _graphs:
        _graphs[model] = cc.builtin_graph(model)
    _check_every_launch(name, cc.matrix_config(name, mc.CONV_MATRIX), _graphs[model], mode, N, B, 3)

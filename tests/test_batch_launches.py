"""FULL batches blob by blob: every image of every frame of a batch, as rtp_submit / rtp_collect ran it — graph replay included.

tests/test_conv_launches.py checks every launch of a plan on ONE frame (the taps run slot 0 with nimg = N).  What the benchmark runs is a
full batch, nframes * N images per launch, replayed from a captured graph, several batch contexts in flight.  Decided by the full image count
and by nothing else: the XCD remap of blockIdx.x in decode_block (with its q / r split where the grid is no multiple of 8), img = tile /
tiles_per_img for the images behind the first frame's, the seam between frame j's last image and frame j + 1's first in the arena, conv_first's
H * NI rows, the pooling and packing launches, the planar store of the later images into the low-res maps, the per-slot staging offsets of the
input, the separately captured partial-batch graphs, a second context beside the first.  rtp_get_batch_blob returns what such a batch left
behind; the cases are _convcheck.BATCH_MATRIX (tests/test_conv_launches_cpu.py asserts what they reach).

(a) test_batch_blobs_equal_single_frame_blobs: 2B + max(B - 1, 1) DIFFERENT frames; each tapped alone (every materialised blob, the low-res
    maps, forward_debug's joints), then two full batches in flight on two contexts and a partial batch behind them.  Every blob of frame j of a
    batch must hold the bits of that frame tapped alone — whole tensors, no sampling (tests/_batchcheck.py has the argument); the tags name the
    frames, the input blob is the submitted tensors, the joints are forward_debug's.  In both execution modes.
(b) test_every_launch_of_a_full_batch_against_float64: for three cases, one full batch in GRAPH mode and _convcheck.check_plan over all
    N * B images with the bound of tests/_convcheck.py, unchanged.  It never runs the one-frame tap: the independent half.

(c) the same two bodies over tests/_manycases.py BATCH_MATRIX: 10 and 32 images per launch (5 and 16 scales, batch_frames 2) and batch_frames 16
    (47 frames, a partial batch of 15), every frame tapped alone — image indices past 8, the q / r split of the XCD remap on those grids, the arena
    seams between up to 32 images, conv_first's H * 32 rows.

Times are printed per case in the `[convcheck]` style; profiles/conv_launch_check.txt has them."""
import re
import time

import numpy as np
import pytest

import _batchcheck as bc
import _convcheck as cc
import _manycases as mc
import _synth

pytestmark = pytest.mark.gpu

INTERIOR = 128        # random interior pixels per launch, shared by its images (borders and tile ends are never cut)
_graphs = {}


def _graph(model):
    if model not in _graphs:
        _graphs[model] = cc.builtin_graph(model)
    return _graphs[model]


def _materialised(e, graph, summary):
    """blob names rtp_get_blob serves for this plan — every blob of the graph but the un-pooled input of a pooling epilogue and the middle blob of a
    fused branch tail (asserted against the engine), without the low-res blob"""
    import caffe_rtpose_amd as r
    _, launches = cc.parse_plan(summary)
    hidden = {n for L in launches if L.pool or L.kind == "pw2" for n in L.layers}
    names = [n for n in list(graph.convs) + list(graph.pools) + list(graph.concats) if n != graph.lowres]
    for n in hidden:
        with pytest.raises(r.RtpError):
            e.get_blob(n)
    return [n for n in names if n not in hidden]


def _outcome(call):
    """(tag, joints) of a frame's post-processing, or (None, None) where connect refuses the frame with RTP_ERANGE: on a net that is taller than wide the
    reference CHECK-fails on PAF sample coordinates of noise maps (postproc.hip, `bad`), and the engine reports that for the frame, alone or in a batch"""
    import caffe_rtpose_amd as r
    try:
        tag, n, joints = call()
    except r.RtpError as err:
        if err.code != r.RTP_ERANGE:
            raise
        return None, None
    assert n == len(joints)
    return tag, joints


def _collect(e, k):
    """outcomes of the next k frames, in FIFO order"""
    return [_outcome(e.collect) for _ in range(k)]


@pytest.mark.parametrize("exec_mode", ["graph", "eager"])
@pytest.mark.parametrize("name", list(cc.BATCH_MATRIX))
def test_batch_blobs_equal_single_frame_blobs(name, exec_mode):
    _batch_blobs_equal_single_frame_blobs(name, exec_mode, cc.BATCH_MATRIX)


@pytest.mark.parametrize("exec_mode", ["graph", "eager"])
@pytest.mark.parametrize("name", list(mc.BATCH_MATRIX))
def test_many_image_batch_blobs_equal_single_frame_blobs(name, exec_mode):
    _batch_blobs_equal_single_frame_blobs(name, exec_mode, mc.BATCH_MATRIX)


def _batch_blobs_equal_single_frame_blobs(name, exec_mode, matrix):
    import caffe_rtpose_amd as r
    mode, model, W, H, N, gap, B, wseed = matrix[name]
    graph = _graph(model)
    t0 = time.time()
    e = r.Engine(cc.batch_config(name, exec_mode=r.EXEC_GRAPH if exec_mode == "graph" else r.EXEC_EAGER, matrix=matrix))
    t1 = time.time()
    summary = r.plan_summary(e.cfg)
    names = _materialised(e, graph, summary)
    nfr = 2 * B + max(B - 1, 1)
    xs = [_synth.random_frame(N, H, W, seed=40 + i) for i in range(nfr)]
    assert all(not np.array_equal(xs[i], xs[j]) for i in range(nfr) for j in range(i))
    # ---- every frame alone: slot 0 of context 0, nimg = N
    single = []
    for x in xs:
        heat = e.forward_heatmaps(x)
        s = {nm: e.get_blob(nm) for nm in names}
        s[graph.lowres], s[graph.input] = heat, x
        def debug():
            d = e.forward_debug(x)
            assert np.array_equal(d["lowres"], heat)
            return 0, d["num_people"], d["joints"][:d["num_people"]].copy()
        s["joints"] = _outcome(debug)[1]
        single.append(s)
    got, tags = e.get_batch_blob(0, graph.lowres)          # a one-frame tap counts as a batch of one frame on context 0 ...
    assert len(tags) == 1 and np.array_equal(got, single[-1][graph.lowres])
    nctx = int(re.search(r"^streams contexts (\d+)", summary, re.M).group(1))
    assert nctx >= 2
    for ci in range(1, nctx):                                # ... and no other context has run a batch yet
        with pytest.raises(r.RtpError, match="has not run a batch"):
            e.get_batch_blob(ci, graph.lowres)
    t2 = time.time()
    t_batch = t_read = 0.0
    nbytes = 0
    all_diffs = []

    def check_contexts(expect):
        """expect: context -> [frame index per slot]: tags, input, every blob, bit for bit"""
        nonlocal t_read, nbytes
        t = time.time()
        for ci, frames in expect.items():
            blobs = {}
            for nm in names + [graph.lowres, graph.input]:
                blobs[nm], tags = e.get_batch_blob(ci, nm)
                assert tags == [100 + f for f in frames], (ci, nm, tags, frames)
                assert blobs[nm].shape[0] == len(frames) * N
                nbytes += blobs[nm].nbytes
            diffs, counts = bc.compare_batch(blobs, [single[f] for f in frames], N)
            for d in diffs:
                print(f"[batchcheck] {name} {exec_mode} context {ci} frames {frames}: {d}")
            all_diffs.extend((ci, d) for d in diffs)
        t_read += time.time() - t

    def run(frames):
        nonlocal t_batch
        t = time.time()
        for f in frames:
            e.submit(xs[f], tag=100 + f)
        if len(frames) % B:
            e.flush()
        got = _collect(e, len(frames))
        t_batch += time.time() - t
        for f, (tag, joints) in zip(frames, got):
            want = single[f]["joints"]
            assert (joints is None) == (want is None), f"frame {f}: connect refused the frame on one side only"
            assert want is None or (tag == 100 + f and np.array_equal(joints, want)), f"frame {f}: joints differ from forward_debug's"

    # ---- two full batches in flight on two contexts
    run(list(range(2 * B)))
    check_contexts({0: list(range(B)), 1: list(range(B, 2 * B))})
    # ---- the partial batch, with its own graph; the context it did not take still holds its full batch
    part = list(range(2 * B, nfr))
    run(part)
    ran = [ci for ci in (0, 1) if e.get_batch_blob(ci, graph.lowres)[1] == [100 + f for f in part]]
    assert len(ran) == 1, "the partial batch ran on one of the two contexts"
    check_contexts({ran[0]: part, 1 - ran[0]: list(range(B)) if ran[0] == 1 else list(range(B, 2 * B))})
    for ci in (-1, nctx):
        with pytest.raises(r.RtpError):
            e.get_batch_blob(ci, graph.lowres)
    e.submit(xs[0], tag=1)                                   # idle engines only
    with pytest.raises(r.RtpError):
        e.get_batch_blob(0, graph.lowres)
    e.flush()
    _collect(e, 1)
    e.close()
    print(f"\n[convcheck] batch case {name} {exec_mode}: {nfr} frames of {N} images, {len(names) + 2} blobs, {nbytes / 1e6:.0f} MB compared bit for bit; "
          f"engine build {t1 - t0:.2f} s, single-frame taps {t2 - t1:.2f} s, batches {t_batch:.2f} s, read-back + compare {t_read:.2f} s")
    assert not all_diffs, f"{len(all_diffs)} blobs of a batch differ from the frame tapped alone, first: context {all_diffs[0][0]}, {all_diffs[0][1]}"


@pytest.mark.parametrize("name", list(cc.BATCH_FLOAT64))
def test_every_launch_of_a_full_batch_against_float64(name):
    _every_launch_of_a_full_batch_against_float64(name, cc.BATCH_MATRIX)


@pytest.mark.parametrize("name", list(mc.BATCH_FLOAT64))
def test_every_launch_of_a_many_image_batch_against_float64(name):
    _every_launch_of_a_full_batch_against_float64(name, mc.BATCH_MATRIX)


def _every_launch_of_a_full_batch_against_float64(name, matrix):
    import caffe_rtpose_amd as r
    mode, model, W, H, N, gap, B, wseed = matrix[name]
    graph = _graph(model)
    t0 = time.time()
    e = r.Engine(cc.batch_config(name, exec_mode=r.EXEC_GRAPH, matrix=matrix))
    t1 = time.time()
    layers = e.conv_layers()
    weights = {n: e.get_conv_weights(i) for i, (n, *_rest) in enumerate(layers)}
    xs = [_synth.random_frame(N, H, W, seed=60 + i) for i in range(B)]
    t2 = time.time()
    for j, x in enumerate(xs):
        e.submit(x, tag=j)
    got = _collect(e, B)
    t3 = time.time()
    assert all(tag in (j, None) for j, (tag, _) in enumerate(got))
    cache = {}

    def blob(nm):
        if nm not in cache:
            cache[nm], tags = e.get_batch_blob(0, nm)
            assert tags == list(range(B)) and cache[nm].shape[0] == N * B
        return cache[nm]

    assert np.array_equal(blob(graph.input), np.concatenate(xs))
    summary = r.plan_summary(e.cfg)
    reps = cc.check_plan(summary, graph, weights, blob, fp32=(mode == "fp32"), n_interior=INTERIOR // (N * B), seed=11, images_per_launch=N * B)
    t4 = time.time()
    e.close()
    nl = len([ln for ln in summary.splitlines() if ln.startswith("step ") and not ln.startswith("step pack")])
    assert len(reps) == nl and all(rep.nchecked > 0 for rep in reps)       # every launch of the plan was checked, over N * B images
    print(f"\n[convcheck] full-batch case {name}: {nl} launches, {N * B} images, {sum(rep.npixels for rep in reps)} pixels, {sum(rep.nchecked for rep in reps)} elements; "
          f"engine build {t1 - t0:.2f} s, batch {t3 - t2:.2f} s, read-back + float64 reference {t4 - t3:.2f} s")
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

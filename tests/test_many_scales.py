"""4 to 16 scales and batches of 16 frames on the GPU: pre-processing, ImResize, fused NMS, connect, the frame pipeline, the CLI.

The cases and what each is there for are in tests/_manycases.py; tests/test_many_scales_cpu.py asserts, without a device, what they reach (which
area-pad group holds which kind of level, where the clamps of the smallest crop are active, that the oracle accepts every case).  The convolution
launches of many images are cases of tests/test_conv_launches.py and tests/test_batch_launches.py.

  * device pre-processing at 5, 9 and 16 scales: launch_area_pad issues one launch per group of four scales (4 + 1, 4 + 4 + 1, 4 x 4) with a
    scale_base offset; debug_preprocess == rtp_preprocess_frame == the independent OpenCV restatement (tests/_cvref.py), on synthetic content and noise
  * the frame pipeline behind it: submit_frame at 9 scales == host preprocess + submit, graph replay == eager launches (the first captured graph with
    more than one area-pad launch); submit_frame_device at 5 scales; the residency stamp of the area-pad slot
  * ImResize at 4, 5, 7, 11, 13 and 16 scales, crops down to 2x2 low-res cells, against the oracle
  * the production post-processing (fused ImResize + NMS, fused pair kernel) at 5, 9 and 16 scales against oracle ImResize -> Nms -> connect, and the
    map-materialising taps against it
  * one frame pipeline at 16 scales with the renderer behind it; the accepted extremes num_scales 16 x batch_frames 16; rtp_set_scales at 16 scales
  * rtpose.bin --num_scales 6

Every comparison is np.array_equal / == (the rendered frame: the boundary-pixel allowance of test_rendered_frame_matches_oracle)."""
import os
import subprocess

import numpy as np
import pytest

import _manycases as mc
import _oracle as orc
import _synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")


def _engine(**kw):
    import caffe_rtpose_amd as r
    return r.Engine(r.Config(**kw))


# ------------------------------------------------------------------------------------------
# pre-processing: area_pad_kernel in groups of four scales
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.PREP_CASES, ids=lambda c: f"{c[0]}-{c[1]}s")
def test_device_preprocess_in_groups_of_four_scales_bit_exact(case):
    import caffe_rtpose_amd as r
    import _cvref
    fw, fh, dw, dh, W, H, N, start, gap = mc.prep_geom(case)
    e = _engine(net_w=W, net_h=H, num_scales=N, start_scale=start, scale_gap=gap, disp_w=dw, disp_h=dh, frames_in_flight=1)
    for img in mc.prep_frames(case):
        want_x, want_disp, want_fs = r.preprocess_frame(img, dw, dh, W, H, N, start, gap)
        ref_x, ref_disp, ref_fs = _cvref.producer_frame(img, dw, dh, W, H, N, start, gap, orc.process_and_pad_image)
        x, disp, fs = e.debug_preprocess(img)
        assert x.shape == (N, 3, H, W)
        assert fs == want_fs == ref_fs
        assert np.array_equal(disp, want_disp) and np.array_equal(disp, ref_disp)
        for i in range(N):      # level by level: a wrong scale_base or group size shows as the FIRST level of a group
            assert np.array_equal(x[i], want_x[i]), f"level {i} (group {i // 4}, {mc.prep_kinds(case)[i][1]}) differs from rtp_preprocess_frame"
            assert np.array_equal(x[i], ref_x[i]), f"level {i} (group {i // 4}) differs from the OpenCV restatement"
    e.close()


def test_submit_frame_at_9_scales_equals_host_preprocess_plus_submit_graph_and_eager():
    """three area-pad launches per frame, captured into the batch graph's input side: submit_frame == preprocess_frame + submit, graph == eager, replays included"""
    import caffe_rtpose_amd as r
    W, H, N, dw, dh = 160, 96, 9, 96, 64          # display below the net: linear, identity, area and fast levels (tests/_manycases.py)
    gap = mc.gap(N)
    kw = dict(net_w=W, net_h=H, num_scales=N, scale_gap=gap, disp_w=dw, disp_h=dh, frames_in_flight=4, batch_frames=2)
    eg = _engine(exec_mode=r.EXEC_GRAPH, **kw)
    ee = _engine(exec_mode=r.EXEC_EAGER, **kw)
    for e in (eg, ee):
        t = r.default_thresholds(0)
        e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], 2, 0.05)   # keep more "people" of the noise maps
    imgs = [r.synth_frame(200, 150, i, seed=33) for i in range(5)]     # two full batches + a partial one (its own capture)
    xs = [r.preprocess_frame(im, dw, dh, W, H, N, 1.0, gap)[0] for im in imgs]

    def run(e, frames):
        out = []
        for rep in range(2):      # the second pass replays what the first captured
            for i in range(len(imgs)):
                if frames:
                    e.submit_frame(imgs[i], tag=10 * rep + i)
                else:
                    e.submit(xs[i], tag=10 * rep + i)
                while e.in_flight() >= 4:
                    out.append(e.collect())
            while e.in_flight():
                out.append(e.collect())
        return out

    want = run(ee, False)
    assert sum(n for _, n, _ in want) > 0
    for e, frames in ((eg, True), (ee, True), (eg, False)):
        got = run(e, frames)
        assert [t for t, _, _ in got] == [t for t, _, _ in want]
        for (t, n, j), (_, wn, wj) in zip(got, want):
            assert n == wn and np.array_equal(j, wj), (frames, t)
    eg.close()
    ee.close()


def test_submit_frame_device_at_5_scales_equals_submit_frame():
    """a frame in device memory read in place (warp from the caller's view, then two area-pad launches): same joints as the host frame, at the
    display size (the import kernel) and off it (the warp)"""
    import torch
    import caffe_rtpose_amd as r
    W, H, N, dw, dh = 160, 96, 5, 160, 96
    e = _engine(net_w=W, net_h=H, num_scales=N, scale_gap=mc.gap(N), disp_w=dw, disp_h=dh, frames_in_flight=2)
    t = r.default_thresholds(0)
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], 2, 0.05)
    people = 0
    for i, (fw, fh) in enumerate(((160, 96), (200, 150), (320, 192))):
        img = r.synth_frame(fw, fh, i, seed=41)
        fs = e.submit_frame(img, tag=2 * i)
        want = e.collect()
        frame = torch.from_numpy(img.copy()).cuda()
        torch.cuda.synchronize()
        fs2 = e.submit_frame_device(frame, tag=2 * i + 1)
        got = e.collect()
        assert fs2 == fs and got[0] == 2 * i + 1 and got[1] == want[1] and np.array_equal(got[2], want[2]), (fw, fh)
        x = r.preprocess_frame(img, dw, dh, W, H, N, 1.0, mc.gap(N))[0]
        assert np.array_equal(e.debug_preprocess(img)[0], x)
        people += want[1]
    assert people > 0
    e.close()


def test_area_pad_stamp_of_several_launches_is_one_span_per_frame():
    """launch_area_pad hands every group's launch the same stamp slot (200 + 2 j + 1): the slot holds min(start), max(end) over the workgroups of
    ALL its launches — one span per frame from the first group's first workgroup to the last group's last one, whatever the number of groups —
    and the probe does not change results.  That the span covers ALL groups follows from the code (kernels.h KStamp: atomicMax on ~start and on
    end; stamp_harvest reads and zeroes the slot once per batch), not from the assertions here: they say one row per frame (not one per launch),
    end behind start, and not before the warp the launches read — a span of the last group alone would meet them too."""
    import caffe_rtpose_amd as r
    W, H, N, dw, dh = 160, 96, 9, 320, 180
    e = _engine(net_w=W, net_h=H, num_scales=N, scale_gap=mc.gap(N), disp_w=dw, disp_h=dh, frames_in_flight=1, exec_mode=r.EXEC_EAGER)
    img = r.synth_frame(200, 150, 0, seed=71)
    e.submit_frame(img, tag=1)
    want = e.collect()
    assert len(e.stamp_probe(1)) == 0
    for i in range(3):
        e.submit_frame(img, tag=i)
        got = e.collect()
        assert got[1] == want[1] and np.array_equal(got[2], want[2])
    st = e.stamp_probe(-1)
    e.stamp_probe(0)
    pad = st[st[:, 0] == 201.0]
    assert len(pad) == 3 and (pad[:, 2] > pad[:, 1]).all(), pad             # three frames, three spans: not one per launch
    warp = st[st[:, 0] == 200.0]
    assert len(warp) == 3 and (pad[:, 1] >= warp[:, 1]).all()               # the area-pad launches start behind the warp they read
    e.close()


# ------------------------------------------------------------------------------------------
# ImResize, fused NMS + connect
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,W,H,N,start,gap", mc.RESIZE_CASES)
def test_resize_many_scales_bit_exact(model, W, H, N, start, gap):
    e = _engine(model=model, net_w=W, net_h=H, num_scales=N, start_scale=start, scale_gap=gap, frames_in_flight=1)
    low = _synth.smooth_field(N * e.heat_channels, H // 8, W // 8, seed=3).reshape(N, e.heat_channels, H // 8, W // 8)
    low = np.ascontiguousarray(low + 0.25 * np.random.default_rng(9).standard_normal(low.shape), np.float32)      # cell-to-cell contrast: a 2x2 crop of a smooth field is almost flat
    got = e.resize(low)
    ref = orc.imresize(low, W, H, start, gap)[0]
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {ref.size} elements differ, max diff {np.abs(got - ref).max()}"
    e.close()


@pytest.mark.parametrize("case", mc.FUSED_CASES, ids=lambda c: f"m{c[0]}-{c[1]}x{c[2]}-{c[3]}s-{c[6]}")
def test_fused_postproc_many_scales_bit_exact(case):
    model, W, H, N, start, gap, kind = case
    ref = mc.fused_reference(case)
    e = _engine(model=model, net_w=W, net_h=H, num_scales=N, start_scale=start, scale_gap=gap, frames_in_flight=1)
    assert e.max_peaks == ref["max_peaks"] and e.get_thresholds() == ref["thr"]
    low = ref["low"]
    assert low.shape == (N, e.heat_channels, H // 8, W // 8)
    peaks, joints, n = e.post_from_lowres(low)
    assert np.array_equal(peaks, ref["peaks"])
    assert n == ref["n"] and np.array_equal(joints[:n], ref["joints"])
    if kind != "noise":
        assert n >= 1
    # the map-materialising taps: resize -> nms -> connect
    res = e.resize(low)
    assert np.array_equal(res, ref["res"])
    pk = e.nms(res)
    assert np.array_equal(pk, ref["peaks"])
    n2, j2 = e.connect(res, pk)
    assert n2 == n and np.array_equal(j2[:n2], ref["joints"])
    peaks3, joints3, n3 = e.post_from_lowres(low)                       # and once more: nothing of the first run is left behind
    assert n3 == n and np.array_equal(peaks3, ref["peaks"]) and np.array_equal(joints3[:n3], ref["joints"])
    e.close()


# ------------------------------------------------------------------------------------------
# the frame pipeline at 16 scales, the accepted extremes
# ------------------------------------------------------------------------------------------
def test_frame_pipeline_at_16_scales_matches_taps_oracle_and_renders():
    """submit_frame / collect_rendered at 16 scales (four area-pad launches, 16 images per conv launch, scale loops of 16 behind them) == the taps on
    the same frame == the oracle's post-processing of the engine's own low-res maps; the rendered frame is the oracle's (allowance for ellipse-boundary
    pixels as in test_rendered_frame_matches_oracle: ocml against glibc trigonometry)"""
    import caffe_rtpose_amd as r
    W, H, N, dw, dh = 160, 96, 16, 320, 180
    gap = mc.gap(N)
    e = _engine(net_w=W, net_h=H, num_scales=N, scale_gap=gap, disp_w=dw, disp_h=dh, frames_in_flight=2, render=1)
    thr = dict(orc.default_thresholds(0), min_subset_cnt=2, min_subset_score=0.05)      # keep more "people" of the noise maps
    e.set_thresholds(thr["nms_threshold"], thr["inter_threshold"], thr["inter_min_above"], thr["min_subset_cnt"], thr["min_subset_score"])
    total = 0
    for i in range(2):
        img = r.synth_frame(400, 300, i, seed=13)
        x, disp, fs = r.preprocess_frame(img, dw, dh, W, H, N, 1.0, gap)
        assert e.submit_frame(img, tag=i) == fs
        tag, n, joints, got = e.collect_rendered()
        d = e.forward_debug(x)
        assert tag == i and n == d["num_people"] and np.array_equal(joints, d["joints"][:n])
        ref_res = orc.imresize(d["lowres"], W, H, 1.0, gap)[0]
        assert np.array_equal(d["resized"], ref_res)
        ref_peaks = orc.nms(ref_res, 18, 64, thr["nms_threshold"], d["peaks"])
        assert np.array_equal(d["peaks"], ref_peaks)
        rn, rj = orc.connect(0, ref_res, ref_peaks, 64, W, H, dw, dh, thr)
        assert rn == n and np.array_equal(rj[:rn], joints)
        want = orc.render_pose(0, disp, joints, n)
        bad = (got != want).any(-1)
        assert bad.mean() < 5e-4, f"{int(bad.sum())} pixels differ"
        total += n
    assert total > 0, "the test frames produced no people: nothing was drawn"
    e.close()


def test_engine_with_16_scales_and_batches_of_16_frames_runs_and_set_scales_matches_a_fresh_engine():
    """the accepted extremes of rtp_engine_create (tests/test_host_cpu.py checks that 17 scales are refused): 256 images per convolution launch"""
    import caffe_rtpose_amd as r
    W, H, N, B, dw, dh = 64, 48, 16, 16, 128, 96
    kw = dict(net_w=W, net_h=H, num_scales=N, disp_w=dw, disp_h=dh, frames_in_flight=B, batch_frames=B)
    e = _engine(scale_gap=mc.gap(N), **kw)
    xs = [_synth.random_frame(N, H, W, seed=70 + i) for i in range(B)]
    alone = [e.forward_debug(x) for x in xs]                             # every frame alone: 16 images per launch
    for i, x in enumerate(xs):
        e.submit(x, tag=i)
    assert e.in_flight() == B
    for i in range(B):                                                   # one full batch: 256 images per launch
        tag, n, joints = e.collect()
        assert tag == i and n == alone[i]["num_people"] and np.array_equal(joints, alone[i]["joints"][:n]), i
    # another valid 16-scale geometry: scales 0.95 .. 0.125
    start, gap = 0.95, 0.055
    e.set_scales(start, gap)
    f = _engine(start_scale=start, scale_gap=gap, **kw)
    low = alone[0]["lowres"]
    ref = orc.imresize(low, W, H, start, gap)[0]
    assert np.array_equal(e.resize(low), ref) and np.array_equal(f.resize(low), ref)
    imgs = [r.synth_frame(160, 120, i, seed=9) for i in range(B + 1)]    # a full batch and a partial one
    want_x = r.preprocess_frame(imgs[0], dw, dh, W, H, N, start, gap)[0]
    assert np.array_equal(e.debug_preprocess(imgs[0])[0], want_x) and np.array_equal(f.debug_preprocess(imgs[0])[0], want_x)
    out = []
    for eng in (e, f):
        got = []
        for i, im in enumerate(imgs):
            eng.submit_frame(im, tag=i)
            while eng.in_flight() >= B:
                got.append(eng.collect())
        while eng.in_flight():
            got.append(eng.collect())
        out.append(got)
    assert [t for t, _, _ in out[0]] == list(range(B + 1))
    for (t, n, j), (t2, n2, j2) in zip(*out):
        assert t == t2 and n == n2 and np.array_equal(j, j2), t
    e.close()
    f.close()


# ------------------------------------------------------------------------------------------
# the CLI passes --num_scales straight through
# ------------------------------------------------------------------------------------------
def test_cli_with_6_scales_writes_the_library_json(tmp_path):
    import caffe_rtpose_amd as r
    out = tmp_path / "js"
    N, gap = 6, mc.gap(6)
    p = subprocess.run([BIN, "--video", "synthetic:320x240:4:7", "--model", "coco", "--net_resolution", "160x96", "--resolution", "320x240",
                        "--num_scales", str(N), "--scale_gap", str(gap), "--write_json", str(out), "--no_frame_drops", "--no_display", "--num_gpu", "1"],
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert sorted(os.listdir(out)) == [f"frame{i:06d}.json" for i in range(4)]
    e = _engine(net_w=160, net_h=96, num_scales=N, scale_gap=gap, disp_w=320, disp_h=240, frames_in_flight=1)
    for i in range(4):
        img = r.synth_frame(320, 240, i, seed=7)
        x, _, fs = r.preprocess_frame(img, 320, 240, 160, 96, N, 1.0, gap)
        d = e.forward_debug(x)
        want = r.format_json(d["joints"], d["num_people"], 18, fs)
        assert want == orc.write_json(d["joints"], d["num_people"], 18, fs)
        assert open(out / f"frame{i:06d}.json", "rb").read() == want, i
    e.close()

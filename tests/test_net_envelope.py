"""The smallest and the widest nets the plan accepts, on the GPU (matrices, inputs and oracle results: tests/_edgecases.py; what they reach:
tests/test_net_envelope_cpu.py).

At 16x16 the 1/8 maps are 2x2: the 7x7 layers read almost only halo, every bicubic neighbour is a clamped one, NMS has 14 interior columns.  From
width 1936 on the fused ImResize+Nms strip kernel runs strips of 4 rows, from 2416 on of 2 rows; several scales run 8-row strips from 1376 on.

(a) every launch of the CONV_EDGE plans ALONE against float64: the body and the bound of tests/test_conv_launches.py, unchanged.  At 16x16 the
    border rule (first and last 4 rows and columns in full) covers every pixel.
(b) full batches of the BATCH_EDGE plans blob by blob against the frame tapped alone, graph and eager: the body of tests/test_batch_launches.py.
(c) post-processing bit for bit over POST_EDGE and the two straddle inputs: the production path (no resized map in memory) and the taps
    resize / nms / connect against the oracle's ImResize -> Nms -> connect and against each other; the peak buffer starts stale-filled, so a slot
    the kernels must not write shows.  On 16x32 the oracle's connect fails its range check: RTP_ERANGE on both paths, and the engine stays usable.
(d) whole frames at both ends, graph and eager: the device preprocessing against rtp_preprocess_frame, submit_frame / collect against
    forward_debug and the oracle's post-processing of the engine's own low-res maps.
(e) the outputs that read net-resolution geometry, at 16x16 and 2736x16: the maps export on the net grid (f32 and u8; wide stores through the
    tap and a dense device view, byte-wise stores through an odd device window) and the heat-map views of the renderer.

The [convcheck] lines of (a) and (b) and the times of every case: profiles/net_envelope_check.txt."""
import numpy as np
import pytest

import _convcheck as cc
import _edgecases as ec
import _mapscases as mc
import _oracle as orc
import _postcases as pc

pytestmark = pytest.mark.gpu

LOWRES_BLOB = "concat_stage7"
_graphs = {}


def _graph(model):
    if model not in _graphs:
        _graphs[model] = cc.builtin_graph(model)
    return _graphs[model]


def _engine(**kw):
    import caffe_rtpose_amd as r
    return r.Engine(r.Config(**kw))


def _same(a, b):
    """equal values; a NaN only has to be a NaN"""
    return np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------
# (a) every launch alone against float64
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.CONV_EDGE))
def test_every_launch_of_an_edge_plan_alone_against_float64(name):
    import test_conv_launches as tcl
    mode, model, W, H, N, gap, B, wseed = ec.CONV_EDGE[name]
    tcl._check_every_launch(name, cc.matrix_config(name, ec.CONV_EDGE), _graph(model), mode, N, B, 3)   # asserts nchecked > 0 and len(reps) == launches


# ------------------------------------------------------------------------------------------
# (b) full batches, blob by blob
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exec_mode", ["graph", "eager"])
@pytest.mark.parametrize("name", list(ec.BATCH_EDGE))
def test_edge_batch_blobs_equal_single_frame_blobs(name, exec_mode):
    import test_batch_launches as tbl
    tbl._batch_blobs_equal_single_frame_blobs(name, exec_mode, ec.BATCH_EDGE)


# ------------------------------------------------------------------------------------------
# (c) post-processing, bit for bit
# ------------------------------------------------------------------------------------------
def _post_engine(case):
    model, W, H, N, start, gap, kind = case
    return _engine(model=model, net_w=W, net_h=H, num_scales=N, start_scale=start, scale_gap=gap, disp_w=ec.DISPLAY[0], disp_h=ec.DISPLAY[1], frames_in_flight=1)


@pytest.mark.parametrize("case", [c for c in ec.POST_EDGE if c != ec.POST_ERANGE] + ec.STRADDLE_EDGE, ids=ec.post_id)
def test_edge_postproc_from_lowres_bit_exact(case):
    import caffe_rtpose_amd as r
    model, W, H, N, start, gap, kind = case
    e = _post_engine(case)
    try:
        assert ec.summary_postproc(r.plan_summary(e.cfg))[0] == ec.strip_rows(W, N)
        assert e.max_peaks == ec.max_peaks(model)
        low = ec.post_input(case)
        ref_res, ref_peaks, rn, rj = ec.post_reference(case)
        stale = ec.stale_peaks(model)
        # the production path: ImResize + Nms fused, no resized map in memory
        peaks, joints, n = e.post_from_lowres(low, stale)
        assert _same(peaks[:, 0, 0], ref_peaks[:, 0, 0]), f"peak counts: {peaks[:, 0, 0]} for {ref_peaks[:, 0, 0]}"
        assert _same(peaks, ref_peaks), f"{int((~np.isclose(peaks, ref_peaks, rtol=0, atol=0, equal_nan=True)).sum())} peak values differ"
        assert n == rn and _same(joints[:n], rj)
        # the map-materialising taps: against the oracle, and against the production path
        res = e.resize(low)
        assert _same(res, ref_res), f"{int((res != ref_res).sum())} resized values differ"
        pk = e.nms(res, stale)
        assert _same(pk, ref_peaks) and _same(pk, peaks)
        n2, j2 = e.connect(res, pk)
        assert n2 == rn and _same(j2[:n2], rj) and _same(j2[:n2], joints[:n])
        # once more: nothing of the first run is left in the engine's buffers
        peaks3, joints3, n3 = e.post_from_lowres(low, stale)
        assert n3 == n and _same(peaks3, peaks) and _same(joints3, joints)
    finally:
        e.close()


def test_portrait_16x32_is_refused_with_erange_on_both_paths_and_the_engine_stays_usable():
    import caffe_rtpose_amd as r
    case = ec.POST_ERANGE
    model = case[0]
    low = ec.post_input(case)
    ref_res, ref_peaks, rn, _ = ec.post_reference(case)
    assert rn is None                                      # the oracle's connect fails its range check on this input
    stale = ec.stale_peaks(model)
    e = _post_engine(case)
    try:
        for _ in range(2):
            with pytest.raises(r.RtpError) as ei:
                e.post_from_lowres(low, stale)
            assert ei.value.code == r.RTP_ERANGE, ei.value
            res = e.resize(low)
            assert _same(res, ref_res)
            pk = e.nms(res, stale)
            assert _same(pk, ref_peaks)
            with pytest.raises(r.RtpError) as ei:
                e.connect(res, pk)
            assert ei.value.code == r.RTP_ERANGE, ei.value
            # still usable: maps without a maximum give no peaks (every slot behind the counts keeps what it held) and no people
            quiet = np.zeros_like(low)
            peaks, joints, n = e.post_from_lowres(quiet, stale)
            assert n == 0 and len(joints) == 0 and not peaks[:, 0, 0].any() and _same(peaks[:, 1:], stale[:, 1:])
            assert _same(peaks, orc.nms(orc.imresize(quiet, case[1], case[2], case[4], case[5])[0], pc._dims(model)[0], ec.max_peaks(model),
                                        orc.default_thresholds(model)["nms_threshold"], stale))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------
# (d) whole frames at both ends
# ------------------------------------------------------------------------------------------
FRAME_CASES = {   # name -> (model, W, H, disp_w, disp_h, num_scales, scale_gap, batch_frames)
    "16x16_3s_b2": (0, 16, 16, 128, 96, 3, 0.15, 2),
    "2416x32": (0, 2416, 32, 1280, 720, 1, 0.3, 1),
}


@pytest.mark.parametrize("exec_mode", ["graph", "eager"])
@pytest.mark.parametrize("name", list(FRAME_CASES))
def test_whole_frames_at_both_ends_of_the_envelope(name, exec_mode):
    import caffe_rtpose_amd as r
    model, W, H, dw, dh, N, gap, B = FRAME_CASES[name]
    e = _engine(model=model, net_w=W, net_h=H, disp_w=dw, disp_h=dh, num_scales=N, scale_gap=gap, frames_in_flight=max(2 * B, 3), batch_frames=B,
                exec_mode=r.EXEC_GRAPH if exec_mode == "graph" else r.EXEC_EAGER)
    try:
        thr = e.get_thresholds()
        imgs = [r.synth_frame(*wh, i, seed=17) for i, wh in enumerate([(dw, dh), (640, 480), (333, 517)])]   # at the display size, and through the warp
        imgs[2] = np.random.default_rng(5).integers(0, 256, imgs[2].shape, dtype=np.uint8)                    # noise: every rounding boundary
        want = []
        for img in imgs:
            x, disp, fs = r.preprocess_frame(img, dw, dh, W, H, N, 1.0, gap)
            gx, gdisp, gfs = e.debug_preprocess(img)
            assert gfs == fs and np.array_equal(gdisp, disp)
            assert np.array_equal(gx, x), f"{int((gx != x).sum())} of {x.size} net-input values differ from rtp_preprocess_frame"
            d = e.forward_debug(x)
            ref_res = orc.imresize(d["lowres"], W, H, 1.0, gap)[0]
            assert _same(d["resized"], ref_res)
            ref_peaks = orc.nms(ref_res, e.num_parts, e.max_peaks, thr["nms_threshold"], d["peaks"])
            assert _same(d["peaks"], ref_peaks)
            rn, rj = orc.connect(model, ref_res, ref_peaks, e.max_peaks, W, H, dw, dh, thr)
            assert rn == d["num_people"] and _same(rj[:rn], d["joints"][:rn])
            want.append((fs, rn, rj[:rn].copy()))
        for rounds in range(2):                                # a full batch and a partial one (B = 2), twice: the second round replays
            got_fs = [e.submit_frame(img, tag=200 + i) for i, img in enumerate(imgs)]
            e.flush()
            for i, (fs, rn, rj) in enumerate(want):
                tag, n, joints = e.collect()
                assert tag == 200 + i and got_fs[i] == fs
                assert n == rn and _same(joints, rj), f"frame {i}: submit_frame / collect differs from forward_debug + the oracle's post-processing"
            assert e.in_flight() == 0
    finally:
        e.close()


# ------------------------------------------------------------------------------------------
# (e) outputs that read net-resolution geometry
# ------------------------------------------------------------------------------------------
OUTPUT_NETS = [(16, 16), (2736, 16)]


@pytest.mark.parametrize("W,H", OUTPUT_NETS, ids=lambda v: str(v))
def test_maps_export_on_the_net_grid(W, H):
    import torch
    import test_maps_out as tmo
    e = _engine(net_w=W, net_h=H, disp_w=128, disp_h=96, frames_in_flight=1)
    tdt = {"f32": torch.float32, "u8": torch.uint8}
    same = {"f32": mc.same_f32, "u8": np.array_equal}
    try:
        C = e.heat_channels
        allc = list(range(C))
        low = mc.planted_lowres(1, C, e.low_h, e.low_w, e.num_parts)      # quantiser ties, both clamps, a NaN and an inf
        want = orc.imresize(low, W, H)[0]
        ref = {"f32": want, "u8": mc.u8_ref_planes(want, allc, e.num_parts)}
        assert np.isnan(want).any() and (ref["u8"] == 0).any() and (ref["u8"] == 255).any()
        x = np.random.default_rng(3).uniform(-0.5, 0.5, (1, 3, H, W)).astype(np.float32)
        for fmt in ("f32", "u8"):
            e.set_maps_output("net", fmt)
            shape, dt, nb = e.maps_info()
            assert shape == (1, C, H, W) and nb == ref[fmt].nbytes
            # the tap: a dense buffer, the wide stores
            got = e.maps_from_lowres(low)[0]
            assert same[fmt](got, ref[fmt]), f"{fmt} tap: {int((got != ref[fmt]).sum())} values differ from the oracle"
            if fmt == "f32":
                assert mc.same_f32(got, e.resize(low))
            # a frame in flight: the host peek, a dense device view (wide stores), an odd window (byte by byte), guards around the windows
            gv = tmo.GUARD if fmt == "u8" else 3.0
            odd_big, odd = tmo._guarded(torch, tdt, fmt, C, H, W, 3, 7)
            al_big, al = tmo._guarded(torch, tdt, fmt, C, H, W, 8, 24)
            view = lambda t: t.unflatten(0, (1, C))
            assert tmo._layout(e, view(odd)) == 0 and tmo._layout(e, view(al)) == 1
            torch.cuda.synchronize()
            e.submit(x, tag=9)
            tag, host = e.peek_maps()
            assert e.peek_maps_device(view(odd), stream=0) == tag == 9
            assert e.peek_maps_device(view(al), stream=0) == 9
            assert e.collect()[0] == 9
            blob, tags = e.get_batch_blob(0, LOWRES_BLOB)
            assert tags == [9]
            want_frame = orc.imresize(blob, W, H)[0]
            ref_frame = want_frame if fmt == "f32" else mc.u8_ref_planes(want_frame, allc, e.num_parts)
            assert same[fmt](host[0], ref_frame), f"{fmt} peek: {int((host[0] != ref_frame).sum())} values differ from ImResize of the frame's low-res maps"
            assert same[fmt](odd.cpu().numpy(), ref_frame), f"{fmt}: the odd window (byte-wise stores) differs"
            assert same[fmt](al.cpu().numpy(), ref_frame), f"{fmt}: the aligned window (wide stores) differs"
            assert tmo._guards_intact(torch, odd_big, gv, C, H, W, 3), f"{fmt}: a byte outside the odd window was written"
            assert tmo._guards_intact(torch, al_big, gv, C, H, W, 8), f"{fmt}: a byte outside the aligned window was written"
    finally:
        e.close()


@pytest.mark.parametrize("W,H", OUTPUT_NETS, ids=lambda v: str(v))
def test_heat_map_views_of_the_renderer(W, H):
    import caffe_rtpose_amd as r
    dw, dh = (128, 96) if W == 16 else (640, 360)
    e = _engine(net_w=W, net_h=H, disp_w=dw, disp_h=dh, frames_in_flight=1)
    try:
        case = (0, W, H, 1, 1.0, 0.3, "noise")
        res = orc.imresize(ec.post_input(case), W, H)[0]
        assert np.array_equal(e.resize(ec.post_input(case)), res)
        img = r.synth_frame(dw, dh, 2, seed=13)
        for part in (3, 19):                                   # one part's heat map; all parts (no libm in either: identical)
            got = e.render(img, np.zeros((0, 3), np.float32), 0, part_to_show=part, resized=res)
            want = orc.render_view(0, img, res, part)
            assert np.array_equal(got, want), f"part_to_show {part}: {int((got != want).any(-1).sum())} pixels differ"
            assert (got != img).any()
    finally:
        e.close()

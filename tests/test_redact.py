"""Redaction mode on the GPU.  Every comparison is integer for integer and byte for byte against rtp_redact_regions and
rtp_redact_apply (which tests/test_redact_cpu.py holds to the numpy restatement): the parity tap on every case of
tests/_redactcases.py for COCO and MPI, an image whose size is a multiple of no tile with regions on tile borders, cut mosaic cells,
blur halos across tiles and the image corner and 96 regions through one tile, the async path in graph and eager mode with every
export, the order against overlay mode, smoothing mode's held parts, the mode switched off again, every refusal, and rtpose.bin
--redact on the GPU against --host_redact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _redactcases as rc
import _redactref as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
NET_W, NET_H = 160, 96
EFFECTS = [dict(effect=rr.MOSAIC), dict(effect=rr.BLUR, radius=3), dict(effect=rr.FILL, colour=0x20C0FF)]


def _engine(min_subset_cnt=2, **kw):
    import caffe_rtpose_amd as r
    kw = dict(dict(net_w=NET_W, net_h=NET_H, disp_w=160, disp_h=96, frames_in_flight=4, batch_frames=2, render=1), **kw)
    e = r.Engine(r.Config(**kw))
    t = e.get_thresholds()
    e.set_thresholds(t["nms_threshold"], t["inter_threshold"], t["inter_min_above"], min_subset_cnt, 0.05)   # keep more "people" of the noise maps
    return e


def _where(a, b):
    return np.argwhere((a != b).any(axis=2))[:5].tolist()


@pytest.mark.parametrize("model", ["coco", "mpi"])
def test_parity_tap_equals_the_host_definitions_on_every_case(model):
    import caffe_rtpose_amd as r
    P = 18 if model == "coco" else 15
    e = _engine(frames_in_flight=1, batch_frames=1, model=r.MODEL_COCO_18 if model == "coco" else r.MODEL_MPI_15)
    bg = rc.background()
    try:
        assert e.num_parts == P
        for case in rc.cases(P):
            for shape in (rr.ELLIPSE, rr.RECT):
                for eff in EFFECTS:
                    cfg = r.redact_config(**dict(case["cfg"], shape=shape, **eff))
                    e.set_redaction(cfg)
                    want = r.redact_regions(case["joints"], P, case["num_people"], cfg)
                    want_img = r.redact_apply(want, bg.copy(), cfg)
                    got, img = e.redact_from_joints(case["joints"], case["num_people"], image=bg)
                    assert np.array_equal(got, want), f"{case['name']}: records\n{got}\nthe host definition's\n{want}"
                    assert np.array_equal(img, want_img), f"{case['name']} shape {shape} {eff}: the image differs at {_where(img, want_img)}"
                    only, none = e.redact_from_joints(case["joints"], case["num_people"])
                    assert none is None and np.array_equal(only, want)
            rc.check_predicates(case, got)
    finally:
        e.close()


def _exact(P, cx, cy, a):
    """a person whose region under EXACT (below) is cx, cy, rx = ry = a: two scored parts at (cx - a, cy) and (cx + a, cy)"""
    j = np.zeros((P, 3), np.float32)
    j[0], j[1] = (cx - a, cy, 1.0), (cx + a, cy, 1.0)
    return j


EXACT = dict(parts=[0, 1], min_radius=0, pad=0, scale_q8=256, aspect_q8=256)   # s = 2 a + 1, rx = s >> 1 = a, ry = a


def test_tile_borders_cut_cells_halos_and_a_crowded_tile():
    """168 x 100 is a multiple of no tile (32 x 32 pixels).  Regions that end exactly on tile borders and one pixel to either side,
    one-pixel regions in the last column and row, a region over the bottom-right corner (mosaic cells cut by both image edges, for
    every cell; at blur radius 16 its halo spans three tiles and the corner), two overlapping blur regions that meet on the tile border
    x = 64 (what an in-place blur gets wrong), 96 regions through one tile, and images smaller than the display size."""
    import caffe_rtpose_amd as r
    P, W, H = 18, 168, 100
    e = _engine(frames_in_flight=1, batch_frames=1, disp_w=W, disp_h=H)
    sets = {
        "borders": [(47, 47, 16), (112, 48, 16), (47, 80, 15), (16, 16, 15), (80, 16, 16), (95, 63, 0), (96, 64, 0), (63, 31, 1), (128, 80, 31)],
        "one_pixel": [(167, 99, 0), (167, 40, 0), (80, 99, 0), (0, 0, 0), (167, 0, 0), (0, 99, 0)],
        "corner": [(156, 90, 14)],
        "meeting_on_a_border": [(56, 40, 8), (70, 40, 8), (60, 50, 9)],
        "crowd": [(66 + 2 * (k % 12), 34 + 3 * (k // 12), 3 + k % 5) for k in range(96)],
    }
    effects = [dict(effect=rr.MOSAIC, cell=c) for c in (2, 4, 8, 16, 32)] + [dict(effect=rr.BLUR, radius=q) for q in (1, 5, 16)] + [dict(effect=rr.FILL, colour=0x0000FF)]
    try:
        for w, h in ((W, H), (95, 70), (33, 17), (1, 1)):
            bg = rc.background(w, h, seed=h)
            for name, regs in sets.items():
                joints = np.stack([_exact(P, *g) for g in regs])
                for shape in (rr.RECT, rr.ELLIPSE):
                    for eff in effects:
                        cfg = r.redact_config(shape=shape, **EXACT, **eff)
                        e.set_redaction(cfg)
                        want = r.redact_regions(joints, P, cfg=cfg)
                        assert [tuple(x[:4]) for x in want.tolist()] == [(cx, cy, a, a) for cx, cy, a in regs], name
                        want_img = r.redact_apply(want, bg.copy(), cfg)
                        got, img = e.redact_from_joints(joints, image=bg)
                        assert np.array_equal(got, want), f"{name} {w}x{h}: records"
                        assert np.array_equal(img, want_img), f"{name} {w}x{h} shape {shape} {eff}: the image differs at {_where(img, want_img)}"
                        if (w, h) == (W, H):
                            assert not np.array_equal(img, bg) or eff["effect"] != rr.FILL
                            if name == "one_pixel" and eff["effect"] == rr.FILL:
                                assert (img[99, 167] == (255, 0, 0)).all() and (img[40, 167] == (255, 0, 0)).all() and (img[99, 80] == (255, 0, 0)).all()
                            if name == "meeting_on_a_border" and eff["effect"] == rr.BLUR:
                                chained = bg.copy()
                                for g in want:
                                    r.redact_apply(g[None], chained, cfg)
                                assert not np.array_equal(chained, want_img), "so that an in-place blur cannot pass"
    finally:
        e.close()


def _frames(order="AABAABBA", seed=41):
    import caffe_rtpose_amd as r
    content = {"A": r.synth_frame(160, 96, 0, seed=seed), "B": r.synth_frame(640, 360, 1, seed=seed)}   # B goes through the warp
    return [content[c] for c in order]


def _stream(e, frames, depth, redact=True, collect=None, tag0=30, extra=None):
    """submit as many frames as fit before each collect; per frame peek_redactions (twice), extra() and collect -> [dict(regs, extra, col)]"""
    out, nxt = [], 0
    while nxt < len(frames) or e.in_flight():
        while nxt < len(frames) and e.in_flight() < depth:
            e.submit_frame(frames[nxt], tag=tag0 + nxt)
            nxt += 1
        d = {}
        if redact:
            t1, d["regs"] = e.peek_redactions()
            t2, again = e.peek_redactions()
            assert t1 == t2 == tag0 + len(out) and np.array_equal(d["regs"], again), "peeking twice gives the same"
        d["extra"] = extra() if extra else None
        d["col"] = (collect or e.collect_rendered)()
        assert d["col"][0] == tag0 + len(out)
        out.append(d)
    return out


ALL = dict(parts=list(range(18)), min_parts=1)   # the noise maps' "people" have few parts: every part spans the region


@pytest.mark.parametrize("mode", ["graph", "eager"])
@pytest.mark.parametrize("pipe", [(4, 2), (1, 1)], ids=lambda p: "inflight%d_batch%d" % p)
def test_async_path_redacts_every_frame(mode, pipe):
    import caffe_rtpose_amd as r
    depth, batch = pipe
    e = _engine(frames_in_flight=depth, batch_frames=batch, exec_mode=r.EXEC_GRAPH if mode == "graph" else r.EXEC_EAGER)
    frames = _frames()
    try:
        plain = _stream(e, frames, depth, redact=False)
        valid = changed = 0
        for eff in [dict(effect=rr.MOSAIC, cell=4), dict(effect=rr.BLUR, radius=5), dict(effect=rr.FILL, colour=0x00FF00)]:
            cfg = r.redact_config(scale_q8=128, **ALL, **eff)
            e.set_redaction(cfg)
            res = _stream(e, frames, depth)
            for i, (d, p) in enumerate(zip(res, plain)):
                n, joints = p["col"][1], p["col"][2]
                assert d["col"][1] == n and np.array_equal(d["col"][2].view(np.uint32), joints.view(np.uint32)), "the joints do not depend on the mode"
                want = r.redact_regions(joints[:n], 18, cfg=cfg)
                assert np.array_equal(d["regs"], want), f"{mode} {pipe} {eff} frame {i}: records\n{d['regs']}\nthe host definition's\n{want}"
                want_img = r.redact_apply(want, p["col"][3].copy(), cfg)
                assert np.array_equal(d["col"][3], want_img), f"{mode} {pipe} {eff} frame {i}: the rendered frame differs at {_where(d['col'][3], want_img)}"
                valid += int(want[:, 5].sum()) if len(want) else 0
                changed += int((want_img != p["col"][3]).any(axis=2).sum())
        assert valid >= 1 and changed >= 1, "so that the test cannot pass vacuously: a frame had a valid region and a changed pixel"
    finally:
        e.close()


def test_export_modes_carry_the_redaction():
    import torch
    import caffe_rtpose_amd as r
    e = _engine()
    frames = _frames("ABAB", seed=43)
    cfg = r.redact_config(scale_q8=128, effect=rr.BLUR, radius=4, **ALL)
    try:
        plain = _stream(e, frames, 4, redact=False)
        want = []
        for p in plain:
            n, joints = p["col"][1], p["col"][2]
            regs = r.redact_regions(joints[:n], 18, cfg=cfg)
            want.append((regs, r.redact_apply(regs, p["col"][3].copy(), cfg), p["col"][3]))
        assert any(not np.array_equal(w[1], w[2]) for w in want), "the frames need redacted pixels"
        out = torch.zeros((96, 160, 3), dtype=torch.uint8, device="cuda")

        def collect_device():
            t, n, j = e.collect_rendered_device(out)
            torch.cuda.synchronize()
            return t, n, j, out.cpu().numpy().copy()

        def collect_yuv():
            t, j, y, u, v = e.collect_rendered_yuv()
            return t, len(j), j, (y.copy(), u.copy(), v.copy())
        e.set_redaction(cfg)
        for form, collect in (("device", collect_device), ("yuv", collect_yuv), ("jpeg", e.collect_rendered_jpeg)):
            if form == "yuv":
                e.set_render_yuv(420)
            if form == "jpeg":
                e.set_render_yuv(0)
                e.set_render_jpeg(90)
            res = _stream(e, frames, 4, collect=collect)
            for i, (d, (regs, img, _)) in enumerate(zip(res, want)):
                assert np.array_equal(d["regs"], regs), f"{form} frame {i}: records"
                got = d["col"][3]
                if form == "device":
                    assert np.array_equal(got, img), f"{form} frame {i}"
                elif form == "yuv":
                    assert all(np.array_equal(a, b) for a, b in zip(got, r.convert_bgr_to_yuv(img, 420))), f"{form} frame {i}"
                else:
                    assert got == r.encode_jpeg(img, 90), f"{form} frame {i}"
        e.set_render_jpeg(0)
    finally:
        e.close()


def test_overlay_is_drawn_on_top_of_the_redaction():
    """tracking, overlay and redaction mode on: the image is the host redaction followed by rtp_overlay_draw — boxes, ids and trails stay
    sharp — and not the opposite order, on frames where a label lies inside a region"""
    import caffe_rtpose_amd as r
    e = _engine()
    frames = _frames("AABA", seed=41)
    tcfg, ocfg = r.track_config(min_parts=2), r.overlay_config(label_scale=1, alpha=256)
    cfg = r.redact_config(effect=rr.MOSAIC, cell=8, shape=rr.RECT, scale_q8=512, pad=12, **ALL)
    try:
        e.set_tracking(tcfg)
        e.set_track_overlay(ocfg)
        e.set_redaction(cfg)
        res = _stream(e, frames, 4, extra=lambda: e.peek_overlay_items()[1])
        inside = differs = 0
        for i, (d, f) in enumerate(zip(res, frames)):
            n, joints, img = d["col"][1], d["col"][2], d["col"][3]
            regs, items = d["regs"], d["extra"]
            assert np.array_equal(regs, r.redact_regions(joints[:n], 18, cfg=cfg))
            plain = e.render(e.debug_preprocess(f)[1], joints[:n], n)
            want = r.overlay_draw(items, r.redact_apply(regs, plain.copy(), cfg))
            assert np.array_equal(img, want), f"frame {i}: differs at {_where(img, want)}"
            other = r.redact_apply(regs, r.overlay_draw(items, plain.copy()), cfg)
            for it in items:
                if it[0] == r.engine.OVERLAY_KIND_LABEL and any(g[5] and abs(it[1] - g[0]) <= g[2] and abs(it[3] - g[0]) <= g[2] and abs(it[2] - g[1]) <= g[3] and
                                                                abs(it[4] - g[1]) <= g[3] and it[1] >= 0 and it[2] >= 0 and it[3] < 160 and it[4] < 96 for g in regs):
                    inside += 1
                    differs += not np.array_equal(other, want)
        assert inside >= 1 and differs == inside, (inside, differs)
        e.set_redaction(None)
        e.set_track_overlay(None)
        e.set_tracking(None)
    finally:
        e.close()


def test_smoothing_holds_a_region_while_its_part_drops_out():
    """with RTP_SMOOTH_RENDER the regions come from joints_s: a person whose only listed part is missing in one frame, and held by
    the filter, still has a region there; without smoothing that person has none"""
    import caffe_rtpose_amd as r
    e = _engine()
    frames = _frames("AAAAAAAA", seed=41) + _frames("ABABABAB", seed=47)
    tcfg, scfg = r.track_config(min_parts=2), r.smooth_config(apply=r.SMOOTH_RENDER, max_hold=5)
    try:
        e.set_tracking(tcfg)
        e.set_smoothing(scfg)
        e.set_redaction(r.redact_config(**ALL))
        first = _stream(e, frames, 4, extra=lambda: e.peek_smoothed()[1])
        found = None
        for i, d in enumerate(first):
            n, raw, js = d["col"][1], d["col"][2], d["extra"]
            assert np.array_equal(d["regs"], r.redact_regions(js[:n], 18, cfg=r.redact_config(**ALL))), f"frame {i}: the regions come from joints_s"
            held = np.argwhere(~(raw[:n, :, 2] > 0) & (js[:n, :, 2] > 0))
            if found is None and len(held):
                found = (i, int(held[0][0]), int(held[0][1]))
        assert found is not None, "the frames need a part that drops out and is held"
        i, k, p = found
        cfg = r.redact_config(parts=[p], min_parts=1)
        for smooth in (True, False):
            e.set_redaction(None)
            e.set_smoothing(None)
            e.set_tracking(None)
            e.set_tracking(tcfg)
            if smooth:
                e.set_smoothing(scfg)
            e.set_redaction(cfg)
            res = _stream(e, frames, 4, extra=(lambda: e.peek_smoothed()[1]) if smooth else None)
            d = res[i]
            n, raw = d["col"][1], d["col"][2]
            assert np.array_equal(raw[:n].view(np.uint32), first[i]["col"][2][:n].view(np.uint32))
            poses = d["extra"] if smooth else raw
            assert np.array_equal(d["regs"], r.redact_regions(poses[:n], 18, cfg=cfg))
            assert int(d["regs"][k, 5]) == (1 if smooth else 0), f"smoothing {smooth}: person {k} of frame {i}, part {p}: {d['regs'][k]}"
    finally:
        e.close()


def test_mode_off_again_changes_nothing():
    import caffe_rtpose_amd as r
    frames = _frames("ABBA", seed=43)

    def run(e):
        e.set_tracking()
        e.set_crops_output(64, 64, 16, margin=0.15)
        res = _stream(e, frames, 4, redact=False, extra=lambda: (e.peek_tracks()[1], e.peek_crops()[1:]))
        e.set_crops_output(None)
        e.set_tracking(None)
        return res
    never = _engine()
    try:
        want = run(never)
    finally:
        never.close()
    e = _engine()
    try:
        for eff in EFFECTS:
            e.set_redaction(r.redact_config(**ALL, **eff))
            on = _stream(e, frames, 4)
        e.set_redaction(None)
        e.set_redaction(None)        # off twice is fine
        got = run(e)
        assert any(not np.array_equal(a["col"][3], b["col"][3]) for a, b in zip(on, want)), "the mode changed pixels while it was on"
        for a, b in zip(want, got):
            assert a["col"][1] == b["col"][1] and np.array_equal(a["col"][2].view(np.uint32), b["col"][2].view(np.uint32)) and np.array_equal(a["col"][3], b["col"][3])
            assert np.array_equal(a["extra"][0], b["extra"][0]) and all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a["extra"][1], b["extra"][1]))
    finally:
        e.close()


def test_refusals_and_lifecycle():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    one = rc.people(rc.head(18, 40, 30))
    plain = _engine(render=0)
    try:
        with pytest.raises(r.RtpError) as ex:
            plain.set_redaction()
        assert ex.value.code == r.RTP_EINVAL and "render" in str(ex.value)
        plain.set_redaction(None)
    finally:
        plain.close()
    e = _engine()
    frames = _frames("AB", seed=45)
    try:
        for call in (e.peek_redactions, e.redaction_info, lambda: e.redact_from_joints(one)):
            with pytest.raises(r.RtpError) as ex:
                call()
            assert ex.value.code == r.RTP_EINVAL and "off" in str(ex.value)
        for kw in (dict(effect=3), dict(shape=2), dict(min_score=-1.0), dict(min_score=float("nan")), dict(min_parts=0), dict(scale_q8=63), dict(scale_q8=4097), dict(aspect_q8=63),
                   dict(aspect_q8=1025), dict(pad=-1), dict(pad=257), dict(min_radius=-1), dict(min_radius=257), dict(cell=3), dict(cell=64), dict(radius=0), dict(radius=17),
                   dict(parts=[0, 0]), dict(parts=[18]), dict(parts=[-1])):
            with pytest.raises(r.RtpError) as ex:
                e.set_redaction(r.redact_config(**kw))
            assert ex.value.code == r.RTP_EINVAL, kw
        bad = r.redact_config()
        bad.struct_size += 4
        with pytest.raises(r.RtpError):
            e.set_redaction(bad)
        with pytest.raises(r.RtpError):     # every refused switch left the mode off
            e.redaction_info()
        cfg = r.redact_config(effect=rr.BLUR, radius=2, colour=0x010203, **ALL)
        e.set_redaction(cfg)                # (it does not need tracking mode)
        info = e.redaction_info()
        assert info["parts"] == list(range(18)) and info["effect"] == rr.BLUR and info["radius"] == 2 and info["colour"] == 0x010203 and info["cell"] == 8
        e.set_redaction(r.redact_config())
        assert e.redaction_info()["parts"] == rr.HEAD_PARTS[18]
        with pytest.raises(r.RtpError) as ex:
            e.set_redaction(r.redact_config(cell=5))
        assert ex.value.code == r.RTP_EINVAL and e.redaction_info()["cell"] == 8, "a refused change keeps the configuration"
        e.set_redaction(cfg)
        with pytest.raises(r.RtpError) as ex:
            e.peek_redactions()
        assert ex.value.code == r.RTP_EAGAIN   # nothing in flight
        big = np.zeros((97, 161, 3), np.uint8)
        for img in (big[:, :160], big[:96]):
            with pytest.raises(r.RtpError) as ex:
                e.redact_from_joints(one, image=img)
            assert ex.value.code == r.RTP_EINVAL and "display" in str(ex.value)
        buf = np.full((2, 6), 77, np.int32)
        m = C.c_int(-1)
        two = np.concatenate([one, one])
        assert _lib.lib.rtp_redact_from_joints(e.h, two.ctypes.data_as(_lib.fp), 2, None, 0, 0, buf.ctypes.data_as(_lib.ip), C.byref(m), 1) == r.RTP_ERANGE
        assert m.value == 2 and (buf == 77).all()
        # a frame submitted as a net input has records, and nothing is redacted (there is no image); rtp_render carries no redaction
        x, disp, _ = e.debug_preprocess(frames[0])
        e.submit(x, tag=5)
        _, regs = e.peek_redactions()
        _, n, joints = e.collect()
        assert np.array_equal(regs, r.redact_regions(joints[:n], 18, cfg=cfg))
        drawn = e.render(disp, joints[:n], n)
        # with a frame in flight: no switch, no tap
        e.submit_frame(frames[0], tag=1)
        for call in (lambda: e.set_redaction(None), lambda: e.set_redaction(r.redact_config()), lambda: e.redact_from_joints(one)):
            with pytest.raises(r.RtpError) as ex:
                call()
            assert ex.value.code == r.RTP_EAGAIN
        # capacity below the count: RTP_ERANGE with *num_regions set, and the frame stays peekable
        tag, regs = e.peek_redactions()
        n = len(regs)
        assert tag == 1 and n >= 1, "the frame needs a person"
        buf = np.full((n, 6), 77, np.int32)
        got_n, t = C.c_int(-1), C.c_uint64()
        assert _lib.lib.rtp_peek_redactions(e.h, C.byref(t), buf.ctypes.data_as(_lib.ip), C.byref(got_n), n - 1) == r.RTP_ERANGE
        assert got_n.value == n and (buf == 77).all()
        assert _lib.lib.rtp_peek_redactions(e.h, C.byref(t), None, C.byref(got_n), n) == r.RTP_EINVAL
        assert _lib.lib.rtp_peek_redactions(e.h, C.byref(t), buf.ctypes.data_as(_lib.ip), C.byref(got_n), n) == r.RTP_OK and np.array_equal(buf, regs)
        _, n1, j1, img = e.collect_rendered()
        assert n1 == n and np.array_equal(regs, r.redact_regions(j1[:n1], 18, cfg=cfg))
        assert np.array_equal(img, r.redact_apply(regs, drawn.copy(), cfg)) and not np.array_equal(img, drawn)
        e.set_redaction(None)
        with pytest.raises(r.RtpError):
            e.redaction_info()
    finally:
        e.close()


def test_cli_redact_on_the_gpu_equals_host_redact(tmp_path):
    """rtpose.bin --redact --write_frames with one worker: redacted on the GPU (the engine's mode, then the GPU's JPEG encoder) and,
    with --host_redact, by the re-orderer on the raw rendered frame (rtp_redact_regions + rtp_redact_apply, then the host encoder): the
    same bytes, and not those of a run without --redact"""
    files = {}
    for mode in ("gpu", "host", "off"):
        out = tmp_path / mode
        out.mkdir()
        extra = [] if mode == "off" else ["--redact", "--redact_effect", "blur", "--redact_radius", "5", "--redact_parts", "all", "--redact_scale", "0.5", "--redact_aspect", "1.5",
                                          "--redact_pad", "3"] + (["--host_redact"] if mode == "host" else [])
        p = subprocess.run([BIN, "--video", "synthetic:160x96:12", "--model", "coco", "--net_resolution", "160x96", "--resolution", "160x96", "--write_frames", str(out) + "/",
                            "--no_frame_drops", "--no_display", "--num_gpu", "1"] + extra, capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        if mode != "off":
            assert (b"redaction on the GPU" in p.stderr) == (mode == "gpu"), p.stderr.decode()[-3000:]
        files[mode] = {f: open(out / f, "rb").read() for f in sorted(os.listdir(out))}
    assert len(files["gpu"]) == 12 and files["gpu"] == files["host"]
    assert sorted(files["off"]) == sorted(files["gpu"]) and files["off"] != files["gpu"]

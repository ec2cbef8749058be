"""Redaction mode without a GPU: rtp_redact_regions and rtp_redact_apply against the numpy restatement of the header's text
(tests/_redactref.py) on every case of tests/_redactcases.py, every effect, shape, cell and the blur's radii, at image sizes from 1 x 1
up and with strided rows; the properties the definition promises (no dependence on the regions' order or overlap, NOT the result of
applying them one after the other, untouched bytes outside, fill idempotent); and every refusal.  Every comparison is integer for
integer and byte for byte."""
import ctypes as C

import numpy as np
import pytest

import _redactcases as rc
import _redactref as rr

ubp = C.POINTER(C.c_ubyte)
SIZES = [(1, 1), (33, 17), (95, 70), (168, 100)]
EFFECTS = [dict(effect=rr.MOSAIC, cell=c) for c in (2, 4, 8, 16, 32)] + [dict(effect=rr.BLUR, radius=1), dict(effect=rr.BLUR, radius=16), dict(effect=rr.FILL, colour=0x1234C8)]


def _cfg(**kw):
    import caffe_rtpose_amd as r
    return r.redact_config(**kw)


@pytest.mark.parametrize("P", [18, 15])
def test_the_restatement_reaches_every_case(P):
    """a guard on the case predicates themselves (it runs no code of the library)"""
    for case in rc.cases(P):
        rc.check_predicates(case, rc.run_ref(case))


def test_defaults():
    import caffe_rtpose_amd as r
    cfg = r.redact_config()
    got = {k: getattr(cfg, k) for k in rr.DEFAULTS if k != "parts"}
    assert got == {k: v for k, v in rr.DEFAULTS.items() if k != "parts"} and not cfg.parts and cfg.struct_size == C.sizeof(cfg)
    assert (r.REDACT_MOSAIC, r.REDACT_BLUR, r.REDACT_FILL, r.REDACT_ELLIPSE, r.REDACT_RECT, r.REDACT_REGION_INTS, r.REDACT_MAX_RADIUS) == (0, 1, 2, 0, 1, 6, 4096)
    assert [r.crops_head_parts(m) for m in (r.MODEL_COCO_18, r.MODEL_MPI_15)] == [rr.HEAD_PARTS[18], rr.HEAD_PARTS[15]]


@pytest.mark.parametrize("P", [18, 15])
def test_regions_and_pixels_equal_the_restatement_on_every_case(P):
    import caffe_rtpose_amd as r
    bg = rc.background()
    for case in rc.cases(P):
        want = rc.run_ref(case)
        got = r.redact_regions(case["joints"], P, case["num_people"], _cfg(**case["cfg"]))
        assert [tuple(int(v) for v in x) for x in got] == want, f"{case['name']}: records\n{got}\nthe restatement's\n{want}"
        rc.check_predicates(case, got)
        for shape in (rr.ELLIPSE, rr.RECT):
            for eff in (dict(effect=rr.MOSAIC), dict(effect=rr.BLUR, radius=3), dict(effect=rr.FILL, colour=0xFF8000)):
                kw = dict(case["cfg"], shape=shape, **eff)
                img = r.redact_apply(got, bg.copy(), _cfg(**kw))
                assert np.array_equal(img, rr.apply(want, rr.config(**kw), bg)), f"{case['name']} {kw}: the image"
    # an explicit part list equals the default one
    j = rc.people(rc.head(P, 40, 30), P=P)
    assert np.array_equal(r.redact_regions(j, P, cfg=_cfg(parts=rr.HEAD_PARTS[P])), r.redact_regions(j, P))
    everything = r.redact_regions(j, P, cfg=_cfg(parts=list(range(P))))
    assert everything[0, 4] == len(rr.HEAD_PARTS[P]) + 1 and everything[0, 2] > 100, "with every part listed the far shoulder counts"


def _regions_for(w, h):
    """regions inside, across every edge and corner, one pixel, zero radii, and one larger than the image"""
    regs = [(w // 2, h // 2, 9, 7, 1, 1), (0, 0, 5, 6, 1, 1), (w - 1, h - 1, 6, 4, 1, 1), (w - 1, 0, 0, 0, 1, 1), (0, h - 1, 3, 0, 1, 1), (w // 3, h - 1, 0, 5, 1, 1),
            (w + 40, h // 2, 8, 8, 1, 1), (w // 4, h // 4, 11, 13, 1, 0), (w // 2 + 6, h // 2 + 3, 10, 10, 2, 1)]
    return regs


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_every_effect_shape_cell_and_radius_at_every_size(w, h):
    import caffe_rtpose_amd as r
    bg = rc.background(w, h, seed=w)
    regs = _regions_for(w, h)
    for shape in (rr.ELLIPSE, rr.RECT):
        for eff in EFFECTS:
            kw = dict(shape=shape, **eff)
            want = rr.apply(regs, rr.config(**kw), bg)
            got = r.redact_apply(rr.as_array(regs), bg.copy(), _cfg(**kw))
            assert np.array_equal(got, want), f"{w}x{h} {kw}: differs at {np.argwhere((got != want).any(axis=2))[:5].tolist()}"
            cov = rr.coverage(regs, rr.config(**kw), w, h)
            assert cov.any() and np.array_equal(got[~cov], bg[~cov]), "bytes outside every region are unchanged"
            # rows of stride 3 * w + 7: the same pixels, the padding untouched
            wide = np.full((h, 3 * w + 7), 0xA5, np.uint8)
            view = wide[:, :3 * w].reshape(h, w, 3)
            view[:] = bg
            r.redact_apply(rr.as_array(regs), view, _cfg(**kw))
            assert np.array_equal(view, want) and (wide[:, 3 * w:] == 0xA5).all(), f"{w}x{h} {kw}: strided rows"
    whole = [(0, 0, rr.MAX_RADIUS, rr.MAX_RADIUS, 1, 1)]
    for eff in EFFECTS:
        assert np.array_equal(r.redact_apply(rr.as_array(whole), bg.copy(), _cfg(**eff)), rr.values(bg, rr.config(**eff))), "a region as large as the clamp covers the image"


def test_order_and_overlap_do_not_matter_but_one_after_the_other_does():
    import caffe_rtpose_amd as r
    bg = rc.background()
    regs = [(60, 40, 14, 17, 1, 1), (72, 46, 14, 17, 1, 1), (66, 30, 10, 12, 1, 1), (140, 80, 6, 6, 1, 1)]
    rng = np.random.default_rng(1)
    for eff in EFFECTS:
        cfg = _cfg(**eff)
        all_at_once = r.redact_apply(rr.as_array(regs), bg.copy(), cfg)
        for _ in range(4):
            perm = [regs[i] for i in rng.permutation(len(regs))]
            assert np.array_equal(r.redact_apply(rr.as_array(perm), bg.copy(), cfg), all_at_once), f"{eff}: a permutation of the regions"
        # the union of the single regions' coverage, each pixel's value taken from the untouched image
        union = bg.copy()
        for g in regs:
            alone = r.redact_apply(rr.as_array([g]), bg.copy(), cfg)
            cov = rr.coverage([g], rr.config(**eff), rc.W, rc.H)
            union[cov] = alone[cov]
        assert np.array_equal(union, all_at_once), f"{eff}: the union of the regions' coverage"
        chained = bg.copy()
        for g in regs:
            r.redact_apply(rr.as_array([g]), chained, cfg)
        if eff["effect"] == rr.BLUR:
            assert not np.array_equal(chained, all_at_once), "a blur applied region after region reads blurred pixels: an in-place shortcut must not pass"
        if eff["effect"] == rr.FILL:
            assert np.array_equal(chained, all_at_once) and np.array_equal(r.redact_apply(rr.as_array(regs), all_at_once.copy(), cfg), all_at_once), "fill twice equals once"


def test_refusals_leave_the_outputs_untouched():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    lib = _lib.lib
    j = rc.people(rc.head(18, 40, 30))
    fp_, ip_ = _lib.fp, _lib.ip
    bad_cfgs = [dict(effect=3), dict(effect=-1), dict(shape=2), dict(min_score=-1.0), dict(min_score=float("nan")), dict(min_score=float("inf")), dict(min_parts=0),
                dict(scale_q8=63), dict(scale_q8=4097), dict(aspect_q8=63), dict(aspect_q8=1025), dict(pad=-1), dict(pad=257), dict(min_radius=-1), dict(min_radius=257),
                dict(cell=0), dict(cell=3), dict(cell=64), dict(radius=0), dict(radius=17), dict(parts=[0, 0]), dict(parts=[18]), dict(parts=[-1]), dict(parts=[])]
    regs = np.full((2, 6), 77, np.int32)
    img = rc.background(40, 30)
    keep = img.copy()
    one = rr.as_array([(20, 15, 5, 5, 1, 1)])

    def regions(cfg, joints=j, people=1, P=18, out=regs):
        return lib.rtp_redact_regions(joints.ctypes.data_as(fp_) if joints is not None else None, people, P, C.byref(cfg) if cfg is not None else None,
                                      out.ctypes.data_as(ip_) if out is not None else None)

    def apply(cfg, rg=one, n=1, image=img, w=40, h=30, stride=120):
        return lib.rtp_redact_apply(rg.ctypes.data_as(ip_) if rg is not None else None, n, C.byref(cfg) if cfg is not None else None,
                                    image.ctypes.data_as(ubp) if image is not None else None, w, h, stride)
    for kw in bad_cfgs:
        cfg = _cfg(**kw)
        assert regions(cfg) == r.RTP_EINVAL, kw
        if "parts" not in kw or kw["parts"] != [18]:   # (rtp_redact_apply knows no model: a list is checked against RTP_MAX_NUM_PARTS)
            assert apply(cfg) == r.RTP_EINVAL, kw
    wrong = _cfg()
    wrong.struct_size -= 4
    ok = _cfg()
    assert regions(wrong) == r.RTP_EINVAL and apply(wrong) == r.RTP_EINVAL
    assert regions(None) == r.RTP_EINVAL and regions(ok, out=None) == r.RTP_EINVAL and regions(ok, joints=None) == r.RTP_EINVAL
    assert regions(ok, P=0) == r.RTP_EINVAL and regions(ok, P=71) == r.RTP_EINVAL
    assert regions(ok, joints=np.zeros((1, 17, 3), np.float32), P=17) == r.RTP_EINVAL, "NULL parts needs a model with head parts"
    assert regions(ok, joints=None, people=0) == 0 and regions(ok, joints=None, people=-5) == 0
    assert apply(None) == r.RTP_EINVAL and apply(ok, image=None) == r.RTP_EINVAL and apply(ok, rg=None) == r.RTP_EINVAL
    for kw in (dict(n=-1), dict(n=97), dict(w=0), dict(h=0), dict(w=32769), dict(h=32769), dict(stride=119)):
        assert apply(ok, **kw) == r.RTP_EINVAL, kw
    assert (regs == 77).all() and np.array_equal(img, keep), "every refusal leaves records and image untouched"
    assert apply(ok, rg=None, n=0) == r.RTP_OK and np.array_equal(img, keep)
    assert apply(ok) == r.RTP_OK and not np.array_equal(img, keep)


def test_python_wrappers_refuse():
    import caffe_rtpose_amd as r
    with pytest.raises(r.RtpError) as ex:
        r.redact_regions(np.zeros((1, 18, 3), np.float32), 18, cfg=r.redact_config(cell=5))
    assert ex.value.code == r.RTP_EINVAL
    with pytest.raises(r.RtpError):
        r.redact_apply(np.zeros((1, 6), np.int32), np.zeros((4, 4, 3), np.uint8), r.redact_config(radius=0))
    with pytest.raises(ValueError):
        r.redact_apply(np.zeros((1, 6), np.int32), np.zeros((4, 4, 3), np.float32))

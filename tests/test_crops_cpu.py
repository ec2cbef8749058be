"""Crops mode on the host: rtp_crop_people against the numpy restatement of the header's text (tests/_cropref.py), byte for byte and
float bit for float bit on every case of tests/_cropcases.py; the predicates that prove each case reaches what it is meant to; n and
the untouched tail; every refusal.  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import _cropcases as cc
import _cropref as cr

GUARD = 0xA5


def _lib():
    from caffe_rtpose_amd import _lib
    return _lib


def _both(img, joints, cw, ch, max_crops, layout, **kw):
    """(library, restatement) on the same arguments; asserts they are equal"""
    import caffe_rtpose_amd as r
    got_b, got_c = r.crop_people(img, joints, cc.NUM_PARTS, cw, ch, max_crops, layout=layout, **kw)
    ref_b, ref_c = cr.crop_people(img, joints, cc.NUM_PARTS, cw, ch, max_crops, layout=layout, **kw)
    assert cc.same_boxes(got_b, ref_b), f"boxes differ in slots {np.flatnonzero((got_b.view(np.uint32) != ref_b.view(np.uint32)).any(1)).tolist()}"
    bad = np.flatnonzero((got_c != ref_c).reshape(len(ref_c), -1).any(1)).tolist() if len(ref_c) else []
    assert not bad, f"crops differ in slots {bad}"
    return got_b, got_c


@pytest.mark.parametrize("crop", cc.CROPS, ids=lambda c: "%dx%d" % c)
@pytest.mark.parametrize("disp", cc.DISPLAYS, ids=lambda d: "%dx%d" % d)
def test_host_definition_equals_the_restatement_and_the_cases_reach_their_targets(disp, crop):
    (W, H), (cw, ch) = disp, crop
    img = cc.display(W, H)
    z = cc.zoo(W, H, cw, ch)
    joints = cc.joints_of(z)
    boxes, crops = _both(img, joints, cw, ch, len(z), cr.HWC_BGR)
    kinds = cc.check_predicates(z, boxes, crops, W, H, cw, ch)
    assert set(kinds) == set(cc.PREDICATES)
    _, planar = _both(img, joints, cw, ch, len(z), cr.CHW_RGB)
    assert np.array_equal(planar, crops[..., ::-1].transpose(0, 3, 1, 2)), "CHW_RGB is the HWC_BGR crop with planes R, G, B"


@pytest.mark.parametrize("case", range(len(cc.variations())))
def test_margins_part_lists_and_thresholds(case):
    (W, H), (cw, ch), kw = cc.variations()[case]
    img = cc.display(W, H)
    z = cc.zoo(W, H, cw, ch)
    joints = cc.joints_of(z)
    base, _ = _both(img, joints, cw, ch, len(z), cr.HWC_BGR)
    for layout in cc.LAYOUTS:
        boxes, _ = _both(img, joints, cw, ch, len(z), layout, **kw)
    kind = [k for k, _ in z]
    inside = kind.index("inside")
    if kw.get("margin") and "parts" not in kw and "min_score" not in kw:
        m = kw["margin"]
        assert boxes[inside][2] > base[inside][2] * (1 + 1.9 * m), "the margin moves both sides out"
    if kw.get("parts") == cc.HEAD:
        assert boxes[inside][5] == 1 and boxes[inside][4] == 2 and boxes[inside][2] < base[inside][2] / 4, "the head list gives the small head box"
        assert boxes[kind.index("one_part")][5] == 0, "no head part was found: no box"
    if kw.get("parts") == [1]:
        assert boxes[inside][4] == 1 and min(boxes[inside][2:4]) == 1, "one listed part: the 1-pixel minimum"
    if kw.get("parts") == cc.PART_LISTS["repeats"]:
        assert boxes[inside][4] == 5, "a repeated entry counts once per repeat"
    if kw.get("min_parts") == 4:
        assert boxes[inside][5] == 1 and boxes[kind.index("tiny")].tolist() == [0, 0, 0, 0, 3, 0], "3 counting parts of 4: no box, the count stays"
    if kw.get("min_score") == 0.9:
        assert not boxes[:, 5].any() and not boxes[:, 4].any(), "a score AT the threshold does not count"


@pytest.mark.parametrize("people,max_crops", [(0, 4), (1, 4), (7, 7), (10, 7), (96, 96)])
def test_people_against_max_crops_and_the_untouched_tail(people, max_crops):
    import caffe_rtpose_amd as r
    L = _lib()
    W, H, cw, ch = 160, 96, 8, 8
    img = cc.display(W, H)
    joints = cc.joints_of(cc.zoo(W, H, cw, ch), people)
    n = min(people, max_crops)
    ref_b, ref_c = cr.crop_people(img, joints, cc.NUM_PARTS, cw, ch, max_crops, margin=0.15)
    assert len(ref_b) == n
    cfg = L.rtp_crops_config()
    cfg.struct_size = C.sizeof(cfg)
    cfg.crop_w, cfg.crop_h, cfg.max_crops, cfg.min_parts, cfg.margin = cw, ch, max_crops, 1, 0.15
    boxes = np.full((max_crops + 2, r.CROP_BOX_FLOATS), 7.5, np.float32)
    crops = np.full((max_crops + 2, ch, cw, 3), GUARD, np.uint8)
    jj = joints if people else np.zeros((1, cc.NUM_PARTS, 3), np.float32)
    rc = L.lib.rtp_crop_people(img.ctypes.data_as(C.POINTER(C.c_ubyte)), W, H, jj.ctypes.data_as(L.fp), people, cc.NUM_PARTS, C.byref(cfg),
                               boxes.ctypes.data_as(L.fp), crops.ctypes.data_as(C.POINTER(C.c_ubyte)))
    assert rc == n
    assert cc.same_boxes(boxes[:n], ref_b) and np.array_equal(crops[:n], ref_c)
    assert (boxes[n:] == 7.5).all() and (crops[n:] == GUARD).all(), "bytes behind the n written slots were touched"
    if people == 96:
        assert boxes[:n, 5].sum() >= 60 and len({c.tobytes() for c in crops[:n]}) > 40, "the 96 people are not copies of a few"
    # boxes alone: no image, no crops
    only = np.full((max_crops + 2, r.CROP_BOX_FLOATS), 7.5, np.float32)
    rc = L.lib.rtp_crop_people(None, W, H, jj.ctypes.data_as(L.fp), people, cc.NUM_PARTS, C.byref(cfg), only.ctypes.data_as(L.fp), None)
    assert rc == n and cc.same_boxes(only, boxes)


def test_every_refusal():
    import caffe_rtpose_amd as r
    L = _lib()
    W, H = 32, 16
    img = cc.display(W, H)
    joints = cc.joints_of(cc.zoo(W, H, 8, 8), 3)
    boxes = np.zeros((4, r.CROP_BOX_FLOATS), np.float32)
    crops = np.zeros((4, 8, 8, 3), np.uint8)
    keep = []

    def call(img_p=True, w=W, h=H, joints_p=True, people=3, num_parts=cc.NUM_PARTS, cfg_p=True, boxes_p=True, crops_p=True, **fields):
        cfg = L.rtp_crops_config()
        cfg.struct_size = C.sizeof(cfg)
        cfg.crop_w, cfg.crop_h, cfg.max_crops, cfg.min_parts = 8, 8, 4, 1
        for k, v in fields.items():
            if k == "parts":
                arr = (C.c_int * len(v))(*v)
                keep.append(arr)
                cfg.parts, cfg.num_parts = arr, len(v)
            else:
                setattr(cfg, k, v)
        return L.lib.rtp_crop_people(img.ctypes.data_as(C.POINTER(C.c_ubyte)) if img_p else None, w, h, joints.ctypes.data_as(L.fp) if joints_p else None, people,
                                     num_parts, C.byref(cfg) if cfg_p else None, boxes.ctypes.data_as(L.fp) if boxes_p else None,
                                     crops.ctypes.data_as(C.POINTER(C.c_ubyte)) if crops_p else None)

    assert call() == 3
    assert call(parts=[0, 17, 17]) == 3
    assert call(people=0, joints_p=False) == 0
    for bad in (dict(cfg_p=False), dict(boxes_p=False), dict(struct_size=8), dict(w=0), dict(h=0), dict(w=32769), dict(people=-1), dict(num_parts=0), dict(num_parts=71),
                dict(crop_w=7), dict(crop_w=513), dict(crop_h=7), dict(crop_h=513), dict(max_crops=0), dict(max_crops=97), dict(min_score=-0.5),
                dict(min_score=float("nan")), dict(min_score=float("inf")), dict(min_parts=0), dict(margin=-0.1), dict(margin=float("nan")), dict(margin=16.5),
                dict(layout=2), dict(layout=-1), dict(joints_p=False), dict(img_p=False)):
        assert call(**bad) == r.RTP_EINVAL, bad
    # the part list: its count and its entries
    cfgs = []
    for n_list, entries in ((0, [0]), (71, [0] * 71), (2, [0, 18]), (1, [-1])):
        cfg = L.rtp_crops_config()
        cfg.struct_size = C.sizeof(cfg)
        cfg.crop_w, cfg.crop_h, cfg.max_crops, cfg.min_parts = 8, 8, 4, 1
        arr = (C.c_int * len(entries))(*entries)
        cfg.parts, cfg.num_parts = arr, n_list
        cfgs.append((cfg, arr))
        rc = L.lib.rtp_crop_people(img.ctypes.data_as(C.POINTER(C.c_ubyte)), W, H, joints.ctypes.data_as(L.fp), 3, cc.NUM_PARTS, C.byref(cfg),
                                   boxes.ctypes.data_as(L.fp), crops.ctypes.data_as(C.POINTER(C.c_ubyte)))
        assert rc == r.RTP_EINVAL, (n_list, entries)
    with pytest.raises(ValueError):
        r.crop_people(img, joints, cc.NUM_PARTS, 8, 8, layout="rgb")
    with pytest.raises(r.RtpError):
        r.crop_people(img, joints, cc.NUM_PARTS, 8, 600)


def test_identity_box_is_a_copy_and_a_doubling_box_is_the_2x2_mean():
    """two closed forms of the definition that need no restatement"""
    import caffe_rtpose_amd as r
    W, H = 40, 24
    img = cc.display(W, H)
    p = cc.person({1: (8.0, 4.0), 8: (24.0, 20.0)})           # a 16 x 16 box at an integer position
    _, crop = r.crop_people(img, p[None], cc.NUM_PARTS, 16, 16)
    assert np.array_equal(crop[0], img[4:20, 8:24]), "a box as large as the crop at an integer position is a plain copy"
    _, half = r.crop_people(img, p[None], cc.NUM_PARTS, 8, 8)
    blk = img[4:20, 8:24].astype(np.int64).reshape(8, 2, 8, 2, 3).sum((1, 3))
    assert np.array_equal(half[0], ((blk + 2) // 4).astype(np.uint8)), "a step of 2 pixels: the mean of the 2 x 2 block, half up"

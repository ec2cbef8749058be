"""Overlay mode without a GPU: rtp_overlay_update and rtp_overlay_draw against the numpy restatement of the header's text
(tests/_overlayref.py) on every case of tests/_overlaycases.py, predicates that do not go through the restatement (a label's pixels
decode back to the id through the glyph table, a box changes exactly its outline's pixels, an empty list changes nothing), and every
refusal.  Every comparison is integer for integer and byte for byte."""
import ctypes as C

import numpy as np
import pytest

import _overlaycases as oc
import _overlayref as orf

ubp = C.POINTER(C.c_ubyte)


@pytest.mark.parametrize("P", [18, 15])
def test_the_restatement_reaches_every_case(P):
    """a guard on the case predicates themselves (it runs no code of the library): every sequence reaches what it is there to reach"""
    for case in oc.cases(P):
        oc.check_predicates(case, *oc.run_ref(case))


@pytest.mark.parametrize("P", [18, 15])
def test_update_and_draw_equal_the_restatement_on_every_case(P):
    import caffe_rtpose_amd as r
    bg = oc.background()
    for case in oc.cases(P):
        tcfg, ocfg = r.track_config(**case["tcfg"]), r.overlay_config(**case["ocfg"])
        ts, st = r.TrackState(P), r.TrailState(P)
        ts.next_id = case["next_id"]
        want_items, want_states, want_recs = oc.run_ref(case)
        items, states, recs = [], [], []
        for i, (joints, num_people) in enumerate(case["frames"]):
            rc = r.track_update(ts, joints, num_people, tcfg)
            got = r.overlay_update(st, joints, num_people, rc, ocfg)
            assert oc.as_tuples(got) == want_items[i], f"{case['name']} frame {i}: items\n{oc.as_tuples(got)}\nthe restatement's\n{want_items[i]}"
            diff = orf.same_state(want_states[i], st)
            assert diff is None, f"{case['name']} frame {i}: {diff}"
            items.append(oc.as_tuples(got))
            states.append(oc.as_ref(st))
            recs.append(np.asarray(rc, np.int64))
            if i in (len(case["frames"]) - 1, 4) and len(got) <= 40:   # (the restatement draws slowly: the last frame, and one in the middle)
                img = r.overlay_draw(got, bg.copy())
                assert np.array_equal(img, orf.draw(want_items[i], bg)), f"{case['name']} frame {i}: the image"
                assert len(got) == 0 or not np.array_equal(img, bg) or case["ocfg"].get("alpha") == 0
        oc.check_predicates(case, items, states, recs)


@pytest.mark.parametrize("name,items", oc.draw_lists(), ids=[n for n, _ in oc.draw_lists()])
def test_draw_equals_the_restatement(name, items):
    import caffe_rtpose_amd as r
    bg = oc.background()
    got = r.overlay_draw(orf.as_array(items), bg.copy())
    assert np.array_equal(got, orf.draw(items, bg)), name
    if name in ("alpha_0", "wholly_outside"):
        assert np.array_equal(got, bg)
    else:
        assert not np.array_equal(got, bg)


def test_a_stride_larger_than_the_row_and_odd_sizes():
    import caffe_rtpose_amd as r
    for w, h, pad in ((160, 96, 52), (37, 23, 1), (1, 1, 0), (168, 100, 7)):
        bg = oc.background(w, h)
        for name, items in oc.draw_lists(w, h):
            wide = np.full((h, w * 3 + pad), 0xA5, np.uint8)
            view = np.lib.stride_tricks.as_strided(wide, (h, w, 3), (wide.strides[0], 3, 1))
            view[:] = bg
            r.overlay_draw(orf.as_array(items), view)
            assert (wide[:, w * 3:] == 0xA5).all(), f"{name} {w}x{h}: the padding behind a row was written"
            assert np.array_equal(view, r.overlay_draw(orf.as_array(items), bg.copy())), f"{name} {w}x{h}: a strided image differs from a dense one"
        if (w, h) == (37, 23):
            for name, items in oc.draw_lists(w, h):
                assert np.array_equal(r.overlay_draw(orf.as_array(items), bg.copy()), orf.draw(items, bg)), f"{name} {w}x{h}"


def test_the_order_of_overlapping_items_matters():
    import caffe_rtpose_amd as r
    bg = oc.background()
    ab, ba = (r.overlay_draw(orf.as_array(oc.overlapping(o)), bg.copy()) for o in (0, 1))
    assert np.array_equal(ab, orf.draw(oc.overlapping(0), bg)) and np.array_equal(ba, orf.draw(oc.overlapping(1), bg))
    differ = (ab != ba).any(axis=2)
    both = (orf.coverage(oc.overlapping(0)[0], oc.W, oc.H) > 0) & (orf.coverage(oc.overlapping(0)[1], oc.W, oc.H) > 0)
    assert differ.any() and not (differ & ~both).any(), "the two orders differ, and only where both items cover a pixel"


@pytest.mark.parametrize("ident", [1, 9, 10, 407, 2147483647, -2147483648, -1, 1234567890])
@pytest.mark.parametrize("scale", [1, 3])
def test_a_label_decodes_back_to_its_id(ident, scale):
    """independent of the restatement: the pixels of a label at alpha 256, sampled once per font pixel, are matched against the glyph
    table of the package, digit by digit"""
    import caffe_rtpose_amd as r
    text = str(ident & 0xFFFFFFFF)
    colour = r.OVERLAY_PALETTE[ident & 15]
    lw, lh = (6 * len(text) + 1) * scale, 9 * scale
    img = np.full((lh + 4, lw + 6, 3), 99, np.uint8)
    r.overlay_draw(np.array([[3, 2, 1, 2 + lw - 1, 1 + lh - 1, scale, colour, 256, ident]], np.int32), img)
    cell = img[1:1 + lh, 2:2 + lw]
    bgr = np.array([colour & 255, (colour >> 8) & 255, (colour >> 16) & 255], np.uint8)
    is_bg = (cell == bgr).all(axis=2)
    is_text = (cell == 0).all(axis=2) | (cell == 255).all(axis=2)
    assert (is_bg | is_text).all() and (img[0] == 99).all() and (img[1 + lh:] == 99).all() and (img[:, :2] == 99).all() and (img[:, 2 + lw:] == 99).all()
    for v in range(lh):   # every pixel of one font pixel is the same
        for u in range(lw):
            assert is_text[v, u] == is_text[v - v % scale, u - u % scale]
    grid = is_text[::scale, ::scale] & ~is_bg[::scale, ::scale]
    assert not grid[0].any() and not grid[8].any() and not grid[:, 0].any()
    decoded = ""
    for i in range(len(text)):
        rows = tuple(int("".join("1" if b else "0" for b in grid[1 + y, 1 + 6 * i:1 + 6 * i + 5]), 2) for y in range(7))
        assert not grid[:, 6 + 6 * i].any(), "the column between two digits is empty"
        assert rows in r.OVERLAY_FONT, f"digit {i}: rows {rows} are no glyph"
        decoded += str(r.OVERLAY_FONT.index(rows))
    assert decoded == text
    assert len(set(r.OVERLAY_FONT)) == 10


@pytest.mark.parametrize("box,width", [((10, 12, 50, 40), 1), ((10, 12, 50, 40), 3), ((10, 12, 17, 40), 4), ((10, 12, 50, 40), 16), ((-5, -5, 20, 20), 2), ((30, 30, 30, 30), 1)])
def test_a_box_changes_exactly_its_outline(box, width):
    import caffe_rtpose_amd as r
    x0, y0, x1, y1 = box
    w, h = 64, 48
    img = np.zeros((h, w, 3), np.uint8)
    r.overlay_draw(np.array([[2, x0, y0, x1, y1, width, 0xFFFFFF, 256, 0]], np.int32), img)
    changed = int((img != 0).any(axis=2).sum())

    def area(ax0, ay0, ax1, ay1):   # of the part inside the image
        return max(min(ax1, w - 1) - max(ax0, 0) + 1, 0) * max(min(ay1, h - 1) - max(ay0, 0) + 1, 0)
    inner = area(x0 + width, y0 + width, x1 - width, y1 - width) if x1 - x0 + 1 > 2 * width and y1 - y0 + 1 > 2 * width else 0
    assert changed == area(x0, y0, x1, y1) - inner and changed > 0


def test_an_empty_list_changes_no_byte():
    import caffe_rtpose_amd as r
    bg = oc.background()
    assert np.array_equal(r.overlay_draw(np.zeros((0, 9), np.int32), bg.copy()), bg)
    assert np.array_equal(r.overlay_draw(np.full((5, 9), 7, np.int32), bg.copy(), num_items=0), bg)


def test_defaults_and_refusals():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    lib = _lib.lib
    cfg = r.overlay_config()
    assert {n: getattr(cfg, n) for n in orf.DEFAULTS} == orf.DEFAULTS and cfg.struct_size == C.sizeof(cfg)
    assert r.OVERLAY_MAX_ITEMS == 96 * 33 and tuple(r.OVERLAY_PALETTE) == tuple(orf.PALETTE) and [list(g) for g in r.OVERLAY_FONT] == orf.FONT
    st = r.TrailState(18)
    assert st.num_parts == 18 and st.frames == 0 and not st.slot["owner"].any() and st == r.TrailState(18) and st != r.TrailState(15)
    for P in (0, 71):
        with pytest.raises(r.RtpError):
            r.TrailState(P)
    person = oc.body(18, 20, 30)[None]
    rec = np.array([[5, 3, 1, 0]], np.int32)
    items = np.zeros((r.OVERLAY_MAX_ITEMS, 9), np.int32)
    m = C.c_int(-1)

    def update(state=st, cfg=cfg, joints=person, n=1, recs=rec, items=items, m=m, cap=r.OVERLAY_MAX_ITEMS):
        return lib.rtp_overlay_update(C.byref(state.c) if state else None, C.byref(cfg) if cfg else None, joints.ctypes.data_as(_lib.fp) if joints is not None else None, n,
                                      recs.ctypes.data_as(_lib.ip) if recs is not None else None, items.ctypes.data_as(_lib.ip) if items is not None else None,
                                      C.byref(m) if m is not None else None, cap)
    before = st.copy()
    for kw in (dict(what=0), dict(what=8), dict(min_score=-1.0), dict(min_score=float("nan")), dict(min_score=float("inf")), dict(box_margin=-1), dict(box_margin=1025),
               dict(line_width=0), dict(line_width=17), dict(label_scale=0), dict(label_scale=9), dict(trail_len=-1), dict(trail_len=33), dict(trail_radius=-1),
               dict(trail_radius=17), dict(alpha=-1), dict(alpha=257)):
        assert update(cfg=r.overlay_config(**kw)) == r.RTP_EINVAL, kw
    bad = r.overlay_config()
    bad.struct_size += 4
    assert update(cfg=bad) == r.RTP_EINVAL
    assert update(state=None) == update(cfg=None) == update(items=None) == update(m=None) == update(cap=-1) == update(joints=None) == update(recs=None) == r.RTP_EINVAL
    for slot in (-1, 128):
        assert update(recs=np.array([[5, slot, 1, 0]], np.int32)) == r.RTP_EINVAL
    two = np.concatenate([person, person])
    assert update(joints=two, n=2, recs=np.array([[5, 3, 1, 0], [6, 3, 1, 0]], np.int32)) == r.RTP_EINVAL      # one slot named twice
    for field, v in (("count", -1), ("count", 33), ("head", -1), ("head", 32)):
        broken = st.copy()
        broken.slot[field][77] = v
        assert update(state=broken) == r.RTP_EINVAL
    wrong = st.copy()
    wrong.c.struct_size = 12
    assert update(state=wrong) == r.RTP_EINVAL
    assert st == before, "a refused call leaves the state untouched"
    # capacity: RTP_ERANGE with the count and the state untouched; an untracked person with a slot of -1 is fine; nobody is fine
    assert update(cap=1) == r.RTP_ERANGE and m.value == 2 and st == before
    assert update(cap=2) == r.RTP_OK and m.value == 2 and st.frames == 1 and st.slot["owner"][3] == 5
    assert update(recs=np.array([[0, -1, 0, 0]], np.int32)) == r.RTP_OK and m.value == 0 and st.frames == 2
    assert update(joints=None, n=0, recs=None, cap=0) == r.RTP_OK and m.value == 0 and st.frames == 3
    st.frames = 0xFFFFFFFF
    assert update() == r.RTP_OK and st.frames == 1, "0 is skipped at the wrap"
    # the draw
    img = np.zeros((8, 8, 3), np.uint8)
    it = np.array([[2, 0, 0, 3, 3, 1, 0xFFFFFF, 256, 0]], np.int32)

    def draw(items=it, n=1, image=img, w=8, h=8, stride=24):
        return lib.rtp_overlay_draw(items.ctypes.data_as(_lib.ip) if items is not None else None, n, image.ctypes.data_as(ubp) if image is not None else None, w, h, stride)
    assert draw(image=None) == draw(items=None) == draw(n=-1) == draw(w=0) == draw(h=0) == draw(stride=23) == r.RTP_EINVAL and not img.any()
    assert draw(items=None, n=0) == r.RTP_OK and not img.any()
    assert draw() == r.RTP_OK and img.any()

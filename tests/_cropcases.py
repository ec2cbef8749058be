"""The cases of crops mode, shared by tests/test_crops_cpu.py and tests/test_crops.py, and one predicate per kind of person that proves
the case reaches what it is meant to reach.  Nothing here imports the library.

A case is a display image, a configuration and a `zoo` of people built for that display and crop size: each person is of one `kind`
(inside, crossing an edge, wholly outside, magnified, box-filtered twice or four times, one part, NaN, overflow, ...), and
PREDICATES[kind] says what the person's box record, Q16 parameters and crop must show."""
import numpy as np

import _cropref as cr

NUM_PARTS = 18                      # COCO
HEAD = [0, 14, 15, 16, 17]          # nose, eyes, ears
DISPLAYS = [(160, 96), (97, 61)]
CROPS = [(8, 8), (20, 12), (25, 17), (64, 64), (128, 96), (16, 48)]   # 20x12: row bytes no multiple of 16; 25x17: odd everything; 16x48: portrait
MARGINS = [0.0, 0.15, 1.0]
LAYOUTS = [cr.HWC_BGR, cr.CHW_RGB]
PART_LISTS = {"all": None, "head": HEAD, "one": [1], "repeats": [1, 8, 1, 8, 8]}
NAN = float("nan")


def display(w, h, seed=3):
    """a u8 BGR image without any smoothness: every tap and weight matters"""
    return np.random.default_rng(seed + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def person(points):
    """points: {part: (x, y) or (x, y, score)}; every other part is the (0, 0, 0) of a part that was not found"""
    p = np.zeros((NUM_PARTS, 3), np.float32)
    for k, v in points.items():
        p[k] = (v[0], v[1], v[2] if len(v) > 2 else 0.9)
    return p


def _span(cx, cy, w, h, extra=None):
    """a person whose parts 1 and 8 (neck, hip) are two opposite corners of a w x h box about (cx, cy); the head parts 0 and 14
    sit inside it, close together, so that the `head` list gives a different, small box"""
    pts = {1: (cx - w / 2, cy - h / 2), 8: (cx + w / 2, cy + h / 2), 0: (cx - w / 8, cy - h / 4), 14: (cx - w / 8 + 0.75, cy - h / 4 + 0.5)}
    pts.update(extra or {})
    return person(pts)


def zoo(W, H, cw, ch):
    """[(kind, person)] for a display of W x H and crops of cw x ch; boxes keep the crop's aspect unless the kind is about the aspect"""
    a = cw / ch
    fit = min(W / a, H) * 0.45            # height of a box that lies inside the display with room to spare
    z = []
    z.append(("inside", _span(W * 0.5 + 0.37, H * 0.5 - 0.21, fit * a, fit)))
    z.append(("cross_left", _span(1.3, H * 0.5, fit * a, fit)))
    z.append(("cross_right", _span(W - 1.6, H * 0.5, fit * a, fit)))
    z.append(("cross_top", _span(W * 0.5, 0.9, fit * a, fit)))
    z.append(("cross_bottom", _span(W * 0.5, H - 1.2, fit * a, fit)))
    z.append(("outside", _span(3.0 * W, 2.5 * H, fit * a, fit)))
    z.append(("negative", _span(-fit * a, -fit, fit * a, fit)))
    tx, ty = float(int(W * 0.4)), float(int(H * 0.4))
    z.append(("tiny", person({1: (tx, ty), 8: (tx + 6, ty + 6), 0: (tx + 2, ty + 3)})))          # 6 pixels, magnified
    z.append(("wide_aspect", _span(W * 0.5, H * 0.5, 30.0, 2.0)))        # the height grows to the crop's aspect
    z.append(("tall_aspect", _span(W * 0.5, H * 0.5, 2.0, 30.0)))        # ... the width does
    z.append(("s2", _span(W * 0.5 + 0.5, H * 0.5, 2.0 * cw, 2.0 * ch)))     # a step of 2 pixels
    z.append(("s4", _span(W * 0.5, H * 0.5 + 0.25, 3.5 * cw, 3.5 * ch)))  # ... of 3.5
    big = max(3.5 * ch, 1.25 * max(W / a, H))
    z.append(("huge", _span(W * 0.5, H * 0.5, big * a, big)))            # larger than the display
    z.append(("one_part", person({11: (W * 0.3 + 0.4, H * 0.6 + 0.6)})))
    z.append(("nan_x", _span(W * 0.4, H * 0.5, fit * a, fit, {5: (NAN, H * 0.5, 0.9), 6: (W * 0.5, float("inf"), 0.9)})))
    z.append(("nan_score", _span(W * 0.6, H * 0.5, fit * a, fit, {5: (9.0 * W, 9.0 * H, NAN)})))
    z.append(("low_score", _span(W * 0.6, H * 0.4, fit * a, fit, {5: (9.0 * W, 9.0 * H, 0.0)})))
    z.append(("neg_zero", person({1: (-0.0, 5.0), 8: (0.0, 9.0), 3: (-0.0, 7.0)})))
    z.append(("overflow", person({1: (2.5e6, 50.0), 8: (10.0, 50.0)})))
    z.append(("overflow_inf", person({1: (3e38, 10.0), 8: (-3e38, 10.0)})))
    z.append(("nobody", person({})))                                       # no part was found at all
    return z


def joints_of(z, people=None):
    """the zoo as a joints array; people: repeat (and shift by a pixel per round) or cut to that many"""
    base = np.stack([p for _, p in z])
    if people is None:
        return base
    out = np.zeros((people, NUM_PARTS, 3), np.float32)
    for k in range(people):
        out[k] = base[k % len(base)]
        out[k, :, :2] += np.float32(k // len(base)) * (out[k, :, 2:3] > 0)
    return out


def _edges(rec):
    left, top, w, h = (float(v) for v in rec[:4])
    return left, top, left + w, top + h


def _q(rec, cw, ch):
    return cr.q16_of(tuple(rec[:4]), cw, ch)


# kind -> predicate(record, crop (HWC), W, H, cw, ch), for margin 0, min_score 0, min_parts 1 and the list of all parts
PREDICATES = {
    "inside": lambda r, c, W, H, cw, ch: r[5] == 1 and r[4] == 4 and _edges(r)[0] >= 0 and _edges(r)[1] >= 0 and _edges(r)[2] <= W and _edges(r)[3] <= H and c.any(),
    "cross_left": lambda r, c, W, H, cw, ch: r[5] == 1 and _edges(r)[0] < -1 and _edges(r)[2] > 1 and not c[:, 0].any() and c[:, -1].any(),
    "cross_right": lambda r, c, W, H, cw, ch: r[5] == 1 and _edges(r)[0] < W - 1 and _edges(r)[2] > W + 1 and c[:, 0].any() and not c[:, -1].any(),
    "cross_top": lambda r, c, W, H, cw, ch: r[5] == 1 and _edges(r)[1] < -1 and _edges(r)[3] > 1 and not c[0].any() and c[-1].any(),
    "cross_bottom": lambda r, c, W, H, cw, ch: r[5] == 1 and _edges(r)[1] < H - 1 and _edges(r)[3] > H + 1 and c[0].any() and not c[-1].any(),
    "outside": lambda r, c, W, H, cw, ch: r[5] == 1 and _edges(r)[0] > W + 1 and not c.any(),
    "negative": lambda r, c, W, H, cw, ch: r[5] == 1 and _edges(r)[2] < -1 and _edges(r)[3] < -1 and not c.any(),
    "tiny": lambda r, c, W, H, cw, ch: r[5] == 1 and r[4] == 3 and min(r[2], r[3]) == 6 and (cw < 64 or (_q(r, cw, ch)[2] < 65536 // 8 and c.any())),
    "wide_aspect": lambda r, c, W, H, cw, ch: r[5] == 1 and r[2] == 30 and r[3] > 2,
    "tall_aspect": lambda r, c, W, H, cw, ch: r[5] == 1 and r[3] == 30 and r[2] > 2,
    "s2": lambda r, c, W, H, cw, ch: r[5] == 1 and _q(r, cw, ch)[4:] == (2, 2) and c.any(),
    "s4": lambda r, c, W, H, cw, ch: r[5] == 1 and _q(r, cw, ch)[4:] == (4, 4) and c.any(),
    "huge": lambda r, c, W, H, cw, ch: r[5] == 1 and _q(r, cw, ch)[4:] == (4, 4) and r[2] > W and r[3] > H and c.any(),
    "one_part": lambda r, c, W, H, cw, ch: r[5] == 1 and r[4] == 1 and min(r[2], r[3]) == 1,
    "nan_x": lambda r, c, W, H, cw, ch: r[5] == 1 and r[4] == 4 and _edges(r)[2] <= W and _edges(r)[3] <= H,
    "nan_score": lambda r, c, W, H, cw, ch: r[5] == 1 and r[4] == 4 and _edges(r)[2] <= W and _edges(r)[3] <= H,
    "low_score": lambda r, c, W, H, cw, ch: r[5] == 1 and r[4] == 4 and _edges(r)[2] <= W and _edges(r)[3] <= H,
    "neg_zero": lambda r, c, W, H, cw, ch: r[5] == 1 and r[4] == 3 and np.signbit(r[0]) and (r[2] == 1 or r[3] == 4),
    "overflow": lambda r, c, W, H, cw, ch: r[5] == 0 and r[4] == 2 and not r[:4].any() and not c.any(),
    "overflow_inf": lambda r, c, W, H, cw, ch: r[5] == 0 and r[4] == 2 and not r[:4].any() and not c.any(),
    "nobody": lambda r, c, W, H, cw, ch: r[5] == 0 and r[4] == 0 and not c.any(),
}


def check_predicates(z, boxes, crops_hwc, W, H, cw, ch):
    """every person of the zoo shows what its kind promises (base configuration); -> the kinds seen"""
    for k, (kind, _) in enumerate(z):
        assert PREDICATES[kind](boxes[k], crops_hwc[k], W, H, cw, ch), f"{W}x{H} crop {cw}x{ch}: person {k} is not '{kind}': record {boxes[k].tolist()}"
    return [kind for kind, _ in z]


def same_boxes(a, b):
    """float bit for float bit"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def variations():
    """(display, crop, kwargs) beyond the base configuration: margins, part lists, min_parts, min_score, max_crops against the people"""
    v = []
    for m in MARGINS[1:]:
        v.append(((160, 96), (64, 64), dict(margin=m)))
        v.append(((97, 61), (25, 17), dict(margin=m)))
    for name in ("head", "one", "repeats"):
        v.append(((160, 96), (20, 12), dict(parts=PART_LISTS[name])))
        v.append(((97, 61), (16, 48), dict(parts=PART_LISTS[name], margin=0.15)))
    v.append(((160, 96), (64, 64), dict(min_parts=4)))
    v.append(((160, 96), (8, 8), dict(min_score=0.9)))          # score > min_score: a part AT the threshold does not count
    v.append(((97, 61), (128, 96), dict(min_score=0.5, min_parts=2, margin=0.15)))
    return v

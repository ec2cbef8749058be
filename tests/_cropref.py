"""Crops mode restated in numpy / Python integers from the text of include/rtpose_mi355x.h (section "crops mode"), independently of
the C code: the box in np.float32 scalars, one rounded operation per line; everything past the four Q16 conversions in Python ints."""
import math

import numpy as np

F = np.float32
BOX_FLOATS = 6
HWC_BGR, CHW_RGB = 0, 1
LIMIT = F(1048576.0)


def _rint_q16(v):
    """(int64) rintf(v * 65536.0f) for a float32 v: the product rounded to float32, then to the nearest integer, ties to even"""
    q = F(v) * F(65536.0)
    return int(np.rint(q))


def box_of(person, parts, min_score, min_parts, margin, crop_w, crop_h):
    """person [num_parts][3] float32 -> (record of 6 float32, (left, top, w, h) as float32 or None)"""
    xs, ys = [], []
    for p in parts:
        x, y, s = F(person[p][0]), F(person[p][1]), F(person[p][2])
        if not (s > F(min_score)):          # a NaN score never counts
            continue
        if not (math.isfinite(float(x)) and math.isfinite(float(y))):
            continue
        xs.append(x + F(0.0))
        ys.append(y + F(0.0))
    count = len(xs)
    none = np.array([0, 0, 0, 0, count, 0], np.float32)
    if count < min_parts:
        return none, None
    with np.errstate(over="ignore", invalid="ignore"):
        x0, x1, y0, y1 = min(xs), max(xs), min(ys), max(ys)
        sx = F(x0 + x1)
        sy = F(y0 + y1)
        cx = F(sx * F(0.5))
        cy = F(sy * F(0.5))
        w = F(x1 - x0)
        h = F(y1 - y0)
        if not (math.isfinite(float(w)) and math.isfinite(float(h))):
            return none, None
        m = w if w > h else h
        g = F(F(F(margin) * m) * F(2.0))
        w = F(w + g)
        h = F(h + g)
        w = w if w > F(1.0) else F(1.0)
        h = h if h > F(1.0) else F(1.0)
        wa = F(F(h * F(crop_w)) / F(crop_h))
        if wa > w:
            w = wa
        else:
            h = F(F(w * F(crop_h)) / F(crop_w))
        left = F(cx - F(w * F(0.5)))
        top = F(cy - F(h * F(0.5)))
        right = F(left + w)
        bottom = F(top + h)
        ok = all(abs(v) <= LIMIT for v in (left, top, right, bottom))   # a NaN or an infinity fails
    if not ok:
        return none, None
    return np.array([left, top, w, h, count, 1], np.float32), (left, top, w, h)


def samples_of(step_q16):
    return 1 if step_q16 <= 98304 else 2 if step_q16 <= 196608 else 4


def q16_of(box, crop_w, crop_h):
    """(ox, oy, dx, dy, Sx, Sy) of a box (left, top, w, h)"""
    left, top, w, h = box
    ox, oy = _rint_q16(left), _rint_q16(top)
    dx = _rint_q16(F(F(w) / F(crop_w)))
    dy = _rint_q16(F(F(h) / F(crop_h)))
    return ox, oy, dx, dy, samples_of(dx), samples_of(dy)


def crop_of(img, box, crop_w, crop_h, layout):
    """img [H][W][3] u8 -> the crop of one slot with a box, vectorised over the output pixels in int64 (exact: every intermediate is
    below 2^44)"""
    H, W = img.shape[:2]
    ox, oy, dx, dy, Sx, Sy = q16_of(box, crop_w, crop_h)
    src = np.zeros((H + 2, W + 2, 3), np.int64)       # the constant border: taps outside the image read 0
    src[1:-1, 1:-1] = img
    i = np.arange(crop_w, dtype=np.int64)
    j = np.arange(crop_h, dtype=np.int64)
    T = np.zeros((crop_h, crop_w, 3), np.int64)
    for b in range(Sy):
        py = oy + j * dy + ((2 * b + 1) * dy) // (2 * Sy) - 32768
        Y = py >> 16
        fy = (((py & 65535) + 16) >> 5)[:, None, None]
        for a in range(Sx):
            px = ox + i * dx + ((2 * a + 1) * dx) // (2 * Sx) - 32768
            X = px >> 16
            fx = (((px & 65535) + 16) >> 5)[None, :, None]

            def tap(yy, xx):
                return src[np.clip(yy + 1, 0, H + 1)[:, None], np.clip(xx + 1, 0, W + 1)[None, :]]
            T += (2048 - fy) * ((2048 - fx) * tap(Y, X) + fx * tap(Y, X + 1)) + fy * ((2048 - fx) * tap(Y + 1, X) + fx * tap(Y + 1, X + 1))
    out = ((T + Sx * Sy * 2097152) // (Sx * Sy * 4194304)).astype(np.uint8)
    return out if layout == HWC_BGR else np.ascontiguousarray(out[:, :, ::-1].transpose(2, 0, 1))


def crop_people(img, joints, num_parts, crop_w, crop_h, max_crops, parts=None, min_score=0.0, min_parts=1, margin=0.0, layout=HWC_BGR):
    """-> (boxes [n][6] float32, crops [n] + shape u8), n = min(people, max_crops)"""
    joints = np.asarray(joints, np.float32).reshape(-1, num_parts, 3)
    n = min(joints.shape[0], max_crops)
    parts = list(range(num_parts)) if parts is None else list(parts)
    shape = (crop_h, crop_w, 3) if layout == HWC_BGR else (3, crop_h, crop_w)
    boxes = np.zeros((n, BOX_FLOATS), np.float32)
    crops = np.zeros((n,) + shape, np.uint8)
    for k in range(n):
        boxes[k], box = box_of(joints[k], parts, min_score, min_parts, margin, crop_w, crop_h)
        if box is not None:
            crops[k] = crop_of(img, box, crop_w, crop_h, layout)
    return boxes, crops

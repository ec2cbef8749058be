"""A numpy restatement of redaction mode's regions and pixels, written from the text of include/rtpose_mi355x.h (THE REGIONS, THE
PIXELS) and not from the C code: tests/test_redact_cpu.py holds rtp_redact_regions and rtp_redact_apply to it, tests/test_redact.py
holds the kernels to those."""
import numpy as np

MAX_PEOPLE, MAX_RADIUS, REGION_INTS = 96, 4096, 6
MOSAIC, BLUR, FILL = 0, 1, 2
ELLIPSE, RECT = 0, 1
HEAD_PARTS = {18: [0, 14, 15, 16, 17], 15: [0, 1]}   # rtp_crops_head_parts
DEFAULTS = dict(effect=MOSAIC, shape=ELLIPSE, parts=None, min_score=0.0, min_parts=1, scale_q8=384, aspect_q8=320, pad=2, min_radius=4, cell=8, radius=8, colour=0)


def config(**kw):
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


def q(v):
    """overlay mode's rounding: clamp to +-32767, one float32 addition of 0.5, floor"""
    v = np.float32(min(max(np.float32(v), np.float32(-32767.0)), np.float32(32767.0)))
    return int(np.floor(np.float32(v + np.float32(0.5))))


def regions(joints, num_people, P, cfg):
    """-> [n] tuples (cx, cy, rx, ry, c, valid)"""
    j = np.asarray(joints, np.float32).reshape(-1, P, 3)
    people = j.shape[0] if num_people is None else num_people
    n = min(max(people, 0), MAX_PEOPLE)
    parts = cfg["parts"] if cfg["parts"] is not None else HEAD_PARTS[P]
    out = []
    for k in range(n):
        pts = [(j[k, p, 0], j[k, p, 1]) for p in parts if j[k, p, 2] > np.float32(cfg["min_score"]) and np.isfinite(j[k, p, 0]) and np.isfinite(j[k, p, 1])]
        c = len(pts)
        if c < cfg["min_parts"]:
            out.append((0, 0, 0, 0, c, 0))
            continue
        x0, x1 = q(min(p[0] for p in pts)), q(max(p[0] for p in pts))
        y0, y1 = q(min(p[1] for p in pts)), q(max(p[1] for p in pts))
        s = max(x1 - x0, y1 - y0) + 1
        rx = min(max(((s * cfg["scale_q8"]) >> 9) + cfg["pad"], cfg["min_radius"]), MAX_RADIUS)
        ry = min((rx * cfg["aspect_q8"]) >> 8, MAX_RADIUS)
        out.append(((x0 + x1) // 2, (y0 + y1) // 2, rx, ry, c, 1))   # (Python's // floors)
    return out


def coverage(regs, cfg, w, h):
    """[h][w] bool: the pixels at least one valid region covers"""
    px, py = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
    cov = np.zeros((h, w), bool)
    for cx, cy, rx, ry, _, valid in regs:
        if not valid:
            continue
        cx, cy = min(max(cx, -65535), 65535), min(max(cy, -65535), 65535)
        rx, ry = min(max(rx, 0), MAX_RADIUS), min(max(ry, 0), MAX_RADIUS)
        dx, dy = px - cx, py - cy
        inside = (np.abs(dx) <= rx) & (np.abs(dy) <= ry)
        if cfg["shape"] == ELLIPSE:
            inside &= (dx * ry) ** 2 + (dy * rx) ** 2 <= (rx * ry) ** 2
        cov |= inside
    return cov


def values(image, cfg):
    """the effect's value for EVERY pixel of the image as it is -> [h][w][3] uint8"""
    h, w = image.shape[:2]
    src = image.astype(np.int64)
    if cfg["effect"] == FILL:
        col = cfg["colour"]
        return np.broadcast_to(np.array([col & 255, (col >> 8) & 255, (col >> 16) & 255], np.uint8), (h, w, 3)).copy()
    out = np.zeros((h, w, 3), np.int64)
    if cfg["effect"] == MOSAIC:
        cell = cfg["cell"]
        for y0 in range(0, h, cell):
            for x0 in range(0, w, cell):
                block = src[y0:y0 + cell, x0:x0 + cell]
                cnt = block.shape[0] * block.shape[1]
                out[y0:y0 + cell, x0:x0 + cell] = (block.sum(axis=(0, 1)) + (cnt >> 1)) // cnt
        return out.astype(np.uint8)
    r = cfg["radius"]
    sat = np.zeros((h + 1, w + 1, 3), np.int64)
    sat[1:, 1:] = src.cumsum(axis=0).cumsum(axis=1)
    ys, xs = np.arange(h), np.arange(w)
    ya, yb = np.maximum(ys - r, 0), np.minimum(ys + r, h - 1) + 1
    xa, xb = np.maximum(xs - r, 0), np.minimum(xs + r, w - 1) + 1
    total = sat[yb][:, xb] - sat[ya][:, xb] - sat[yb][:, xa] + sat[ya][:, xa]
    cnt = ((yb - ya)[:, None] * (xb - xa)[None, :])[:, :, None]
    return ((total + (cnt >> 1)) // cnt).astype(np.uint8)


def apply(regs, cfg, image):
    """-> a new image: covered pixels take the value computed from `image` as it is, every other byte is image's"""
    img = np.asarray(image, np.uint8)
    cov = coverage(regs, cfg, img.shape[1], img.shape[0])
    out = img.copy()
    out[cov] = values(img, cfg)[cov]
    return out


def as_array(regs):
    return np.asarray(regs, np.int32).reshape(-1, REGION_INTS)

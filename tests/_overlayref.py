"""Overlay mode restated in numpy and Python integers from the text of include/rtpose_mi355x.h (THE UPDATE, AN ITEM, THE DRAWING): the
second, independent statement that tests/test_overlay_cpu.py holds rtp_overlay_update and rtp_overlay_draw to.  The palette and the
font are typed in here from the header, not imported from the package."""
import numpy as np

MAX_PEOPLE, MAX_TRACKS, TRAIL_MAX, ITEM_INTS = 96, 128, 32, 9
BOX, LABEL, TRAIL = 1, 2, 4
CAPSULE, RECT, LABEL_KIND = 1, 2, 3
PALETTE = [0x3C14DC, 0x32CD32, 0xFF901E, 0x00D7FF, 0xD355BA, 0xD1CE00, 0x008CFF, 0x9314FF, 0x578B2E, 0xE16941, 0x20A5DA, 0xCC3299, 0xAAB220, 0x2D52A0, 0x7FFF00, 0xB469FF]
FONT = [[0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E], [0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E], [0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F],
        [0x1E, 0x01, 0x01, 0x0E, 0x01, 0x01, 0x1E], [0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02], [0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E],
        [0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E], [0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08], [0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E],
        [0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C]]
DEFAULTS = dict(what=BOX | LABEL | TRAIL, min_score=0.0, box_margin=4, line_width=2, label_scale=1, trail_len=16, trail_radius=1, alpha=192)


class State:
    def __init__(self, num_parts):
        self.num_parts, self.frames = num_parts, 0
        self.owner = np.zeros(MAX_TRACKS, np.int64)
        self.count = np.zeros(MAX_TRACKS, np.int64)
        self.head = np.zeros(MAX_TRACKS, np.int64)
        self.pts = np.zeros((MAX_TRACKS, TRAIL_MAX, 2), np.int64)


def _q(v):
    """round half up after the clamp, the sum being ONE float32 addition"""
    v = np.float32(min(max(np.float32(v), np.float32(-32767.0)), np.float32(32767.0)))
    return int(np.floor(np.float32(v + np.float32(0.5))))


def update(st, joints, num_people, recs, **kw):
    """-> the frame's items, a list of 9-tuples of Python ints"""
    c = dict(DEFAULTS, **kw)
    P = st.num_parts
    n = min(max(int(num_people), 0), MAX_PEOPLE)
    j = np.asarray(joints, np.float32).reshape(-1, P, 3)
    st.frames = (st.frames + 1) & 0xFFFFFFFF or 1
    items = []
    for k in range(n):
        ident, t = int(recs[k][0]), int(recs[k][1])
        if ident == 0:
            continue
        x, y, s = j[k, :, 0], j[k, :, 1], j[k, :, 2]
        with np.errstate(invalid="ignore"):
            counts = (s > np.float32(c["min_score"])) & np.isfinite(x) & np.isfinite(y)
        if not counts.any():
            continue
        m = c["box_margin"]
        x0, y0 = _q(x[counts].min()) - m, _q(y[counts].min()) - m
        x1, y1 = _q(x[counts].max()) + m, _q(y[counts].max()) + m
        if st.owner[t] != ident:
            st.owner[t], st.count[t], st.head[t] = ident, 0, 0
        st.pts[t, st.head[t]] = ((x0 + x1) // 2, (y0 + y1) // 2)
        st.head[t] = (st.head[t] + 1) % TRAIL_MAX
        st.count[t] = min(st.count[t] + 1, c["trail_len"])
        colour = PALETTE[ident & 15]
        cnt, head = int(st.count[t]), int(st.head[t])
        if c["what"] & TRAIL:
            kept = [tuple(int(v) for v in st.pts[t, (head - cnt + i) % TRAIL_MAX]) for i in range(cnt)]
            pairs = len(kept) - 1
            for i in range(pairs):
                items.append((CAPSULE, kept[i][0], kept[i][1], kept[i + 1][0], kept[i + 1][1], c["trail_radius"], colour, c["alpha"] * (i + 1) // pairs, 0))
        if c["what"] & BOX:
            items.append((RECT, x0, y0, x1, y1, c["line_width"], colour, c["alpha"], 0))
        if c["what"] & LABEL:
            digits = len(str(ident & 0xFFFFFFFF))
            lw, lh = (6 * digits + 1) * c["label_scale"], 9 * c["label_scale"]
            ly = y0 - lh if y0 - lh >= 0 else y0
            items.append((LABEL_KIND, x0, ly, x0 + lw - 1, ly + lh - 1, c["label_scale"], colour, c["alpha"], ident))
    return items


def _clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def coverage(item, w, h):
    """-> int array [h][w]: 0 = not covered, 1 = the item's colour, 2 = the text colour.  Exact: Python integers where products are large."""
    kind = int(item[0])
    cov = np.zeros((h, w), np.int64)
    if kind not in (CAPSULE, RECT, LABEL_KIND):
        return cov
    x0, y0, x1, y1 = (_clamp(v, -65535, 65535) for v in item[1:5])
    size = _clamp(item[5], 1, 8) if kind == LABEL_KIND else _clamp(item[5], 0, 16)
    py, px = np.mgrid[0:h, 0:w]
    if kind == RECT:
        inside = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        edge = (px - x0 < size) | (x1 - px < size) | (py - y0 < size) | (y1 - py < size)
        cov[inside & edge] = 1
    elif kind == CAPSULE:
        # (only pixels within `size` of the segment's bounding box can be covered: the rest is not evaluated)
        ya, yb = max(min(y0, y1) - size, 0), min(max(y0, y1) + size, h - 1) + 1
        xa, xb = max(min(x0, x1) - size, 0), min(max(x0, x1) + size, w - 1) + 1
        if ya < yb and xa < xb:
            py, px = np.mgrid[ya:yb, xa:xb]
            px, py = px.astype(object), py.astype(object)    # Python integers: nothing overflows
            dx, dy, r2 = x1 - x0, y1 - y0, size * size
            ux, uy = px - x0, py - y0
            L, t = dx * dx + dy * dy, ux * dx + uy * dy
            near_a = (ux * ux + uy * uy) <= r2
            near_b = ((px - x1) * (px - x1) + (py - y1) * (py - y1)) <= r2
            cross = ux * dy - uy * dx
            strip = (cross * cross) <= r2 * L
            hit = near_a if L == 0 else np.where(t < 0, near_a, np.where(t > L, near_b, strip))
            cov[ya:yb, xa:xb][hit.astype(bool)] = 1
    else:
        text = str(int(item[8]) & 0xFFFFFFFF)
        inside = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        cov[inside] = 1
        for yy, xx in zip(*np.nonzero(inside)):
            u, v = (int(xx) - x0) // size, (int(yy) - y0) // size
            if 1 <= v <= 7 and u >= 1:
                col, i = (u - 1) % 6, (u - 1) // 6
                if col < 5 and i < len(text) and (FONT[int(text[i])][v - 1] >> (4 - col)) & 1:
                    cov[yy, xx] = 2
    return cov


def draw(items, image):
    """-> a new image [h][w][3] uint8 with the items drawn in order"""
    img = np.array(image, np.int64)
    h, w = img.shape[:2]
    for it in items:
        cov = coverage(it, w, h)
        if not cov.any():
            continue
        a = _clamp(it[7], 0, 256)
        b, g, r = int(it[6]) & 255, (int(it[6]) >> 8) & 255, (int(it[6]) >> 16) & 255
        text = 0 if (29 * b + 150 * g + 77 * r) >> 8 >= 128 else 255
        for ch, col in enumerate((b, g, r)):
            c = np.where(cov == 2, text, col)
            img[..., ch] = np.where(cov > 0, (img[..., ch] * (256 - a) + c * a + 128) >> 8, img[..., ch])
    return img.astype(np.uint8)


def as_array(items):
    return np.asarray(items, np.int32).reshape(-1, ITEM_INTS)


def same_state(ref, got):
    """None when the TrailState `got` holds the restatement's table, else what differs"""
    if got.frames != ref.frames or got.num_parts != ref.num_parts:
        return f"frames {got.frames} / num_parts {got.num_parts}, expected {ref.frames} / {ref.num_parts}"
    for name in ("owner", "count", "head", "pts"):
        a, b = getattr(ref, name), got.slot[name].astype(np.int64)
        if not np.array_equal(a, b):
            w = tuple(int(v) for v in np.argwhere(a != b)[0])
            return f"slot {name}{w}: {b[w]}, expected {a[w]}"
    return None

"""Appearance-aided tracking restated in numpy from the text of include/rtpose_mi355x.h alone ("THE DESCRIPTOR", "THE TABLE", "THE
COST", "THE TABLE UPDATE"): np.float32 scalars, one operation per statement, python integers past the four Q16 conversions.
tests/test_appearance_cpu.py holds rtp_appearance_describe and rtp_track_update_appearance to it; the GPU tests then compare against
those two."""
import numpy as np

import _trackref as tr

MAX_TRACKS, MAX_PEOPLE, MAX_PARTS, REC_INTS = tr.MAX_TRACKS, tr.MAX_PEOPLE, tr.MAX_PARTS, tr.REC_INTS
BINS, GRID = 128, 32
F = np.float32
DEFAULTS = dict(parts=None, min_score=0.0, min_parts=3, margin=0.0, weight=0.125, max_dist=1.0, unknown=0.25, rate=32)
TORSO = {18: [1, 2, 5, 8, 11], 15: [1, 2, 5, 8, 11, 14]}


def config(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return {**DEFAULTS, **kw}


def part_list(c, P):
    """the configuration's list; None = the model's torso parts (models of 18 and 15 parts), every part for any other model"""
    if c["parts"] is not None:
        return list(c["parts"])
    return TORSO.get(P, list(range(P)))


class State:
    def __init__(self):
        self.owner = np.zeros(MAX_TRACKS, np.int32)
        self.desc = np.zeros((MAX_TRACKS, BINS), np.uint16)

    def copy(self):
        s = State()
        s.owner, s.desc = self.owner.copy(), self.desc.copy()
        return s


def _rint(v):
    """(int64)rintf(v) of a finite float32: round half to even"""
    return int(np.rint(F(v)))


def box(person, plist, c):
    """-> (left, top, w, h) as float32, or None where the person has no descriptor"""
    x0, x1, y0, y1 = F(np.inf), F(-np.inf), F(np.inf), F(-np.inf)
    zero = F(0.0)
    count = 0
    for p in plist:
        x, y, s = F(person[p, 0]), F(person[p, 1]), F(person[p, 2])
        if not (bool(s > F(c["min_score"])) and bool(np.isfinite(x)) and bool(np.isfinite(y))):
            continue
        x = F(x + zero)
        y = F(y + zero)
        x0, x1, y0, y1 = min(x0, x), max(x1, x), min(y0, y), max(y1, y)
        count += 1
    if count < c["min_parts"]:
        return None
    sx = F(x0 + x1)
    sy = F(y0 + y1)
    cx = F(sx * F(0.5))
    cy = F(sy * F(0.5))
    w = F(x1 - x0)
    h = F(y1 - y0)
    if not (np.isfinite(w) and np.isfinite(h)):
        return None
    gm = F(F(c["margin"]) * max(w, h))
    g = F(gm * F(2.0))
    wg = F(w + g)
    hg = F(h + g)
    w = max(wg, F(1.0))
    h = max(hg, F(1.0))
    hw = F(w * F(0.5))
    hh = F(h * F(0.5))
    left = F(cx - hw)
    top = F(cy - hh)
    right = F(left + w)
    bottom = F(top + h)
    lim = F(1048576.0)
    if not (abs(left) <= lim and abs(top) <= lim and abs(right) <= lim and abs(bottom) <= lim):   # (a NaN fails)
        return None
    return left, top, w, h


def describe(image, joints, num_parts, **kw):
    """-> (bins [n][128] uint16, valid [n] uint8) of joints [people][num_parts][3] on the u8 BGR image [h][w][3]"""
    c = config(**kw)
    img = np.ascontiguousarray(image, np.uint8)
    ih, iw = img.shape[:2]
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, num_parts, 3)
    n = min(j.shape[0], MAX_PEOPLE)
    plist = part_list(c, num_parts)
    bins = np.zeros((n, BINS), np.uint16)
    valid = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        for k in range(n):
            b = box(j[k], plist, c)
            if b is None:
                continue
            left, top, w, h = b
            ox = _rint(F(left * F(65536.0)))
            oy = _rint(F(top * F(65536.0)))
            dx = _rint(F(F(w / F(32.0)) * F(65536.0)))
            dy = _rint(F(F(h / F(32.0)) * F(65536.0)))
            cols = [min(max((ox + i * dx + dx // 2) >> 16, 0), iw - 1) for i in range(GRID)]
            rows = [min(max((oy + i * dy + dy // 2) >> 16, 0), ih - 1) for i in range(GRID)]
            px = img[np.array(rows)[:, None], np.array(cols)[None, :]].astype(np.int64)   # [j][i][BGR]
            code = (px[:, :, 2] >> 6) * 16 + (px[:, :, 1] >> 6) * 4 + (px[:, :, 0] >> 6)
            code[16:] += 64
            bins[k] = np.bincount(code.ravel(), minlength=BINS).astype(np.uint16)
            valid[k] = 1
    return bins, valid


def update(ts, ap, joints, num_people=None, bins=None, valid=None, track=None, **kw):
    """one frame; ts: a _trackref.State, ap: a State; track: the keywords of the tracking configuration; -> records [n][4] int64"""
    c = config(**kw)
    tcfg = tr.config(**(track or {}))
    P = ts.num_parts
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, P, 3)
    people = j.shape[0] if num_people is None else num_people
    n = min(max(people, 0), MAX_PEOPLE)
    zero = F(0.0)
    if bins is None:
        ok = np.zeros(n, bool)
    else:
        ok = np.asarray(valid)[:n] != 0
        b16 = np.asarray(bins, np.int64).reshape(-1, BINS)[:n] * 16
    with np.errstate(all="ignore"):
        # 1, 2: as in tracking mode
        pc = np.array([[tr._counts(j[k, p], tcfg["min_score"]) for p in range(P)] for k in range(n)], bool).reshape(n, P)
        trackable = [int(pc[k].sum()) >= tcfg["min_parts"] for k in range(n)]
        has = (ap.owner == ts.id) & (ts.id != 0)
        cand = []
        for t in range(MAX_TRACKS):
            if ts.id[t] == 0:
                continue
            tj = ts.joints[t]
            tcn = [tr._counts(tj[p], tcfg["min_score"]) for p in range(P)]
            x0, x1, y0, y1 = F(np.inf), F(-np.inf), F(np.inf), F(-np.inf)
            for p in range(P):
                if not tcn[p]:
                    continue
                x = F(tj[p, 0] + zero)
                y = F(tj[p, 1] + zero)
                x0, x1, y0, y1 = min(x0, x), max(x1, x), min(y0, y), max(y1, y)
            w = F(x1 - x0)
            h = F(y1 - y0)
            ww = F(w * w)
            hh = F(h * h)
            wh = F(ww + hh)
            d = wh if wh > F(1.0) else F(1.0)
            s, m = np.zeros(n, np.float32), np.zeros(n, np.int64)
            for p in range(P):
                if not tcn[p]:
                    continue
                both = pc[:, p]
                dx = j[:n, p, 0] - tj[p, 0]
                dy = j[:n, p, 1] - tj[p, 1]
                a = dx * dx
                b = dy * dy
                cc = a + b
                s = np.where(both, s + cc, s)
                m = m + both
            for k in range(n):
                if not trackable[k] or m[k] < tcfg["min_common"]:
                    continue
                q = F(s[k] / F(m[k]))
                cost = F(q / d)
                if not np.isfinite(cost) or not cost <= F(tcfg["max_cost"]):
                    continue
                # THE COST
                if has[t] and ok[k]:
                    L = int(np.abs(ap.desc[t].astype(np.int64) - b16[k]).sum())
                    a = F(F(L) / F(32768.0))
                    if not a <= F(c["max_dist"]):
                        continue
                else:
                    a = F(c["unknown"])
                wa = F(F(c["weight"]) * a)
                total = F(cost + wa)
                if not np.isfinite(total):
                    continue
                cand.append((tr.bits(F(total + zero)), t, k))
        # 3
        cand.sort()
        slot_of, person_of, cost_of = {}, {}, {}
        for b, t, k in cand:
            if t in person_of or k in slot_of:
                continue
            person_of[t], slot_of[k], cost_of[k] = k, t, b
        # 4, 5
        for t in range(MAX_TRACKS):
            if ts.id[t] == 0:
                continue
            if t in person_of:
                ts.joints[t, :P] = j[person_of[t]]
                ts.hits[t] += 1
                ts.misses[t] = 0
            else:
                ts.misses[t] += 1
                if ts.misses[t] > tcfg["max_misses"]:
                    ts.id[t] = ts.hits[t] = ts.misses[t] = 0
                    ts.joints[t] = 0
        # 6
        born = set()
        for k in range(n):
            if not trackable[k] or k in slot_of:
                continue
            free = np.flatnonzero(ts.id == 0)
            if not len(free):
                break
            t = int(free[0])
            if ts.next_id == 0:
                ts.next_id = 1
            ts.id[t] = np.array([ts.next_id], np.uint32).view(np.int32)[0]
            ts.next_id = (ts.next_id + 1) & 0xFFFFFFFF
            if ts.next_id == 0:
                ts.next_id = 1
            ts.hits[t], ts.misses[t] = 1, 0
            ts.joints[t, :P] = j[k]
            slot_of[k] = t
            born.add(k)
        # THE TABLE UPDATE
        rate = int(c["rate"])
        for k in range(n):
            if k not in slot_of or not ok[k]:
                continue
            t = slot_of[k]
            if ap.owner[t] == ts.id[t] and ts.id[t] != 0:
                ap.desc[t] = ((ap.desc[t].astype(np.int64) * (256 - rate) + b16[k] * rate + 128) >> 8).astype(np.uint16)
            else:
                ap.desc[t] = b16[k].astype(np.uint16)
                ap.owner[t] = ts.id[t]
        # 7
        ts.frames = (ts.frames + 1) & 0xFFFFFFFF
    recs = np.zeros((n, REC_INTS), np.int64)
    for k in range(n):
        if k not in slot_of:
            recs[k] = (0, -1, 0, 0)
        else:
            t = slot_of[k]
            recs[k] = (ts.id[t], t, ts.hits[t], 0 if k in born else cost_of[k])
    return recs


def same_state(ref, st):
    """ref (State) against a caffe_rtpose_amd.AppearanceState; -> None or what differs"""
    if not np.array_equal(ref.owner, st.owner):
        return f"owner differs in slots {np.flatnonzero(ref.owner != st.owner).tolist()}"
    if not np.array_equal(ref.desc, st.desc):
        return f"desc differs in slots {np.flatnonzero((ref.desc != st.desc).any(1)).tolist()}"
    return None

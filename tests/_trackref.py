"""Tracking mode restated in numpy from the text of include/rtpose_mi355x.h alone ("THE UPDATE", "THE RECORD"): np.float32 scalars,
one operation per statement.  tests/test_track_cpu.py holds rtp_track_update to it; the GPU tests then compare against
rtp_track_update."""
import numpy as np

MAX_TRACKS, MAX_PEOPLE, MAX_PARTS, REC_INTS = 128, 96, 70, 4
F = np.float32
DEFAULTS = dict(min_score=0.0, min_parts=3, min_common=2, max_cost=0.0625, max_misses=15)


def config(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return {**DEFAULTS, **kw}


class State:
    def __init__(self, num_parts):
        assert 1 <= num_parts <= MAX_PARTS
        self.num_parts = num_parts
        self.next_id = 1
        self.frames = 0
        self.id = np.zeros(MAX_TRACKS, np.int32)
        self.hits = np.zeros(MAX_TRACKS, np.int32)
        self.misses = np.zeros(MAX_TRACKS, np.int32)
        self.joints = np.zeros((MAX_TRACKS, MAX_PARTS, 3), np.float32)

    def copy(self):
        s = State(self.num_parts)
        s.next_id, s.frames = self.next_id, self.frames
        s.id, s.hits, s.misses, s.joints = self.id.copy(), self.hits.copy(), self.misses.copy(), self.joints.copy()
        return s


def bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _counts(part, min_score):
    x, y, s = F(part[0]), F(part[1]), F(part[2])
    return bool(s > F(min_score)) and bool(np.isfinite(x)) and bool(np.isfinite(y))   # (a NaN score fails the comparison)


def update(st, joints, num_people=None, **kw):
    """one frame; -> records [n][4] int64 (cost bits as unsigned)"""
    c = config(**kw)
    P = st.num_parts
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, P, 3)
    people = j.shape[0] if num_people is None else num_people
    n = min(max(people, 0), MAX_PEOPLE)
    zero = F(0.0)
    with np.errstate(all="ignore"):
        # 1
        pc = [[_counts(j[k, p], c["min_score"]) for p in range(P)] for k in range(n)]
        trackable = [sum(pc[k]) >= c["min_parts"] for k in range(n)]
        pcm = np.array(pc, bool).reshape(n, P)
        # 2
        cand = []
        for t in range(MAX_TRACKS):
            if st.id[t] == 0:
                continue
            tj = st.joints[t]
            tc = [_counts(tj[p], c["min_score"]) for p in range(P)]
            x0, x1, y0, y1 = F(np.inf), F(-np.inf), F(np.inf), F(-np.inf)
            for p in range(P):
                if not tc[p]:
                    continue
                x = F(tj[p, 0] + zero)
                y = F(tj[p, 1] + zero)
                x0, x1, y0, y1 = min(x0, x), max(x1, x), min(y0, y), max(y1, y)
            w = F(x1 - x0)
            h = F(y1 - y0)
            ww = F(w * w)
            hh = F(h * h)
            wh = F(ww + hh)
            d = wh if wh > F(1.0) else F(1.0)   # fmaxf(ww + hh, 1.0f): never a NaN here (ww, hh >= 0 or +inf)
            # (all people at once, as float32 arrays: every element is still one rounded operation per statement, parts in order)
            s, m = np.zeros(n, np.float32), np.zeros(n, np.int64)
            for p in range(P):
                if not tc[p]:
                    continue
                both = pcm[:, p]
                dx = j[:n, p, 0] - tj[p, 0]
                dy = j[:n, p, 1] - tj[p, 1]
                a = dx * dx
                b = dy * dy
                cc = a + b
                s = np.where(both, s + cc, s)
                m = m + both
            assert s.dtype == np.float32
            for k in range(n):
                if not trackable[k] or m[k] < c["min_common"]:
                    continue
                q = F(s[k] / F(m[k]))
                cost = F(q / d)
                if not np.isfinite(cost) or not cost <= F(c["max_cost"]):
                    continue
                cand.append((bits(F(cost + zero)), t, k))
        # 3
        cand.sort()
        slot_of, person_of, cost_of = {}, {}, {}
        for b, t, k in cand:
            if t in person_of or k in slot_of:
                continue
            person_of[t], slot_of[k], cost_of[k] = k, t, b
        # 4, 5
        for t in range(MAX_TRACKS):
            if st.id[t] == 0:
                continue
            if t in person_of:
                st.joints[t, :P] = j[person_of[t]]
                st.hits[t] += 1
                st.misses[t] = 0
            else:
                st.misses[t] += 1
                if st.misses[t] > c["max_misses"]:
                    st.id[t] = st.hits[t] = st.misses[t] = 0
                    st.joints[t] = 0
        # 6
        born = set()
        for k in range(n):
            if not trackable[k] or k in slot_of:
                continue
            free = np.flatnonzero(st.id == 0)
            if not len(free):
                break
            t = int(free[0])
            if st.next_id == 0:
                st.next_id = 1
            st.id[t] = np.array([st.next_id], np.uint32).view(np.int32)[0]
            st.next_id = (st.next_id + 1) & 0xFFFFFFFF
            if st.next_id == 0:
                st.next_id = 1
            st.hits[t], st.misses[t] = 1, 0
            st.joints[t, :P] = j[k]
            slot_of[k] = t
            born.add(k)
        # 7
        st.frames = (st.frames + 1) & 0xFFFFFFFF
    recs = np.zeros((n, REC_INTS), np.int64)
    for k in range(n):
        if k not in slot_of:
            recs[k] = (0, -1, 0, 0)
        else:
            t = slot_of[k]
            recs[k] = (st.id[t], t, st.hits[t], 0 if k in born else cost_of[k])
    return recs


def same_state(ref, ts):
    """ref (State) against a caffe_rtpose_amd.TrackState: int for int, float bit for float bit; -> None or what differs"""
    if (ref.num_parts, ref.next_id, ref.frames) != (ts.num_parts, ts.next_id, ts.frames):
        return f"num_parts / next_id / frames {(ref.num_parts, ref.next_id, ref.frames)} against {(ts.num_parts, ts.next_id, ts.frames)}"
    for name in ("id", "hits", "misses"):
        a, b = getattr(ref, name), getattr(ts, name)
        if not np.array_equal(a, b):
            return f"{name} differs in slots {np.flatnonzero(a != b).tolist()}"
    a, b = ref.joints.view(np.uint32), np.ascontiguousarray(ts.joints, np.float32).view(np.uint32)
    if not np.array_equal(a, b):
        return f"joints differ in slots {np.flatnonzero((a != b).reshape(MAX_TRACKS, -1).any(1)).tolist()}"
    return None


def same_recs(ref, got):
    """reference records (int64, cost bits unsigned) against int32 records"""
    got = np.ascontiguousarray(got, np.int32).reshape(-1, REC_INTS)
    return ref.shape == got.shape and np.array_equal(ref.astype(np.uint32), got.view(np.uint32))

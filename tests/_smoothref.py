"""Smoothing mode restated in numpy from the text of include/rtpose_mi355x.h alone ("THE UPDATE" of smoothing mode): np.float32
scalars, one operation per statement, gaps in uint32 arithmetic.  tests/test_smooth_cpu.py holds rtp_smooth_update to it; the GPU
tests then compare against rtp_smooth_update.  It shares no code with the library."""
import numpy as np

MAX_TRACKS, MAX_PEOPLE, MAX_PARTS, REC_INTS = 128, 96, 70, 4
F = np.float32
U = 0xFFFFFFFF
TWO_PI = np.array([0x40C90FDB], np.uint32).view(np.float32)[0]
DEFAULTS = dict(min_score=0.0, min_cutoff=float(F(1.0) / F(30.0)), beta=0.01, d_cutoff=float(F(1.0) / F(30.0)), max_hold=5)


def config(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return {**DEFAULTS, **kw}


class State:
    def __init__(self, num_parts):
        assert 1 <= num_parts <= MAX_PARTS
        self.num_parts = num_parts
        self.frames = 0
        self.owner = np.zeros((MAX_TRACKS, MAX_PARTS), np.int32)
        self.last = np.zeros((MAX_TRACKS, MAX_PARTS), np.uint32)
        self.pos = np.zeros((MAX_TRACKS, MAX_PARTS, 2), np.float32)
        self.vel = np.zeros((MAX_TRACKS, MAX_PARTS, 2), np.float32)
        self.score = np.zeros((MAX_TRACKS, MAX_PARTS), np.float32)

    def copy(self):
        s = State(self.num_parts)
        s.frames = self.frames
        s.owner, s.last, s.pos, s.vel, s.score = self.owner.copy(), self.last.copy(), self.pos.copy(), self.vel.copy(), self.score.copy()
        return s


def bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _coordinate(v, vh, dvh, dt, c):
    """one coordinate of the FILTER step -> (vh', e)"""
    d = F(v - vh)
    dv = F(d / dt)
    rd = F(TWO_PI * F(c["d_cutoff"]))
    rd = F(rd * dt)
    ad = F(rd / F(rd + F(1.0)))
    t1 = F(ad * dv)
    t2 = F(F(F(1.0) - ad) * dvh)
    e = F(t1 + t2)
    fc = F(F(c["beta"]) * F(np.abs(e)))
    fc = F(F(c["min_cutoff"]) + fc)
    r = F(TWO_PI * fc)
    r = F(r * dt)
    a = F(r / F(r + F(1.0)))
    u1 = F(a * v)
    u2 = F(F(F(1.0) - a) * vh)
    return F(u1 + u2), e


def update(st, joints, num_people, recs, **kw):
    """one frame; recs [n][4] -> (joints_s [n][P][3] float32, vel [n][P][2] float32, flags [n][P] uint8)"""
    c = config(**kw)
    P = st.num_parts
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, P, 3)
    people = j.shape[0] if num_people is None else num_people
    n = min(max(people, 0), MAX_PEOPLE)
    rc = np.asarray(recs, np.int64).reshape(-1, REC_INTS)
    js, vel, flags = np.zeros((n, P, 3), np.float32), np.zeros((n, P, 2), np.float32), np.zeros((n, P), np.uint8)
    st.frames = (st.frames + 1) & U
    if st.frames == 0:
        st.frames = 1
    now = st.frames
    max_hold = c["max_hold"]
    with np.errstate(all="ignore"):
        for k in range(n):
            ident, t = int(np.int32(rc[k, 0])), int(np.int32(rc[k, 1]))
            for p in range(P):
                x, y, s = j[k, p]
                counts = bool(s > F(c["min_score"])) and bool(np.isfinite(x)) and bool(np.isfinite(y))
                js[k, p] = j[k, p]          # (a bit copy: float32 to float32)
                if ident == 0:
                    flags[k, p] = 1 if counts else 0
                    continue
                live = int(st.owner[t, p]) == ident and int(st.last[t, p]) != 0
                g = (now - int(st.last[t, p])) & U
                start = counts and (not live or ((g - 1) & U) > max_hold)
                if counts and not start:
                    dt = F(g)
                    xh, ex = _coordinate(x, st.pos[t, p, 0], st.vel[t, p, 0], dt, c)
                    yh, ey = _coordinate(y, st.pos[t, p, 1], st.vel[t, p, 1], dt, c)
                    if np.isfinite(xh) and np.isfinite(yh) and np.isfinite(ex) and np.isfinite(ey):
                        st.pos[t, p] = (xh, yh)
                        st.vel[t, p] = (ex, ey)
                        st.score[t, p] = s
                        st.last[t, p] = now
                        js[k, p, 0], js[k, p, 1] = xh, yh
                        vel[k, p] = (ex, ey)
                        flags[k, p] = 2
                    else:
                        start = True
                if start:
                    st.owner[t, p] = ident
                    st.last[t, p] = now
                    st.pos[t, p] = (x, y)
                    st.vel[t, p] = 0
                    st.score[t, p] = s
                    flags[k, p] = 1
                elif not counts:
                    if live and g <= max_hold:
                        js[k, p, :2] = st.pos[t, p]
                        js[k, p, 2] = st.score[t, p]
                        vel[k, p] = st.vel[t, p]
                        flags[k, p] = 3
                    else:
                        flags[k, p] = 0
    return js, vel, flags


def same_out(want, got):
    """None, or what differs between two (joints_s, vel, flags) triples (floats by their bits)"""
    for name, a, b in zip(("joints_s", "vel", "flags"), want, got):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape:
            return f"{name}: shape {b.shape}, expected {a.shape}"
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)
        if not np.array_equal(a, b):
            w = np.argwhere(a != b)[0]
            return f"{name}{tuple(int(v) for v in w)}: {b[tuple(w)]:#x}, expected {a[tuple(w)]:#x} ({len(np.argwhere(a != b))} differ)"
    return None


def same_state(ref, lib_state):
    """None, or what differs between a State and the library's SmoothState (the whole table, floats by their bits)"""
    if (ref.num_parts, ref.frames) != (lib_state.num_parts, lib_state.frames):
        return f"num_parts / frames {(lib_state.num_parts, lib_state.frames)}, expected {(ref.num_parts, ref.frames)}"
    cell = lib_state.cell
    for name, a in (("owner", ref.owner), ("last", ref.last), ("pos", ref.pos), ("vel", ref.vel), ("score", ref.score)):
        b = np.ascontiguousarray(cell[name])
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if not np.array_equal(a, b):
            w = tuple(int(v) for v in np.argwhere(a != b)[0])
            return f"cell {name}{w}: {b[w]}, expected {a[w]}"
    return None

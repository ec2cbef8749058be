"""Short joint sequences for smoothing mode, one per rule of the definition in include/rtpose_mi355x.h, each with a predicate that
says what the sequence is there to reach.  Every sequence runs through the tracker first (the records are its), then through the
filter.  The inputs are chosen so that tests/_trackref.py and tests/_smoothref.py alone satisfy every predicate (check_predicates;
tests/test_smooth_cpu.py runs it on the CPU).

A case: dict(name, P, tcfg / scfg (keywords of the two configurations that differ from the defaults), frames [(joints [people][P][3],
num_people or None = the array's)], pred(out per frame = (joints_s, vel, flags), smoothing state after each frame, records per
frame) -> bool)."""
import numpy as np

import _smoothref as sr
import _trackcases as tc
import _trackref as tr

NAN, INF = float("nan"), float("inf")
body, shifted, frame = tc.body, tc.shifted, tc.frame


def without(j, parts, score=0.0):
    o = j.copy()
    for p in parts:
        o[p, 2] = score
    return o


def fl(o, i, k=0):
    """the flags of person k of frame i as a list"""
    return [int(v) for v in o[i][2][k]]


def bit_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def cases(P):
    A, B = body(P, 100, 100), body(P, 400, 100)
    out = []

    def add(name, frames, pred, tcfg=None, **scfg):
        out.append(dict(name=f"{name}_P{P}", P=P, tcfg=tcfg or {}, scfg=scfg, frames=frames, pred=pred))

    add("nobody", [frame(A, P=P), frame(P=P), frame(shifted(A, 1, 0), P=P)],
        lambda o, s, r: o[1][0].shape == (0, P, 3) and o[1][2].shape == (0, P) and s[1].frames == 2 and (s[1].last[0, :P] == 1).all()
        and fl(o, 2) == [2] * P and (s[2].last[0, :P] == 3).all())
    crowd = np.stack([body(P, 100 * (i % 12), 100 * (i // 12)) for i in range(96)]).astype(np.float32)
    add("num_people_out_of_range", [(crowd, 200), (crowd, -3), (crowd[:2].copy(), None)],
        lambda o, s, r: o[0][0].shape == (96, P, 3) and (o[0][2] == 1).all() and o[1][0].shape == (0, P, 3) and s[1].frames == 2
        and o[2][0].shape == (2, P, 3) and (o[2][2] == 2).all() and (s[2].last[:2, :P] == 3).all() and (s[2].last[2:96, :P] == 1).all())
    add("one_person", [frame(A, P=P), frame(shifted(A, 1, 0), P=P), frame(shifted(A, 2, 0.5), P=P)],
        lambda o, s, r: fl(o, 0) == [1] * P and fl(o, 1) == [2] * P and fl(o, 2) == [2] * P and not o[0][1].any() and (o[1][1][0, :, 0] > 0).all()
        and not o[1][1][0, :, 1].any() and (o[2][1][0, :, 1] > 0).all() and (o[1][0][0, :, 0] > A[:, 0]).all() and (o[1][0][0, :, 0] < A[:, 0] + 1).all()
        and bit_equal(o[2][0][0, :, 2], A[:, 2]) and not s[2].owner[:, P:].any() and not s[2].last[1:].any())
    add("ninety_six_people", [(crowd, None), (crowd + np.float32(0.5), None), (crowd[::-1].copy(), None)],
        lambda o, s, r: (o[1][2] == 2).all() and (o[2][2] == 2).all() and sorted(int(x) for x in r[2][:, 1]) == list(range(96)) and int(r[2][0, 1]) == 95
        and (s[2].last[:96, :P] == 3).all() and not s[2].last[96:].any())
    few = body(P, 400, 100, parts={1, 4})
    few[6] = (NAN, 3.0, 1.0)
    few[7] = (3.0, 2.0, NAN)
    add("untracked_person", [frame(A, few, P=P), frame(shifted(A, 1, 0), few, P=P)],
        lambda o, s, r: int(r[1][1, 0]) == 0 and fl(o, 1, 1) == [1 if p in (1, 4) else 0 for p in range(P)] and bit_equal(o[1][0][1], few) and not o[1][1][1].any()
        and not s[1].owner[1:].any() and fl(o, 1, 0) == [2] * P)
    gone = without(A, {5, 7})
    add("held_for_exactly_max_hold", [frame(A, P=P), frame(A, P=P), frame(gone, P=P), frame(gone, P=P), frame(shifted(A, 1, 0), P=P)],
        lambda o, s, r: [fl(o, i)[5] for i in range(5)] == [1, 2, 3, 3, 2] and [fl(o, i)[7] for i in range(5)] == [1, 2, 3, 3, 2]
        and bit_equal(o[3][0][0, 5], (s[1].pos[0, 5, 0], s[1].pos[0, 5, 1], A[5, 2])) and s[3].last[0, 5] == 2 and s[4].last[0, 5] == 5
        and fl(o, 4)[4] == 2, max_hold=2)
    add("held_for_max_hold_plus_one", [frame(A, P=P), frame(A, P=P), frame(gone, P=P), frame(gone, P=P), frame(gone, P=P), frame(shifted(A, 1, 0), P=P)],
        lambda o, s, r: [fl(o, i)[5] for i in range(6)] == [1, 2, 3, 3, 0, 1] and bit_equal(o[4][0][0, 5], gone[5]) and not o[4][1][0, 5].any()
        and bit_equal(o[5][0][0, 5], shifted(A, 1, 0)[5]) and not o[5][1][0, 5].any() and fl(o, 5)[4] == 2, max_hold=2)
    k = 3
    moved = shifted(A, 4, 0)
    add("track_missed_and_rematched", [frame(A, P=P)] + [frame(P=P)] * k + [frame(moved, P=P)],
        lambda o, s, r: [int(v) for v in r[k + 1][0, :3]] == [1, 0, 2] and fl(o, k + 1) == [2] * P and (s[k + 1].last[0, :P] == k + 2).all()
        # dt = k + 1: the first velocity estimate is ad * (4 / dt), with ad = rd / (rd + 1), rd = TWO_PI * d_cutoff * dt
        and bit_equal(o[k + 1][1][0, :, 0], [_first_velocity(4.0, k + 1)] * P), max_hold=k)
    add("slot_reborn_with_a_new_id", [frame(A, P=P), frame(P=P), frame(shifted(A, 200, 0), P=P)],
        lambda o, s, r: [int(v) for v in r[2][0, :2]] == [2, 0] and fl(o, 2) == [1] * P and (s[1].owner[0, :P] == 1).all() and (s[2].owner[0, :P] == 2).all()
        and (s[2].last[0, :P] == 3).all() and not o[2][1].any(), tcfg=dict(max_misses=0))
    bad = body(P, 100, 100)
    bad[3, 0], bad[4, 1], bad[5, 0], bad[6, 1], bad[8, 2], bad[9, 2] = INF, NAN, NAN, -INF, NAN, INF
    turns_bad = A.copy()
    turns_bad[2, 0], turns_bad[10, 2] = NAN, NAN
    add("nan_and_inf", [frame(bad, P=P), frame(shifted(bad, 1, 0), P=P), frame(A, P=P), frame(turns_bad, P=P)],
        lambda o, s, r: [fl(o, 1)[p] for p in (3, 4, 5, 6, 8, 9)] == [0, 0, 0, 0, 0, 2] and bit_equal(o[1][0][0, 4], shifted(bad, 1, 0)[4]) and fl(o, 2)[3] == 1
        and fl(o, 3)[2] == 3 and fl(o, 3)[10] == 3 and np.isfinite(o[3][0][0, 2]).all() and np.isfinite(o[3][0][0, 10]).all() and s[3].last[0, 2] == 3)
    add("max_hold_zero", [frame(A, P=P), frame(A, P=P), frame(gone, P=P), frame(A, P=P), frame(A, P=P)],
        lambda o, s, r: [fl(o, i)[5] for i in range(5)] == [1, 2, 0, 1, 2] and [fl(o, i)[4] for i in range(5)] == [1, 2, 2, 2, 2], max_hold=0)
    add("huge_beta_overflows_r", [frame(A, P=P), frame(moved, P=P), frame(moved, P=P)],
        lambda o, s, r: [int(v) for v in r[1][0, :3]] == [1, 0, 2] and fl(o, 1) == [1] * P and bit_equal(o[1][0][0], moved) and not o[1][1].any()
        and fl(o, 2) == [2] * P and np.isfinite(o[2][0]).all(), beta=3e38)
    # parts the tracker does not count (score under ITS min_score) and the filter does: their jump does not cost the track its id
    far = without(A, {3, 6}, score=0.25)
    far[3, 0], far[6, 0] = 1e30, 3e38
    back = shifted(far, 1, 0)
    back[3, 0], back[6, 0] = -1e30, -3e38
    add("coordinates_at_1e30", [frame(far, P=P), frame(far, P=P), frame(back, P=P)],
        lambda o, s, r: [int(v) for v in r[2][0, :3]] == [1, 0, 3] and fl(o, 1) == [2] * P and abs(float(o[1][0][0, 3, 0]) - 1e30) < 1e24 and fl(o, 2)[3] == 1 and fl(o, 2)[6] == 1
        and fl(o, 2)[4] == 2 and np.isfinite(o[2][0]).all() and np.isfinite(o[2][1]).all() and bits_of(s[2].pos[0, 3, 0]) == bits_of(-1e30), tcfg=dict(min_score=0.5), beta=1e10)
    return out


def bits_of(x):
    return sr.bits(x)


def _first_velocity(d, dt):
    """e of the FILTER step for a cell at rest (dvh = 0) that moved by d in dt frames, default d_cutoff"""
    F = np.float32
    dt = F(dt)
    dv = F(F(d) / dt)
    rd = F(F(sr.TWO_PI * F(sr.DEFAULTS["d_cutoff"])) * dt)
    ad = F(rd / F(rd + F(1.0)))
    return F(F(ad * dv) + F(F(F(1.0) - ad) * F(0.0)))


def run_ref(case):
    """both restatements over the case; -> (out per frame, a copy of the smoothing state after each frame, records per frame)"""
    ts, ss = tr.State(case["P"]), sr.State(case["P"])
    outs, states, recs = [], [], []
    for joints, num_people in case["frames"]:
        rc = tr.update(ts, joints, num_people, **case["tcfg"])
        outs.append(sr.update(ss, joints, num_people, rc, **case["scfg"]))
        states.append(ss.copy())
        recs.append(np.asarray(rc, np.int64))
    return outs, states, recs


def as_ref(lib_state):
    """the library's SmoothState as a _smoothref.State (for the predicates)"""
    s = sr.State(lib_state.num_parts)
    s.frames = lib_state.frames
    c = lib_state.cell
    s.owner, s.last, s.pos, s.vel, s.score = c["owner"].copy(), c["last"].copy(), c["pos"].copy(), c["vel"].copy(), c["score"].copy()
    return s


def check_predicates(case, outs, states, recs):
    assert len(outs) == len(states) == len(recs) == len(case["frames"])
    assert case["pred"](outs, states, recs), f"{case['name']} does not reach its target: flags of person 0 {[o[2][:1].tolist() for o in outs]}"

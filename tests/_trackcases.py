"""Short joint sequences for tracking mode, one per rule of the definition in include/rtpose_mi355x.h, each with a predicate that says
what the sequence is there to reach.  The inputs are chosen so that tests/_trackref.py alone satisfies every predicate
(check_predicates; tests/test_track_cpu.py runs it on the CPU).

A case: dict(name, P, cfg (keywords of the configuration that differ from the defaults), frames [(joints [people][P][3], num_people
or None = the array's)], pred(recs per frame, state after each frame) -> bool).  Records are compared as unsigned 32-bit values."""
import numpy as np

import _trackref as tr

OX = (0.0, 1.0, 0.25, 0.5, 0.75)
NAN, INF = float("nan"), float("inf")


def body(P, x, y, w=12.0, h=16.0, score=1.0, parts=None):
    """a person whose parts span exactly [x, x + w] x [y, y + h] (w, h multiples of 4: every coordinate is exact); the diagonal squared
    of the default is 144 + 256 = 400.  parts: the scored parts (others get score 0)"""
    j = np.zeros((P, 3), np.float32)
    for p in range(P):
        j[p] = (x + w * OX[p % 5], y + h * OX[(p // 5 + p) % 5], score if parts is None or p in parts else 0.0)
    return j


def shifted(j, dx, dy):
    o = j.copy()
    o[:, 0] += np.float32(dx)
    o[:, 1] += np.float32(dy)
    return o


def frame(*people, P):
    return (np.stack(people).astype(np.float32) if people else np.zeros((0, P, 3), np.float32), None)


def ids(r):
    return [int(x) for x in r[:, 0]]


def u32(v):
    return int(np.uint32(np.int64(v) & 0xFFFFFFFF))


UNTRACKED = [0, u32(-1), 0, 0]


def rec(r, k):
    return [u32(v) for v in r[k]]


def cases(P):
    A, B, Cc = body(P, 100, 100), body(P, 400, 100), body(P, 700, 300)
    out = []

    def add(name, frames, pred, **cfg):
        out.append(dict(name=f"{name}_P{P}", P=P, cfg=cfg, frames=frames, pred=pred))

    # match, birth, death after exactly max_misses + 1 misses
    add("match_birth_death_mm0",
        [frame(A, B, P=P), frame(shifted(A, 1, 0), P=P), frame(shifted(A, 2, 0), Cc, P=P), frame(P=P)],
        lambda r, s: rec(r[0], 0)[:3] == [1, 0, 1] and rec(r[0], 1)[:3] == [2, 1, 1] and rec(r[1], 0)[:3] == [1, 0, 2] and rec(r[1], 0)[3] == tr.bits(1 / 400)
        and s[1].id[1] == 0 and rec(r[2], 0)[:3] == [1, 0, 3] and rec(r[2], 1) == [3, 1, 1, 0] and len(r[3]) == 0 and not s[3].id.any() and not s[3].joints.any()
        and s[3].next_id == 4 and s[3].frames == 4, max_misses=0)
    add("match_birth_death_mm2",
        [frame(A, B, P=P)] + [frame(A, P=P)] * 3 + [frame(A, B, P=P)],
        lambda r, s: s[2].id[1] == 2 and s[2].misses[1] == 2 and s[3].id[1] == 0 and s[3].hits[1] == 0 and s[3].misses[1] == 0 and not s[3].joints[1].any()
        and rec(r[4], 0) == [1, 0, 5, 0] and rec(r[4], 1) == [3, 1, 1, 0], max_misses=2)
    add("freed_slot_reused_in_the_same_frame",
        [frame(A, B, P=P), frame(shifted(B, 0, 1), Cc, P=P)],
        lambda r, s: rec(r[1], 0)[:3] == [2, 1, 2] and rec(r[1], 1) == [3, 0, 1, 0] and tr.bits(s[1].joints[0, 0, 0]) == tr.bits(700.0), max_misses=0)
    crowd = [body(P, 100 * (i % 12), 100 * (i // 12)) for i in range(96)]
    far = [shifted(b, 5000, 0) for b in crowd]
    add("table_full",
        [frame(*crowd, P=P), frame(*far, P=P), frame(*far, P=P)],
        lambda r, s: ids(r[0]) == list(range(1, 97)) and ids(r[1]) == list(range(97, 129)) + [0] * 64 and all(rec(r[1], k) == UNTRACKED for k in range(32, 96))
        and s[1].id.all() and [rec(r[2], k)[:3] for k in range(32)] == [[97 + k, 96 + k, 2] for k in range(32)]
        and [rec(r[2], k) for k in range(32, 96)] == [[129 + k - 32, k - 32, 1, 0] for k in range(32, 96)] and (s[2].id != 0).sum() == 96, max_misses=1)
    # ties: equal cost bits are decided by the slot, then by the person
    add("tie_between_two_people", [frame(A, P=P), frame(shifted(A, 1, 0), shifted(A, -1, 0), P=P)],
        lambda r, s: rec(r[1], 0) == [1, 0, 2, tr.bits(1 / 400)] and rec(r[1], 1) == [2, 1, 1, 0])
    add("tie_between_two_tracks", [frame(A, shifted(A, 2, 0), P=P), frame(shifted(A, 1, 0), P=P)],
        lambda r, s: ids(r[0]) == [1, 2] and rec(r[1], 0) == [1, 0, 2, tr.bits(1 / 400)] and s[1].misses[1] == 1)
    # displacement (3, 4) on every part of a track whose diagonal squared is 400: 25 / 400 = 0.0625 exactly
    add("cost_at_max_cost", [frame(A, P=P), frame(shifted(A, 3, 4), P=P)], lambda r, s: rec(r[1], 0) == [1, 0, 2, tr.bits(0.0625)])
    add("cost_one_ulp_above_max_cost", [frame(A, P=P), frame(shifted(A, 3, 4), P=P)], lambda r, s: rec(r[1], 0) == [2, 1, 1, 0] and s[1].misses[0] == 1,
        max_cost=float(np.nextafter(np.float32(0.0625), np.float32(0))))
    add("common_parts_one_below_min_common",
        [frame(body(P, 100, 100, parts={0, 1, 2, 3}), P=P), frame(body(P, 100, 100, parts={2, 3, 4, 5}), P=P), frame(body(P, 100, 100, parts={0, 1, 2}), P=P)],
        lambda r, s: rec(r[1], 0) == [2, 1, 1, 0] and rec(r[2], 0) == [1, 0, 2, 0] and s[2].hits[0] == 2 and s[2].misses[1] == 1, min_common=3, min_parts=2)
    # scores: a score AT min_score does not count, a NaN score does not count
    at = body(P, 100, 100, score=0.75, parts={0, 1, 2})
    at[3:, 2] = 0.5
    at2 = body(P, 400, 100, score=0.75, parts={0, 1})
    at2[2:, 2] = 0.5
    add("score_at_min_score", [frame(at, at2, P=P), frame(at2, at, P=P)],
        lambda r, s: rec(r[0], 0) == [1, 0, 1, 0] and rec(r[0], 1) == UNTRACKED and rec(r[1], 0) == UNTRACKED and rec(r[1], 1) == [1, 0, 2, 0], min_score=0.5)
    nn = body(P, 100, 100, parts={0, 1, 2})
    nn[3:, 2] = NAN
    nn2 = body(P, 400, 100, parts={0, 1})
    nn2[2:, 2] = NAN
    add("nan_score", [frame(nn, nn2, P=P), frame(shifted(nn, 1, 1), nn2, P=P)],
        lambda r, s: rec(r[0], 1) == UNTRACKED and rec(r[1], 0) == [1, 0, 2, tr.bits(np.float32(2) / np.float32(400))] and rec(r[1], 1) == UNTRACKED)
    # coordinates: an infinite or NaN x or y takes the part out, -0.0 is carried bit for bit
    bad = body(P, 100, 100)
    bad[3, 0], bad[4, 1], bad[5, 0], bad[6, 1] = INF, NAN, NAN, -INF
    add("inf_nan_coordinates", [frame(bad, P=P), frame(shifted(bad, 0, 2), P=P)],
        lambda r, s: rec(r[0], 0) == [1, 0, 1, 0] and rec(r[1], 0) == [1, 0, 2, tr.bits(np.float32(4) / np.float32(400))] and np.isnan(s[1].joints[0, 4, 1]))
    nz = body(P, 0, 0)
    nz[nz[:, 0] == 0, 0] = -0.0
    nz[nz[:, 1] == 0, 1] = -0.0
    add("negative_zero", [frame(nz, P=P), frame(nz, P=P)],
        lambda r, s: rec(r[1], 0) == [1, 0, 2, 0] and tr.bits(s[1].joints[0, 0, 0]) == 0x80000000 and tr.bits(s[1].joints[0, 0, 1]) == 0x80000000)
    # overflow: the sum of squares overflows to infinity, the pair is no candidate
    ov = A.copy()
    ov[2, 0] = 3e38
    add("overflow_in_the_sum", [frame(A, P=P), frame(ov, P=P)], lambda r, s: rec(r[1], 0) == [2, 1, 1, 0] and s[1].misses[0] == 1)
    big = A.copy()
    big[0, 0], big[1, 0] = 3e38, -3e38
    add("overflow_in_the_track_size", [frame(big, P=P), frame(big, P=P), frame(shifted(big, 1, 0), P=P)],
        lambda r, s: rec(r[1], 0) == [1, 0, 2, 0] and rec(r[2], 0) == [1, 0, 3, 0])   # (d = inf: every finite mean divides to 0)
    add("a_frame_with_nobody", [frame(A, P=P), frame(P=P), frame(A, P=P)], lambda r, s: len(r[1]) == 0 and s[1].misses[0] == 1 and rec(r[2], 0) == [1, 0, 2, 0] and s[2].misses[0] == 0)
    add("num_people_out_of_range", [(np.stack(crowd).astype(np.float32), 200), (np.stack(crowd).astype(np.float32), -3), (np.stack(crowd[:2]).astype(np.float32), None)],
        lambda r, s: len(r[0]) == 96 and ids(r[0]) == list(range(1, 97)) and len(r[1]) == 0 and (s[1].misses[:96] == 1).all() and s[1].frames == 2
        and [rec(r[2], k) for k in range(2)] == [[1, 0, 2, 0], [2, 1, 2, 0]])
    return out


def run_ref(case):
    """the restatement over the case; -> (records per frame, a copy of the state after each frame)"""
    st = tr.State(case["P"])
    recs, states = [], []
    for joints, num_people in case["frames"]:
        recs.append(tr.update(st, joints, num_people, **case["cfg"]))
        states.append(st.copy())
    return recs, states


def check_predicates(case, recs, states):
    assert len(recs) == len(states) == len(case["frames"])
    assert case["pred"](recs, states), f"{case['name']} does not reach its target: records {[np.asarray(r).tolist() for r in recs][:4]}"

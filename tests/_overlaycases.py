"""Short joint sequences for overlay mode's update, one per rule of the definition in include/rtpose_mi355x.h, each with a predicate
that says what the sequence is there to reach, and hand-written draw lists for its drawing.  Every sequence runs through the tracker
first (the records are its).  The inputs are chosen so that tests/_trackref.py and tests/_overlayref.py alone satisfy every predicate
(check_predicates; tests/test_overlay_cpu.py runs it on the CPU).

A case: dict(name, P, tcfg / ocfg (keywords of the two configurations that differ from the defaults), next_id (the tracker's first
id), frames [(joints [people][P][3], num_people or None = the array's)], pred(items per frame (lists of 9-tuples), trail state after
each frame, records per frame) -> bool)."""
import copy

import numpy as np

import _overlayref as orf
import _trackcases as tc
import _trackref as tr

NAN, INF = float("nan"), float("inf")
body, shifted, frame = tc.body, tc.shifted, tc.frame
CAPSULE, RECT, LABEL = orf.CAPSULE, orf.RECT, orf.LABEL_KIND
W, H = 160, 96   # the image the sequences are drawn into


def kinds(items):
    return [it[0] for it in items]


def cases(P):
    A, B = body(P, 20, 30), body(P, 100, 40)
    out = []

    def add(name, frames, pred, tcfg=None, next_id=1, **ocfg):
        out.append(dict(name=f"{name}_P{P}", P=P, tcfg=tcfg or {}, ocfg=ocfg, next_id=next_id, frames=frames, pred=pred))

    # born, moved, missed for two frames, rematched, killed; then somebody else takes the slot: a new id, and the trail restarts
    walk = [shifted(A, 3 * i, 2 * i) for i in range(4)]
    add("born_moved_missed_rematched_killed_reborn",
        [frame(walk[0], P=P), frame(walk[1], P=P), frame(P=P), frame(P=P), frame(walk[2], P=P), frame(P=P), frame(P=P), frame(P=P), frame(walk[3], P=P), frame(shifted(walk[3], 2, 0), P=P)],
        lambda it, s, r: kinds(it[0]) == [RECT, LABEL] and kinds(it[1]) == [CAPSULE, RECT, LABEL] and it[2] == [] and s[3].count[0] == 2 and s[3].frames == 4
        and kinds(it[4]) == [CAPSULE, CAPSULE, RECT, LABEL] and it[4][0][1:5] == (26, 38, 29, 40) and it[4][1][1:5] == (29, 40, 32, 42) and int(r[4][0, 0]) == 1
        and int(r[8][0, 0]) == 2 and int(r[8][0, 1]) == 0 and kinds(it[8]) == [RECT, LABEL] and s[8].owner[0] == 2 and s[8].count[0] == 1 and s[8].head[0] == 1
        and it[8][1][8] == 2 and kinds(it[9]) == [CAPSULE, RECT, LABEL] and it[9][0][6] == orf.PALETTE[2] and it[4][0][6] == orf.PALETTE[1],
        tcfg=dict(max_misses=2), trail_len=8)
    # the ring: 40 steps with every trail_len; with 32 the ring wraps and the oldest kept point is 31 steps back
    steps = [frame(shifted(A, 2 * i, i % 3), P=P) for i in range(40)]
    for L in (0, 1, 2, 32):
        add(f"trail_len_{L}", steps,
            lambda it, s, r, L=L: all(kinds(it[i]).count(CAPSULE) == max(min(i + 1, L) - 1, 0) for i in range(40)) and s[39].count[0] == L and s[39].head[0] == 40 % 32
            and (L < 2 or (it[39][0][1] == 26 + 2 * (39 - (L - 1)) and it[39][L - 2][3] == 26 + 2 * 39 and [x[7] for x in it[39][:L - 1]] == [192 * (j + 1) // (L - 1) for j in range(L - 1)])),
            trail_len=L)
    # a person the tracker does not track (two parts: id 0), one it tracks but none of whose parts counts for the overlay, and one drawn
    few = body(P, 60, 10, parts={1, 4})
    dim = body(P, 100, 40, score=0.5)
    add("untracked_and_no_counting_part", [frame(few, dim, A, P=P), frame(few, dim, shifted(A, 1, 1), P=P)],
        lambda it, s, r: [int(v) for v in r[1][:, 0]] == [0, 1, 2] and kinds(it[1]) == [CAPSULE, RECT, LABEL] and it[1][2][8] == 2 and s[1].owner[0] == 0 and s[1].owner[1] == 2
        and s[1].count[0] == 0, min_score=0.75)
    crowd = np.stack([body(P, 13 * (i % 12), 11 * (i // 12), w=8.0, h=8.0) for i in range(96)]).astype(np.float32)
    add("num_people_out_of_range", [(crowd, 200), (crowd, -3), (crowd[:2].copy(), None)],
        lambda it, s, r: kinds(it[0]) == [RECT, LABEL] * 96 and it[1] == [] and s[1].frames == 2 and kinds(it[2]) == [CAPSULE, RECT, LABEL] * 2 and (s[2].count[:96] == [2, 2] + [1] * 94).all(),
        tcfg=dict(max_cost=0.01))
    # coordinates that are not numbers, and numbers far outside every image: the first are not counted, the second are clamped
    bad = body(P, 40, 40)
    bad[3, 0], bad[4, 1], bad[5, 0], bad[6, 1], bad[8, 2] = INF, NAN, NAN, -INF, NAN
    huge = body(P, 40, 40)
    huge[0, 0], huge[1, 1], huge[2, 0] = 1e30, -3e38, 40000.0
    add("nan_inf_and_huge_coordinates", [frame(bad, P=P), frame(huge, P=P)],
        lambda it, s, r: it[0][0][1:5] == (36, 36, 56, 60) and it[1][-2][0] == RECT and it[1][-2][1:5] == (36, -32771, 32771, 60) and it[1][-1][1:3] == (36, -32771)
        and all(abs(v) <= 32767 + 4 + 70 for x in it[1] for v in x[1:5]))
    # the ids a label has to print: 9 -> 10 (one more digit), the largest positive id and the one after it (negative as an int), and
    # the one after the counter's wrap
    two = [frame(A, P=P), frame(A, B, P=P)]
    add("ids_9_and_10", two, lambda it, s, r: it[1][2][8] == 9 and it[1][2][3] - it[1][2][1] + 1 == 7 and it[1][4][8] == 10 and it[1][4][3] - it[1][4][1] + 1 == 13
        and it[1][3][6] == orf.PALETTE[10], next_id=9)
    add("ids_2147483647_and_the_next", two, lambda it, s, r: it[1][2][8] == 2147483647 and it[1][4][8] == -2147483648 and it[1][4][6] == orf.PALETTE[0]
        and it[1][4][3] - it[1][4][1] + 1 == 61 * 2 and it[1][4][4] - it[1][4][2] + 1 == 18, next_id=2147483647, label_scale=2)
    add("ids_across_the_wrap", two, lambda it, s, r: it[1][2][8] == -1 and it[1][2][3] - it[1][2][1] + 1 == 61 and it[1][2][6] == orf.PALETTE[15] and it[1][4][8] == 1,
        next_id=0xFFFFFFFF)
    # a label that would leave the image's top goes inside the box
    top = body(P, 30, 6)
    add("label_inside_at_the_top", [frame(top, P=P), frame(shifted(top, 0, 8), P=P)],
        lambda it, s, r: it[0][0][2] == 2 and it[0][1][2] == 2 and it[1][-2][2] == 10 and it[1][-1][2] == 1, what=orf.BOX | orf.LABEL | orf.TRAIL)
    for what in range(1, 8):
        add(f"what_{what}", [frame(A, B, P=P), frame(shifted(A, 2, 1), shifted(B, -2, 1), P=P), frame(shifted(A, 4, 2), shifted(B, -4, 2), P=P)],
            lambda it, s, r, what=what: kinds(it[2]) == ([CAPSULE] * 2 * bool(what & 4) + [RECT] * bool(what & 1) + [LABEL] * bool(what & 2)) * 2 and s[2].count[0] == 3,
            what=what, alpha=128 if what & 1 else 256, line_width=3, trail_radius=what % 3)
    return out


def run_ref(case):
    """both restatements over the case -> (items per frame, a copy of the trail state after each frame, records per frame)"""
    ts, st = tr.State(case["P"]), orf.State(case["P"])
    ts.next_id = case["next_id"]
    items, states, recs = [], [], []
    for joints, num_people in case["frames"]:
        rc = tr.update(ts, joints, num_people, **case["tcfg"])
        items.append(orf.update(st, joints, _people(joints, num_people), rc, **case["ocfg"]))
        states.append(copy.deepcopy(st))
        recs.append(np.asarray(rc, np.int64))
    return items, states, recs


def _people(joints, num_people):
    return len(joints) if num_people is None else num_people


def as_ref(lib_state):
    """the library's TrailState as an _overlayref.State (for the predicates)"""
    s = orf.State(lib_state.num_parts)
    s.frames = lib_state.frames
    for name in ("owner", "count", "head", "pts"):
        setattr(s, name, lib_state.slot[name].astype(np.int64))
    return s


def as_tuples(items):
    return [tuple(int(v) for v in it) for it in np.asarray(items).reshape(-1, orf.ITEM_INTS)]


def check_predicates(case, items, states, recs):
    assert len(items) == len(states) == len(recs) == len(case["frames"])
    assert case["pred"](items, states, recs), f"{case['name']} does not reach its target: items {items[-1]}, records {recs[-1].tolist()}"


def background(w=W, h=H, seed=7):
    """an image with every byte value somewhere, so that a wrong blend shows"""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def draw_lists(w=W, h=H):
    """hand-written draw lists for a w x h image -> [(name, items)]: alpha 0 / 128 / 256, items wholly outside, straddling each border
    and at negative coordinates, a zero-length capsule, radius 0, an outline wider than its box, every label scale, kinds that do not
    exist and fields out of their range"""
    c = orf.PALETTE
    L = []
    for a in (0, 128, 256):
        L.append((f"alpha_{a}", [(RECT, 10, 10, 60, 50, 3, c[0], a, 0), (CAPSULE, 20, 60, 90, 20, 4, c[1], a, 0), (LABEL, 70, 5, 70 + 19 * 2 - 1, 5 + 17, 2, c[2], a, 123)]))
    L.append(("wholly_outside", [(RECT, w, 0, w + 20, 20, 2, c[3], 256, 0), (RECT, -30, -30, -1, -1, 2, c[3], 256, 0), (CAPSULE, -40, -40, -10, -10, 5, c[4], 256, 0),
                                 (CAPSULE, 0, h + 17, w, h + 17, 16, c[4], 256, 0), (LABEL, 10, h, 22, h + 8, 1, c[5], 256, 42), (LABEL, -13, 0, -1, 8, 1, c[5], 256, 42)]))
    L.append(("straddling_every_border", [(RECT, -10, -10, 15, 12, 4, c[6], 200, 0), (RECT, w - 12, h - 9, w + 30, h + 30, 5, c[7], 200, 0), (CAPSULE, -20, 40, 30, 70, 6, c[8], 200, 0),
                                          (CAPSULE, w - 10, 10, w + 40, -20, 3, c[9], 200, 0), (CAPSULE, 50, h - 3, 90, h + 25, 7, c[10], 200, 0), (LABEL, -8, 30, -8 + 37 - 1, 38, 1, c[11], 256, 654321),
                                          (LABEL, w - 20, -10, w - 20 + 3 * 13 - 1, -10 + 26, 3, c[12], 256, 77), (LABEL, 60, h - 5, 72, h + 3, 1, c[13], 256, 8)]))
    L.append(("zero_length_capsule_and_radius_0", [(CAPSULE, 40, 40, 40, 40, 9, c[14], 256, 0), (CAPSULE, 80, 40, 80, 40, 0, c[15], 256, 0), (CAPSULE, 5, 5, 150, 90, 0, c[0], 256, 0),
                                                    (CAPSULE, 100, 80, 100, 10, 0, c[1], 160, 0), (CAPSULE, 10, 70, 70, 70, 1, c[2], 160, 0)]))
    L.append(("outline_wider_than_its_box", [(RECT, 20, 20, 30, 26, 16, c[3], 256, 0), (RECT, 50, 20, 50, 20, 1, c[4], 256, 0), (RECT, 60, 20, 72, 33, 6, c[5], 100, 0), (RECT, 90, 40, 80, 30, 2, c[6], 256, 0)]))
    L.append(("every_label_scale", [(LABEL, 2 + 3 * s, 11 * s - 9, 2 + 3 * s + 13 * s - 1, 11 * s - 9 + 9 * s - 1, s, c[s], 256, 10 * s + 9 - s) for s in range(1, 9)]))
    L.append(("all_ten_digits", [(LABEL, 5, 5, 5 + 61 - 1, 13, 1, c[7], 256, 1234567890), (LABEL, 5, 20, 5 + 61 * 2 - 1, 37, 2, c[8], 256, -1), (LABEL, 5, 45, 5 + 61 - 1, 53, 1, c[0], 256, -2147483648)]))
    L.append(("unknown_kinds_and_fields_out_of_range", [(0, 10, 10, 50, 50, 2, c[9], 256, 0), (4, 10, 10, 50, 50, 2, c[9], 256, 0), (-1, 0, 0, w, h, 2, c[9], 256, 0),
                                                         (RECT, 10, 10, 50, 50, 40, c[10], 999, 0), (RECT, 60, 10, 90, 50, -3, c[10], 256, 0), (CAPSULE, 20, 80, 120, 60, 99, c[11], -5, 0),
                                                         (CAPSULE, 20, 80, 120, 60, 99, c[11], 90, 0), (LABEL, 100, 60, 130, 90, 0, c[12], 256, 5), (LABEL, 100, 10, 159, 50, 77, c[13], 256, 3),
                                                         (RECT, -2147483648, -2147483648, 2147483647, 2147483647, 3, c[14], 128, 0), (CAPSULE, -2147483648, 5, 2147483647, 5, 2, c[15], 128, 0),
                                                         (CAPSULE, -65535, -65535, 65535, 65535, 16, c[1], 77, 0)]))
    return L


def overlapping(order):
    """two half-transparent items that overlap, in either order"""
    a, b = (RECT, 20, 20, 60, 60, 16, orf.PALETTE[0], 128, 0), (CAPSULE, 30, 30, 90, 50, 8, orf.PALETTE[1], 128, 0)
    return [a, b] if order == 0 else [b, a]

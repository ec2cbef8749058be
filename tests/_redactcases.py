"""Joint sets for redaction mode's regions, one per rule of the definition in include/rtpose_mi355x.h, each with a predicate that says
what the set is there to reach.  The inputs are chosen so that tests/_redactref.py alone satisfies every predicate (check_predicates;
tests/test_redact_cpu.py runs it on the CPU).

A case: dict(name, P, cfg (keywords of the configuration that differ from the defaults), joints [people][P][3], num_people (or None =
the array's), pred(records: list of 6-tuples) -> bool).  The records are applied to background(W, H)."""
import numpy as np

import _redactref as rr

NAN, INF = float("nan"), float("inf")
W, H = 160, 96   # the image the regions are applied to


def background(w=W, h=H, seed=5):
    """noise over a gradient: every blur window and every mosaic cell has its own mean"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 3) % 256], axis=2).astype(np.int64)
    return ((img + rng.integers(0, 96, (h, w, 3))) % 256).astype(np.uint8)


def head(P, x, y, span=8.0, score=1.0, only=None):
    """a person whose head parts span `span` pixels around (x, y); a scored shoulder far away shows that unlisted parts do not count.
    only: the indices INTO the head list that are scored (None = all)."""
    j = np.zeros((P, 3), np.float32)
    if P == 18:
        pts = {0: (x, y), 14: (x - span / 4, y - span / 4), 15: (x + span / 4, y - span / 4), 16: (x - span / 2, y), 17: (x + span / 2, y)}
    else:
        pts = {0: (x, y - span / 2), 1: (x, y + span / 2)}
    for i, (p, (px, py)) in enumerate(pts.items()):
        if only is None or i in only:
            j[p] = (px, py, score)
    j[5] = (x + 300.0, y + 300.0, 1.0)
    return j


def people(*persons, P=18):
    return np.stack(persons).astype(np.float32) if persons else np.zeros((0, P, 3), np.float32)


def cases(P):
    out = []
    nhead = len(rr.HEAD_PARTS[P])

    def add(name, joints, pred, num_people=None, **cfg):
        out.append(dict(name=f"{name}_P{P}", P=P, cfg=cfg, joints=joints, num_people=num_people, pred=pred))

    # span 8: x1 - x0 = 8 (COCO, ear to ear) or y1 - y0 = 8 (MPI, head to neck): s = 9, rx = ((9 * 384) >> 9) + 2 = 8, ry = (8 * 320) >> 8 = 10
    add("inside", people(head(P, 40, 30), head(P, 120, 60, span=16), P=P),
        lambda r: r[0] == ((40, 30 - (P == 18), 8, 10, nhead, 1) if P == 18 else (40, 30, 8, 10, nhead, 1)) and r[1][2:] == (14, 17, nhead, 1))
    # across each edge; the first one's centre has a negative, odd coordinate sum: floor, not truncation
    add("crossing_each_edge", people(head(P, -3.5 if P == 18 else -3, 40 if P == 18 else -3, span=3 if P == 18 else 5), head(P, 158, 40), head(P, 80, 1), head(P, 80, 95), P=P),
        lambda r: all(x[5] == 1 for x in r) and (r[0][0] == -4 if P == 18 else r[0][1] == -3) and r[0][0] + r[0][2] >= 0 and r[1][0] + r[1][2] > W - 1 and r[2][1] - r[2][3] < 0 and r[3][1] + r[3][3] > H - 1)
    add("wholly_outside", people(head(P, -100, -100), head(P, 400, 300), head(P, 80, -40), P=P), lambda r: all(x[5] == 1 for x in r) and r[0][0] + r[0][2] < 0 and r[1][0] - r[1][2] >= W)
    # one counting part: s = 1, rx = 0 + pad = 2, and min_radius 4 decides; with min_radius 0 the pad does
    add("one_counting_part", people(head(P, 50, 50, only={0}), P=P), lambda r: r[0][2:] == (4, 5, 1, 1))
    add("one_counting_part_min_radius_0", people(head(P, 50, 50, only={0}), P=P), lambda r: r[0][2:] == (2, 2, 1, 1), min_radius=0)
    add("none_counting", people(head(P, 50, 50, only=set()), head(P, 90, 50, score=0.25), P=P), lambda r: r == [(0, 0, 0, 0, 0, 0)] * 2, min_score=0.25)
    add("below_min_parts", people(head(P, 50, 50, only={0}), head(P, 90, 50), P=P), lambda r: r[0] == (0, 0, 0, 0, 1, 0) and r[1][4:] == (nhead, 1), min_parts=2)
    # coordinates and scores that are not numbers do not count; what is left spans the region
    bad = head(P, 60, 40)
    lst = rr.HEAD_PARTS[P]
    bad[lst[0], 0] = NAN
    bad[lst[1], 2] = NAN
    if P == 18:
        bad[lst[2], 1], bad[lst[3], 0] = -INF, INF
    add("nan_inf_coordinates_and_a_nan_score", people(bad, P=P), lambda r: r[0][4:] == ((1, 1) if P == 18 else (0, 0)) and (P == 15 or r[0][:2] == (64, 40)))
    huge = head(P, 60, 40)
    huge[lst[0], 0], huge[lst[1], 1] = 1e30, -3e38
    add("coordinates_beyond_32767", people(huge, P=P), lambda r: r[0][5] == 1 and r[0][2] == rr.MAX_RADIUS and r[0][3] == rr.MAX_RADIUS and abs(r[0][0]) <= 32767 and abs(r[0][1]) <= 32767)
    add("two_overlapping", people(head(P, 60, 40, span=16), head(P, 72, 46, span=16), P=P), lambda r: abs(r[0][0] - r[1][0]) < r[0][2] + r[1][2])
    add("three_overlapping", people(head(P, 60, 40, span=16), head(P, 72, 46, span=16), head(P, 66, 30, span=12), P=P), lambda r: len(r) == 3 and all(x[5] for x in r))
    crowd = people(*[head(P, 8 + 13 * (i % 12), 6 + 11 * (i // 12), span=4 + i % 5) for i in range(96)], P=P)
    add("96_people", crowd, lambda r: len(r) == 96 and all(x[5] for x in r))
    add("num_people_minus_1", crowd, lambda r: r == [], num_people=-1)
    add("num_people_0", crowd, lambda r: r == [], num_people=0)
    add("num_people_200", crowd, lambda r: len(r) == 96, num_people=200)
    # radii of zero: the centre pixel, the centre row, the centre column
    add("rx_and_ry_0", people(head(P, 50, 50, only={0}), P=P), lambda r: r[0][2:4] == (0, 0), min_radius=0, pad=0, scale_q8=64)
    add("ry_0", people(head(P, 50, 50, only={0}), P=P), lambda r: r[0][2:4] == (3, 0), min_radius=0, pad=3, aspect_q8=64)
    add("rx_0_ry_0_ellipse_row", people(head(P, 50, 50, only={0}), P=P), lambda r: r[0][2:4] == (1, 4), min_radius=0, pad=1, aspect_q8=1024)
    # s = 17: (17 * 64) >> 9 = 2 and (17 * 4096) >> 9 = 136; rx = 4: (4 * 64) >> 8 = 1 and (4 * 1024) >> 8 = 16
    add("scale_q8_64", people(head(P, 80, 48, span=16), P=P), lambda r: r[0][2] == 2, scale_q8=64, pad=0, min_radius=0)
    add("scale_q8_4096", people(head(P, 80, 48, span=16), P=P), lambda r: r[0][2] == 136, scale_q8=4096, pad=0, min_radius=0)
    add("aspect_q8_64", people(head(P, 80, 48, only={0}), P=P), lambda r: r[0][2:4] == (4, 1), aspect_q8=64)
    add("aspect_q8_1024", people(head(P, 80, 48, only={0}), P=P), lambda r: r[0][2:4] == (4, 16), aspect_q8=1024)
    add("as_large_as_the_clamp", people(head(P, 80, 48, span=3000), P=P), lambda r: r[0][2:4] == (rr.MAX_RADIUS, rr.MAX_RADIUS), scale_q8=4096, aspect_q8=1024)
    return out


def check_predicates(case, regs):
    assert case["pred"]([tuple(int(v) for v in r) for r in regs]), f"{case['name']}: the predicate fails on {[tuple(int(v) for v in r) for r in regs][:6]}"


def run_ref(case):
    return rr.regions(case["joints"], case["num_people"], case["P"], rr.config(**case["cfg"]))

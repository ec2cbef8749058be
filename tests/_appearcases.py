"""Inputs for appearance-aided tracking, one per rule of the definition in include/rtpose_mi355x.h, each with a predicate that says what
the input is there to reach.  They are chosen so that tests/_appearref.py alone satisfies every predicate (tests/test_appearance_cpu.py
runs that on the CPU).

A describe case: dict(name, P, image [h][w][3] u8 BGR, joints [people][P][3], cfg (keywords that differ from the defaults),
pred(bins, valid) -> bool).
An update case: dict(name, P, cfg, track (keywords of the tracking configuration), frames [(joints, num_people or None, image or None =
a frame without a display image)], pred(recs per frame, track state after each frame, appearance state after each frame, (bins, valid)
per frame) -> bool).  Update images are W x H = 160 x 96, the display size of the GPU tests' engines."""
import numpy as np

import _appearref as ar
import _trackcases as tc
import _trackref as tr

W, H = 160, 96
NAN, INF = float("nan"), float("inf")
RED, BLUE, GREEN, GREY = (0, 0, 255), (255, 0, 0), (0, 255, 0), (128, 128, 128)   # BGR
rec, ids = tc.rec, tc.ids


def code(bgr, lower=False):
    """the bin of a colour in the upper (or lower) half"""
    b, g, r = bgr
    return (64 if lower else 0) + (r >> 6) * 16 + (g >> 6) * 4 + (b >> 6)


def canvas(w=W, h=H, colour=GREY):
    img = np.zeros((h, w, 3), np.uint8)
    img[:] = colour
    return img


def paint(img, x, y, colour, w=14, h=20):
    """the clothing of tc.body(P, x, y): a rectangle that covers the body's extent"""
    img[max(y - 1, 0):y - 1 + h, max(x - 1, 0):x - 1 + w] = colour
    return img


def scene(P, *people):
    """people: (x, y, colour or None = unpainted, joints or None = tc.body) -> (joints [n][P][3], image)"""
    img = canvas()
    js = []
    for x, y, colour, j in people:
        if colour is not None:
            paint(img, x, y, colour)
        js.append(tc.body(P, x, y) if j is None else j)
    return (np.stack(js).astype(np.float32) if js else np.zeros((0, P, 3), np.float32)), img


def torsoless(P, x, y):
    """tc.body with the scores of the torso parts at 0: trackable, but without a descriptor"""
    j = tc.body(P, x, y)
    j[ar.TORSO[P], 2] = 0.0
    return j


def describe_cases(P=18):
    out = []

    def add(name, image, joints, pred, **cfg):
        out.append(dict(name=f"{name}_P{P}", P=P, image=image, joints=np.asarray(joints, np.float32).reshape(-1, P, 3), cfg=cfg, pred=pred))

    rng = np.random.default_rng(17)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    inside = np.stack([tc.body(P, 20, 20), tc.body(P, 100, 50, w=40.0, h=32.0)])
    add("random_image", noise, inside, lambda b, v: v.tolist() == [1, 1] and (b.sum(1) == 1024).all() and (b[:, :64].sum(1) == 512).all())
    add("margin", noise, inside, lambda b, v: v.all() and (b.sum(1) == 1024).all(), margin=0.25)
    partly = np.stack([tc.body(P, -6, -8), tc.body(P, W - 6, H - 8), tc.body(P, -200, 40), tc.body(P, 40, 4000)])
    # (wholly outside: the border is replicated, so every sample of a grid row, or of a grid column, reads the same pixel)
    add("partly_and_wholly_outside", noise, partly, lambda b, v: v.all() and (b.sum(1) == 1024).all() and (b[2] % 32 == 0).all() and (b[3] % 16 == 0).all())
    one = tc.body(P, 30.5, 30.5, w=0.0, h=0.0)    # w = h = fmaxf(0, 1) = 1, left = top = 30: every sample reads pixel (30, 30)
    add("box_of_one_pixel", noise, one, lambda b, v: v.tolist() == [1] and b[0, :64].max() == 512 and b[0, 64:].max() == 512)
    wide = tc.body(P, 0, 40)
    wide[1, 0], wide[5, 0] = 524288.0, -524288.0   # x1 - x0 = 2^20 exactly: |left| = |right| = 2^19, a step of 2^31 in Q16
    add("box_2_pow_20_wide", noise, wide, lambda b, v: v.tolist() == [1] and b[0].sum() == 1024)
    wider = wide.copy()
    wider[1, 0] = 1048576.0 + 1.0
    wider[5, 0] = -1048576.0
    add("box_beyond_the_bound", noise, wider, lambda b, v: v.tolist() == [0] and not b.any())
    bad = np.stack([tc.body(P, 20, 20)] * 3)
    T = ar.TORSO[P]
    bad[0, T[0], 0], bad[0, T[1], 1] = NAN, INF     # two torso parts out: 3 or 4 left, still a descriptor
    for i, p in enumerate(T[:-2]):                   # all but two out: no descriptor
        bad[1, p, i % 2] = (NAN, -INF, INF)[i % 3]
    bad[2, :, 2] = NAN                               # a NaN score never counts
    add("nan_inf_joints", noise, bad, lambda b, v: v.tolist() == [1, 0, 0] and b[0].sum() == 1024 and not b[1:].any())
    huge = tc.body(P, 20, 20)
    huge[1, 0], huge[5, 0] = 3e38, -3e38            # the width overflows to infinity
    add("overflow_in_the_box", noise, huge, lambda b, v: v.tolist() == [0] and not b.any())
    few = np.stack([tc.body(P, 20, 20, parts={1, 2, 5, 8}), tc.body(P, 20, 20, parts={1, 2, 5})])
    add("count_below_min_parts", noise, few, lambda b, v: v.tolist() == [1, 0] and not b[1].any(), min_parts=4)
    add("score_at_min_score", noise, np.stack([tc.body(P, 20, 20, score=0.5), tc.body(P, 20, 20, score=0.75)]), lambda b, v: v.tolist() == [0, 1], min_score=0.5)
    add("image_of_one_pixel", np.array([[[10, 200, 130]]], np.uint8), inside,
        lambda b, v: v.all() and b[0, code((10, 200, 130))] == 512 and b[0, code((10, 200, 130), True)] == 512 and (b[0] > 0).sum() == 2)
    rep = tc.body(P, 20, 20, parts={1, 2})
    add("repeated_list_entry", noise, np.stack([rep, rep]), lambda b, v: v.tolist() == [1, 1] and b[0].sum() == 1024, parts=[1, 1, 2], min_parts=3)
    add("repeated_entry_counts_per_repeat", noise, rep, lambda b, v: v.tolist() == [0], parts=[1, 1, 2], min_parts=4)
    add("all_parts_listed", noise, inside, lambda b, v: v.all(), parts=list(range(P)))
    add("single_bin", canvas(colour=RED), tc.body(P, 40, 0, w=64.0, h=0.0), lambda b, v: v.tolist() == [1] and b[0, code(RED)] == 512 and b[0, code(RED, True)] == 512)
    # a box of exactly 32 x 32 pixels at an integer position samples each pixel once; each half (16 rows x 32 columns = 512 samples)
    # holds each of the 64 colours 8 times
    every = canvas()
    for jj in range(32):
        for ii in range(32):
            c = ((jj % 16) * 32 + ii) % 64
            every[10 + jj, 50 + ii] = ((c & 3) << 6, ((c >> 2) & 3) << 6, (c >> 4) << 6)
    full = tc.body(P, 50, 10, w=32.0, h=32.0)
    full[:, 2] = 0.0
    full[[1, 2, 5], 2] = 1.0
    full[1, :2], full[2, :2], full[5, :2] = (50, 10), (82, 42), (66, 20)
    add("all_128_bins", every, full, lambda b, v: v.tolist() == [1] and (b[0] == 8).all())
    return out


def update_cases(P=18):
    out = []

    def add(name, frames, pred, track=None, **cfg):
        out.append(dict(name=f"{name}_P{P}", P=P, cfg=cfg, track=track or {}, frames=frames, pred=pred))

    def fr(*people):
        j, img = scene(P, *people)
        return (j, None, img)

    def blend(d, b, rate):
        return ((d.astype(np.int64) * (256 - rate) + 16 * b.astype(np.int64) * rate + 128) >> 8).astype(np.uint16)

    for rate in (1, 128, 256):
        add(f"rate_{rate}", [fr((20, 20, RED, None)), fr((20, 20, BLUE, None)), fr((20, 20, BLUE, None))],
            lambda r, ts, ap, d, rate=rate: ids(r[2]) == [1] and ap[0].owner[0] == 1 and np.array_equal(ap[0].desc[0], 16 * d[0][0][0])
            and np.array_equal(ap[1].desc[0], blend(ap[0].desc[0], d[1][0][0], rate)) and np.array_equal(ap[2].desc[0], blend(ap[1].desc[0], d[2][0][0], rate))
            and (rate == 256) == np.array_equal(ap[1].desc[0], 16 * d[1][0][0]) and rec(r[1], 0)[3] == tr.bits(np.float32(0.125)), rate=rate, weight=0.125)
    add("owner_is_a_dead_id", [fr((20, 20, RED, None)), fr(), fr((20, 20, GREEN, None))],
        lambda r, ts, ap, d: ts[1].id[0] == 0 and ap[1].owner[0] == 1 and rec(r[2], 0) == [2, 0, 1, 0] and ap[2].owner[0] == 2
        and np.array_equal(ap[2].desc[0], 16 * d[2][0][0]) and ap[2].desc[0, code(GREEN)] == 8192, track=dict(max_misses=0))
    # born without a descriptor, matched by a person with one (unknown: the track's side), then by one without (unknown: the person's side)
    add("unknown_on_either_side", [fr((20, 20, RED, torsoless(P, 20, 20))), fr((20, 20, RED, None)), fr((20, 20, BLUE, torsoless(P, 20, 20))), fr((20, 20, RED, None))],
        lambda r, ts, ap, d: d[0][1].tolist() == [0] and rec(r[0], 0) == [1, 0, 1, 0] and ap[0].owner[0] == 0 and not ap[0].desc.any()
        and rec(r[1], 0) == [1, 0, 2, tr.bits(np.float32(0.5) * np.float32(0.75))] and ap[1].owner[0] == 1 and np.array_equal(ap[1].desc[0], 16 * d[1][0][0])
        and rec(r[2], 0) == [1, 0, 3, tr.bits(np.float32(0.5) * np.float32(0.75))] and np.array_equal(ap[2].desc, ap[1].desc) and rec(r[3], 0) == [1, 0, 4, 0],
        weight=0.5, unknown=0.75, max_dist=0.25)
    # the gate: the same place in other clothing is a birth (a = 1 > max_dist), while unknown = 1 above passes it ungated
    add("max_dist_turns_a_match_into_a_birth", [fr((20, 20, RED, None)), fr((20, 20, BLUE, None))],
        lambda r, ts, ap, d: rec(r[1], 0) == [2, 1, 1, 0] and ts[1].misses[0] == 1 and ap[1].owner[:2].tolist() == [1, 2] and np.array_equal(ap[1].desc[0], ap[0].desc[0]),
        max_dist=0.5)
    add("distance_at_max_dist_passes", [fr((20, 20, RED, None)), fr((20, 20, BLUE, None))],
        lambda r, ts, ap, d: rec(r[1], 0) == [1, 0, 2, tr.bits(np.float32(0.125))], max_dist=1.0, rate=256)
    j2, img2 = scene(P, (20, 20, RED, None), (80, 40, BLUE, None))
    add("a_frame_without_a_display_image", [(j2, None, img2), (j2, None, None), (j2, None, img2)],
        lambda r, ts, ap, d: d[1][0] is None and ids(r[1]) == [1, 2] and rec(r[1], 0)[3] == tr.bits(np.float32(0.125) * np.float32(0.25))
        and np.array_equal(ap[1].desc, ap[0].desc) and rec(r[2], 1) == [2, 1, 3, 0])
    out.append(crossing(P))
    return out


# THE CROSSING.  Two people 20 pixels apart, in red and in blue, have swapped places in the next frame.  A body spans 12 x 16 pixels:
# the track's squared diagonal is 400, so keeping the ids costs 20 * 20 / 400 = 1.0 per pair and swapping them costs 0.  max_cost = 2.0
# lets both kinds of pair through the motion gate.  The motion cost alone (rtp_track_update) takes the two zero-cost pairs: the ids swap.
# With the descriptors, the wrong pairs are red against blue: L = 32768, a = 1, total = 0 + weight; the right pairs are a = 0, total = 1.0.
# weight = 4.0 puts the wrong pairs (4.0) behind the right ones (1.0): the ids stay.
CROSSING = dict(distance=20, max_cost=2.0, weight=4.0)


def crossing(P):
    x0, x1, y = 50, 50 + CROSSING["distance"], 40
    f0 = scene(P, (x0, y, RED, None), (x1, y, BLUE, None))
    f1 = scene(P, (x1, y, RED, None), (x0, y, BLUE, None))   # person 0 is still the one in red
    return dict(name=f"crossing_P{P}", P=P, cfg=dict(weight=CROSSING["weight"]), track=dict(max_cost=CROSSING["max_cost"]),
                frames=[(f0[0], None, f0[1]), (f1[0], None, f1[1])],
                pred=lambda r, ts, ap, d: ids(r[0]) == [1, 2] and rec(r[1], 0) == [1, 0, 2, tr.bits(1.0)] and rec(r[1], 1) == [2, 1, 2, tr.bits(1.0)])


def run_ref(case):
    """the restatement over an update case; -> (records, track states, appearance states, (bins, valid)) per frame"""
    ts, ap = tr.State(case["P"]), ar.State()
    recs, tss, aps, descs = [], [], [], []
    for joints, num_people, image in case["frames"]:
        b, v = ar.describe(image, joints, case["P"], **case["cfg"]) if image is not None else (None, None)
        recs.append(ar.update(ts, ap, joints, num_people, b, v, track=case["track"], **case["cfg"]))
        tss.append(ts.copy())
        aps.append(ap.copy())
        descs.append((b, v))
    return recs, tss, aps, descs


def check_predicates(case, *result):
    assert case["pred"](*result), f"{case['name']} does not reach its target: records {[np.asarray(r).tolist() for r in result[0]][:4]}"

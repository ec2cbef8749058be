"""Post-processing kernels off their built-in sizes — TEST INFRASTRUCTURE of tests/test_postproc_sizes.py (GPU) and tests/test_postproc_sizes_cpu.py.

plan.cpp takes any nms_param max_peaks in [1, 127] from the deploy prototxt and rtp_set_thresholds takes any thresholds, but the built-in
graphs only ever run max_peaks 64 (COCO) and 20 (MPI) at the reference's default thresholds.  Here: the matrix of engines (a built-in
prototxt with its `max_peaks:` line rewritten), the inputs, the threshold sets, the oracle results of every (engine, input, threshold set) and
Python restatements of the conditions under which csrc/postproc.hip takes the branches B1..B10 that the built-in sizes never take.  The CPU
file asserts that the matrix reaches each of them; the GPU file compares the kernels with the oracle on exactly this matrix, bit for bit.

Thresholds outside the reference's arithmetic: connect_inter_min_above_threshold < 0 accepts a pair with count == 0, whose score is 0 / 0; the
reference then hands NaNs to std::sort, which is undefined.  rtp_set_thresholds refuses it (RTP_EINVAL; tested in the GPU file) and no set
below has it.  inter_min_above >= 10 is defined (no pair can have more than 10 samples above the threshold: no connection at all) and is in.

All inputs live at net 320x176 (low-res 40x22): the smallest net at which a white-noise map still has more than 127 maxima in every part."""
import atexit
import functools
import os
import shutil
import tempfile
from collections import OrderedDict

import numpy as np

import _oracle as orc
import _synth

NET_W, NET_H = 320, 176
LOW_W, LOW_H = NET_W // 8, NET_H // 8
MAX_PEOPLE = 96

# ---- engines: name -> (model, max_peaks, (disp_w, disp_h), num_scales, scale_gap).  63 / 65, 90 / 91 and 120 / 121 sit on either side of the
# second occupancy word, of the 64 KiB of sort keys and of the assemble kernel's LDS copy; emission scales by disp / net.
ENGINES = OrderedDict([
    ("coco1", (0, 1, (1280, 720), 1, 0.3)),
    ("coco2", (0, 2, (1280, 720), 1, 0.3)),
    ("coco63", (0, 63, (1280, 720), 1, 0.3)),
    ("coco65", (0, 65, (333, 201), 1, 0.3)),
    ("coco90", (0, 90, (1280, 720), 1, 0.3)),
    ("coco91", (0, 91, (1280, 720), 1, 0.3)),
    ("coco120", (0, 120, (1280, 720), 1, 0.3)),
    ("coco121", (0, 121, (1920, 1080), 1, 0.3)),
    ("coco127", (0, 127, (1280, 720), 1, 0.3)),
    ("coco127x3", (0, 127, (1280, 720), 3, 0.15)),   # the multi-scale pair kernel; the NMS column skip is off
    ("mpi1", (1, 1, (1280, 720), 1, 0.3)),
    ("mpi19", (1, 19, (1280, 720), 1, 0.3)),
    ("mpi64", (1, 64, (640, 360), 1, 0.3)),
    ("mpi127", (1, 127, (1280, 720), 1, 0.3)),
])


def _thr(model, **kw):
    t = dict(orc.default_thresholds(model))
    t.update(kw)
    return t


# ---- threshold sets: name -> changes against the model's defaults
THRESHOLDS = OrderedDict(
    [("default", {})] +
    [(f"above{v}", dict(inter_min_above=v)) for v in (0, 4, 7, 9, 10, 12)] +
    [("sub1_0", dict(min_subset_cnt=1, min_subset_score=0.0)), ("sub2_005", dict(min_subset_cnt=2, min_subset_score=0.05)),
     ("sub3_03", dict(min_subset_cnt=3, min_subset_score=0.3)), ("sub5_12", dict(min_subset_cnt=5, min_subset_score=1.2))] +
    [("inter0", dict(inter_threshold=0.0)), ("inter-1", dict(inter_threshold=-1.0)), ("inter03", dict(inter_threshold=0.3))] +
    [("nms0", dict(nms_threshold=0.0)), ("nms-001", dict(nms_threshold=-0.01)), ("nms005", dict(nms_threshold=0.05)),
     ("nms02", dict(nms_threshold=0.2)), ("nms05", dict(nms_threshold=0.5))])
NMS_SETS = ["nms0", "nms-001", "nms005", "nms02", "nms05"]


def thresholds(engine, name):
    return _thr(ENGINES[engine][0], **THRESHOLDS[name])


# ---- cases: (engine, input, threshold sets).  No cross product: each engine gets the sets its branches need (test_postproc_sizes_cpu.py says which).
CASES = [
    ("coco1", "noise", ["default", "sub1_0", "inter-1"]),
    ("coco1", "people5", ["default", "sub2_005"]),
    ("coco2", "noise", ["default", "sub1_0", "above0"]),
    ("coco2", "people5", ["default", "sub3_03"]),
    ("coco63", "noise", ["default", "above10", "above12", "above7"]),
    ("coco63", "people40", ["default", "sub3_03", "sub5_12"]),
    ("coco63", "straddle05", NMS_SETS),
    ("coco63", "straddle20", NMS_SETS),
    ("coco63", "straddle50", NMS_SETS),
    ("coco65", "noise", ["default", "above4", "inter0"]),
    ("coco65", "ties", ["default", "above0"]),
    ("coco65", "single_sided", ["default", "sub1_0"]),
    ("coco90", "noise", ["default", "above0"]),
    ("coco91", "noise", ["default", "above0"]),
    ("coco91", "ties", ["default"]),
    ("coco120", "noise", ["default", "sub1_0"]),
    ("coco120", "late_cap", ["default"]),
    ("coco121", "noise", ["default", "above0", "sub2_005"]),
    ("coco121", "late_cap", ["default", "sub3_03"]),
    ("coco121", "people40", ["default", "sub5_12"]),
    ("coco127", "noise", ["default", "above0", "above4", "inter-1", "sub2_005"]),
    ("coco127", "people5", ["default", "inter03"]),
    ("coco127", "people40", ["default", "sub3_03", "above0", "above4", "above7"]),
    ("coco127", "ties", ["default", "above9"]),
    ("coco127", "single_sided", ["default", "sub1_0"]),
    ("coco127", "late_cap", ["default"]),
    ("coco127x3", "noise", ["default", "above7", "nms0"]),
    ("mpi1", "noise", ["default", "sub1_0", "above0"]),
    ("mpi1", "people5", ["default"]),
    ("mpi19", "noise", ["default", "above7"]),
    ("mpi19", "people5", ["default", "sub2_005"]),
    ("mpi19", "ties", ["default"]),
    ("mpi19", "straddle20", NMS_SETS),
    ("mpi64", "noise", ["default", "above0"]),
    ("mpi64", "single_sided", ["default", "sub1_0"]),
    ("mpi127", "noise", ["default", "above4", "inter03"]),
    ("mpi127", "people40", ["default", "sub3_03", "above0", "above4"]),
    ("mpi127", "ties", ["default", "above0"]),
    ("mpi127", "single_sided", ["default", "sub1_0"]),
]


def case_id(case):
    return f"{case[0]}-{case[1]}"


# ------------------------------------------------------------------------------------------
# prototxt with a chosen max_peaks
# ------------------------------------------------------------------------------------------
_dir = []


def proto_text(model, max_peaks):
    import caffe_rtpose_amd as r
    if not _dir:
        _dir.append(tempfile.mkdtemp(prefix="postcases_"))
        atexit.register(shutil.rmtree, _dir[0], ignore_errors=True)
    base = os.path.join(_dir[0], f"builtin{model}.prototxt")
    if not os.path.exists(base):
        r.write_builtin_prototxt(model, base)
    with open(base) as f:
        lines = f.read().split("\n")
    hits = [i for i, l in enumerate(lines) if l.strip().startswith("max_peaks:")]
    assert len(hits) == 1, hits
    lines[hits[0]] = lines[hits[0]].split("max_peaks:")[0] + f"max_peaks: {max_peaks}"
    return "\n".join(lines)


def proto_file(model, max_peaks):
    """path of the built-in graph of `model` with `max_peaks: N`, written once per process into a directory that goes away at exit"""
    text = proto_text(model, max_peaks)
    path = os.path.join(_dir[0], f"m{model}_peaks{max_peaks}.prototxt")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(text)
    return path


def config(engine, **kw):
    """the cheapest plan: only the post-processing taps run on these engines"""
    import caffe_rtpose_amd as r
    model, mp, (dw, dh), N, gap = ENGINES[engine]
    args = dict(model=model, proto_path=proto_file(model, mp), net_w=NET_W, net_h=NET_H, disp_w=dw, disp_h=dh, num_scales=N, scale_gap=gap,
                precision=r.PREC_FP16, frames_in_flight=1)
    args.update(kw)
    return r.Config(**args)


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def _dims(model):
    num_parts, num_limbs, _, _ = orc.model_tables(model)
    return num_parts, num_limbs, num_parts + 1 + 2 * num_limbs


def _grid(n, ox, oy):
    """n points on a 16-column grid of pitch 18 x 17 px, shifted by (ox, oy): inside 320x176 for n <= 127 and shifts up to 12.  The pitches
    differ so that only a peak's own partner (same index, shifted along (1, 1)) lies exactly along the constant PAF."""
    i = np.arange(n)
    return 10.0 + 18.0 * (i % 16) + ox, 10.0 + 17.0 * (i // 16) + oy


def _const_paf(model):
    """every PAF channel holds the unit vector along (1, 1): all pairs of one direction tie"""
    num_parts, _, C = _dims(model)
    res = np.zeros((C, NET_H, NET_W), np.float32)
    res[num_parts + 1:] = 0.70710677
    return res


def _noise(model, mp, N):
    """white noise on top of a smooth field: every part has more maxima than any cap"""
    _, _, C = _dims(model)
    low = (0.25 * _synth.smooth_field(N * C, LOW_H, LOW_W, seed=31).reshape(N, C, LOW_H, LOW_W)
           + np.random.default_rng(7).uniform(-1.0, 1.0, (N, C, LOW_H, LOW_W)).astype(np.float32))
    return dict(kind="low", low=np.ascontiguousarray(low, np.float32))


def _people(model, mp, N, P):
    low, _ = _synth.people_lowres(model, orc.model_tables(model), P, LOW_H, LOW_W, seed=44, N=N)
    return dict(kind="low", low=low)


def _ties(model, mp, N):
    """the constant-PAF construction of test_connect_ties_and_saturation with up to max_peaks peaks per part: peaks of a part on a line of
    direction (2, 1), every coordinate a multiple of 0.25, so that pairs with the same j - i have exactly the same score"""
    num_parts, _, _ = _dims(model)
    rs = np.random.RandomState(11)
    peaks = np.zeros((num_parts, mp + 1, 3), np.float32)
    for p in range(num_parts):
        n = mp if p % 3 == 0 else int(rs.randint(max(1, mp // 2), mp + 1))
        peaks[p, 0, 0] = n
        bx, by = np.round(rs.uniform(4, 30) * 4) / 4, np.round(rs.uniform(4, 25) * 4) / 4
        i = np.arange(1, n + 1)
        peaks[p, 1:n + 1, 0] = bx + 2.0 * i + 1.5 * p
        peaks[p, 1:n + 1, 1] = by + 1.0 * i + 1.0 * p
        peaks[p, 1:n + 1, 2] = rs.uniform(0.3, 0.9, n)
    assert peaks[:, :, 0].max() < NET_W - 1 and peaks[:, :, 1].max() < NET_H - 1
    return dict(kind="tap", res=_const_paf(model), peaks=peaks)


# peak ordinals of the far end that sit over a peak of the near end, i.e. that a connection holds before the one-sided limb comes: below and above 64
HELD_COCO = list(range(1, 47)) + [60, 62, 63, 64, 66, 67, 69, 70]
HELD_MPI = [2, 5, 9, 30, 41, 63, 64, 66, 69, 70]


def _single_sided(model, mp, N):
    """Limbs with peaks at one end only, sized so that every row comes out under the max_people cap when min_subset_cnt is 1.
    a = the part that starts the skeleton's first limb, b = its other end with n = min(max_peaks, 70) peaks on the grid, and the part behind b is
    empty.  a's peaks lie under the peaks HELD_* of b, so limb 0 puts those ordinals of b into rows; the limb behind b then sees b alone.
    COCO appends "only peaks no row holds yet": the ordinals 47..59, 61, 65, 68 — 86 rows in all, so a held ordinal that slipped
    through the filter would come out too.  It has a second chain (c = part 5 behind a, nothing behind c) built the same way.
    MPI appends all n; parts 5 and 14 get one peak each, so that its two other limbs that start at b are no further one-sided limbs on b."""
    num_parts, _, limb_seq, _ = orc.model_tables(model)
    peaks = np.zeros((num_parts, mp + 1, 3), np.float32)
    a, b = limb_seq[0], limb_seq[1]
    n = min(mp, 70)
    held = [h for h in (HELD_COCO if model == 0 else HELD_MPI) if h <= n]
    rs = np.random.RandomState(5)

    def put(part, idx, ox, oy):
        x, y = _grid(n, ox, oy)
        k = len(idx)
        peaks[part, 0, 0] = k
        peaks[part, 1:k + 1, 0], peaks[part, 1:k + 1, 1], peaks[part, 1:k + 1, 2] = x[idx], y[idx], rs.uniform(0.3, 0.9, k)

    put(a, np.array(held) - 1, 0, 0)
    put(b, np.arange(n), 6, 6)            # along (1, 1) from a's peaks: the constant PAF scores exactly these pairs highest
    if model == 0:
        assert limb_seq[2] == a
        put(limb_seq[3], np.arange(n), 3, 3)
    else:
        put(5, np.array([0]), 9, 9)
        put(14, np.array([1]), 9, 9)
    return dict(kind="tap", res=_const_paf(model), peaks=peaks)


def _late_cap(model, mp, N):
    """COCO: parts 2, 5 and 8 have peaks and their neighbours none, so the limbs (1,2), (1,5), (1,8) append 3 * max_peaks one-part rows, which
    fail min_subset_cnt; then the chain 11 -> 12 -> 13 builds max_peaks three-part rows of high score behind them."""
    assert model == 0 and 3 * mp > 256 and mp > MAX_PEOPLE
    peaks = np.zeros((18, mp + 1, 3), np.float32)
    rs = np.random.RandomState(6)
    for part, (ox, oy), lo, hi in ((2, (0, 0), 0.06, 0.2), (5, (3, 1), 0.06, 0.2), (8, (1, 4), 0.06, 0.2),
                                   (11, (0, 0), 0.8, 0.95), (12, (5, 5), 0.8, 0.95), (13, (10, 10), 0.8, 0.95)):
        x, y = _grid(mp, ox, oy)
        peaks[part, 0, 0] = mp
        peaks[part, 1:, 0], peaks[part, 1:, 1], peaks[part, 1:, 2] = x, y, rs.uniform(lo, hi, mp)
    return dict(kind="tap", res=_const_paf(model), peaks=peaks)


def _straddle(model, mp, N, t):
    """Three people plus a background of +-b in every part plane: 1.95 * b is 3 % below the NMS threshold t in the left half of the columns and
    3 % above it in the right half, with Gaussians across the seam: the fused NMS kernel skips some columns of a strip and evaluates others."""
    num_parts, _, C = _dims(model)
    low, _ = _synth.people_lowres(model, orc.model_tables(model), 3, LOW_H, LOW_W, seed=44, N=1)
    low = low.reshape(C, LOW_H, LOW_W)
    rs = np.random.RandomState(8)
    b = np.where(np.arange(LOW_W) < LOW_W // 2, 0.97, 1.03).astype(np.float32) * np.float32(t / 1.95)
    bg = rs.choice([-1.0, 1.0], (num_parts, LOW_H, LOW_W)) * rs.uniform(0.9, 1.0, (num_parts, LOW_H, LOW_W)) * b[None, None, :]
    yy, xx = np.mgrid[0:LOW_H, 0:LOW_W].astype(np.float32)
    for g in range(6):
        p, cx, cy = int(rs.randint(num_parts)), LOW_W / 2 + rs.uniform(-2.5, 2.5), rs.uniform(3, LOW_H - 3)
        low[p] = np.maximum(low[p], 0.9 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 0.9 * 0.9)))
    low[:num_parts] += bg.astype(np.float32)
    return dict(kind="low", low=np.ascontiguousarray(low.reshape(1, C, LOW_H, LOW_W), np.float32))


@functools.lru_cache(maxsize=None)
def inputs(engine, name):
    model, mp, _, N, _ = ENGINES[engine]
    if name == "noise":
        return _noise(model, mp, N)
    if name.startswith("people"):
        return _people(model, mp, N, int(name[6:]))
    if name.startswith("straddle"):
        return _straddle(model, mp, N, int(name[8:]) / 100.0)
    return {"ties": _ties, "single_sided": _single_sided, "late_cap": _late_cap}[name](model, mp, N)


def stale_peaks(engine):
    """what the peak buffer holds before a run: the slots the kernels do not write must keep it"""
    model, mp, _, _, _ = ENGINES[engine]
    return np.full((_dims(model)[0], mp + 1, 3), -7.0, np.float32)


# ------------------------------------------------------------------------------------------
# oracle results (computed once per process, never modified)
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_resized(engine, name):
    inp = inputs(engine, name)
    if inp["kind"] == "tap":
        return inp["res"]
    res = orc.imresize(inp["low"], NET_W, NET_H, 1.0, ENGINES[engine][4])[0]
    res.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _ref_peaks(engine, name, nms_threshold):
    inp = inputs(engine, name)
    model, mp, _, _, _ = ENGINES[engine]
    pk = inp["peaks"] if inp["kind"] == "tap" else orc.nms(ref_resized(engine, name), _dims(model)[0], mp, nms_threshold, stale_peaks(engine))
    pk.setflags(write=False)
    return pk


def ref_peaks(engine, name, thr_name):
    return _ref_peaks(engine, name, thresholds(engine, thr_name)["nms_threshold"])


def _connect_args(engine, name, thr_name):
    model, mp, (dw, dh), _, _ = ENGINES[engine]
    return (model, ref_resized(engine, name), ref_peaks(engine, name, thr_name), mp, NET_W, NET_H, dw, dh, thresholds(engine, thr_name))


@functools.lru_cache(maxsize=None)
def reference(engine, name, thr_name):
    """(resized map, peaks, num_people, joints[num_people]) of the oracle chain ImResize -> Nms -> connect"""
    n, joints = orc.connect(*_connect_args(engine, name, thr_name))
    return ref_resized(engine, name), ref_peaks(engine, name, thr_name), n, joints[:n].copy()


# ------------------------------------------------------------------------------------------
# what a run reaches: facts from the oracle's decision trace, and the conditions B1..B10 of csrc/postproc.hip restated on them
# ------------------------------------------------------------------------------------------
K_POST_DYN_LDS_MAX = 160 * 1024 - 4096       # kPostDynLdsMax


def sort_keys(mp):
    """launch_connect_impl: n2, the power of two >= max_peaks^2 (at least 64) that sizes the match kernel's key array"""
    n2 = 64
    while n2 < mp * mp:
        n2 <<= 1
    return n2


def keys_of(nc):
    """connect_match_limb: the power of two >= the limb's survivors (at least 64) that the bitonic sort runs over"""
    n2 = 64
    while n2 < nc:
        n2 <<= 1
    return n2


def assemble_preload(model, mp):
    """launch_connect_impl: does the assemble kernel's LDS copy of its inputs fit next to the subset table?"""
    num_parts, num_limbs, _ = _dims(model)
    lds2 = num_limbs * mp * (8 + 2 + 2 * num_parts)
    extra = 8 + (num_parts * 3 * (mp + 1) + num_limbs * mp * 3 + num_limbs) * 4
    return lds2 + extra <= K_POST_DYN_LDS_MAX


def _axis_nb(x, offset, f, osize):
    """axis_nb of postproc.hip for start_scale 1 (no padding): clamped integer position, first and last neighbour"""
    x_on = np.float32(np.float32(x - offset) * f)
    xn1 = max(int(np.float64(x_on) + 1e-5), 0)
    n0 = xn1 if xn1 - 1 < 0 else xn1 - 1
    xn2 = osize - 1 if xn1 + 1 >= osize else xn1 + 1
    n3 = osize - 1 if xn2 + 1 >= osize else xn2 + 1
    return xn1, n0, xn2, n3


def nms_skip_stats(low, num_parts, threshold, strip_rows=8):
    """nms_fused_strip_kernel's bound pre-pass on a one-scale low-res map, strip by strip: (strips skipped whole, strips with the column skip on
    that skip some columns AND evaluate others, strips evaluated in full).
    The value the kernel leaves in a skipped column cannot show: it is the threshold itself, the true value there is at most the threshold, and a
    flag needs v > threshold, so v compares alike with either; the write kernel evaluates its 7x7 window again from the low-res maps."""
    assert low.shape[0] == 1
    h, w = low.shape[2:]
    H, W = 8 * h, 8 * w
    bound, thr = np.float32(1.95), np.float32(threshold)
    off_y, fy = np.float32(np.float64(np.float32(H / np.float32(h)) / 2) - 0.5), np.float32(np.float32(h) / H)
    off_x, fx = np.float32(np.float64(np.float32(W / np.float32(w)) / 2) - 0.5), np.float32(np.float32(w) / W)
    cols = [_axis_nb(x, off_x, fx, w) for x in range(W)]
    whole = mixed = full = 0
    for part in range(num_parts):
        for y0 in range(0, H, strip_rows):
            y1 = min(y0 + strip_rows, H)
            ya, yb = max(y0 - 1, 0), min(y1, H - 1)
            rlo, rhi = _axis_nb(ya, off_y, fy, h)[1], _axis_nb(yb, off_y, fy, h)[3]
            colmax = np.abs(low[0, part, rlo:rhi + 1]).max(axis=0)
            if not bound * colmax.max() > thr:
                whole += 1
                continue
            if bound * colmax.min() > thr or rhi - rlo + 1 >= 8:
                full += 1
                continue
            skipped = [not bound * max(colmax[a], colmax[b], colmax[c], colmax[d]) > thr for b, a, c, d in cols]
            mixed += any(skipped) and not all(skipped)
            full += not any(skipped)
    return whole, mixed, full


def facts(engine, name, thr_name):
    """what the oracle did on one (engine, input, threshold set), as far as the branches below depend on it"""
    model, mp, _, N, _ = ENGINES[engine]
    num_parts, num_limbs, limb_seq, _ = orc.model_tables(model)
    args = _connect_args(engine, name, thr_name)
    thr = args[-1]
    n, joints, cand, conn, rows = orc.connect_trace(*args)
    pk = args[2]
    cnt = np.minimum(pk[:, 0, 0].astype(int), mp)
    limbs = [(int(cnt[limb_seq[2 * k]]), int(cnt[limb_seq[2 * k + 1]])) for k in range(num_limbs)]
    survivors = np.bincount(cand[cand[:, 3] > 0, 0].astype(int), minlength=num_limbs) if len(cand) else np.zeros(num_limbs, int)
    kept = np.flatnonzero(rows[:, num_parts + 2] > 0) if len(rows) else np.zeros(0, int)
    f = dict(engine=engine, input=name, thr=thr_name, model=model, max_peaks=mp, num_scales=N, thresholds=thr, n=n, counts=pk[:, 0, 0].copy(),
             limbs=limbs, survivors=survivors, conn=conn, rows=rows, kept=kept, num_parts=num_parts, limb_seq=limb_seq)
    # accepted candidates of one limb that share a score: std::sort's order of equal elements decides (the stdsort_replica path)
    tied_hi = False
    if len(cand):
        acc = cand[cand[:, 3] > 0]
        for k in range(num_limbs):
            a = acc[acc[:, 0] == k]
            if len(a) > 1:
                s, first, c = np.unique(a[:, 4], return_index=True, return_counts=True)
                dup = np.isin(a[:, 4], s[c > 1])
                tied_hi = tied_hi or bool((dup & (a[:, 1] > 64) & (a[:, 2] > 64)).any())
    f["tied_above_64"] = tied_hi
    if inputs(engine, name)["kind"] == "low" and N == 1:
        f["nms_skip"] = nms_skip_stats(inputs(engine, name)["low"], num_parts, thr["nms_threshold"])
    return f


def one_sided_chains(f):
    """[dict] per part that some limb sees at one end only (the first such limb): its peak count n, the ordinals a connection's row holds
    (`held`), the ordinals appended as one-part rows (`appended`) and those of them that are emitted, i.e. among the first max_people kept
    rows (`emitted`).  Rows of one part are one-sided appends by construction: no later limb extends them in these inputs."""
    out, seen = [], set()
    NP = f["num_parts"]
    peaks_offset = 3 * (f["max_peaks"] + 1)
    rows = f["rows"]
    rank = {int(r): k for k, r in enumerate(f["kept"])}           # row index -> position among the kept rows
    for k, (nA, nB) in enumerate(f["limbs"]):
        if (nA == 0) != (nB == 0):
            part = f["limb_seq"][2 * k + 1] if nA == 0 else f["limb_seq"][2 * k]
            if part in seen:
                continue
            seen.add(part)
            ordinal = lambda v: int(v - part * peaks_offset - 2) // 3
            has = np.flatnonzero(rows[:, part] > 0) if len(rows) else []
            held = sorted(ordinal(rows[r, part]) for r in has if rows[r, NP] >= 2)
            app = [(ordinal(rows[r, part]), int(r)) for r in has if rows[r, NP] == 1]
            out.append(dict(limb=k, part=part, n=nB if nA == 0 else nA, held=held, appended=[o for o, _ in app],
                            emitted=[o for o, r in app if rank.get(r, MAX_PEOPLE) < MAX_PEOPLE]))
    return out


def b6(f):
    """a limb with more than 64 peaks at one end only whose one-part rows with ordinals above 64 are EMITTED (under the max_people cap).  COCO
    ("only peaks no row holds yet"): ordinals below and above 64 both among the held and among the emitted ones, and so few rows that every
    held ordinal above 64, appended by mistake, would be emitted too.  MPI: all n appended, the held ones too, and every row emitted."""
    chains = [c for c in one_sided_chains(f) if c["n"] > 64 and any(o > 64 for o in c["emitted"])]
    if f["model"] == 1:     # (a later limb may extend an appended row: it then counts as held here)
        return any(len(c["held"]) + len(c["appended"]) > c["n"] for c in chains) and len(f["kept"]) == len(f["rows"]) <= MAX_PEOPLE
    extra = sum(sum(o > 64 for o in c["held"]) for c in chains)
    return any(min(c["held"]) < 64 < max(c["held"]) and min(c["emitted"]) < 64 for c in chains) and len(f["kept"]) == len(f["rows"]) \
        and len(f["rows"]) + extra <= MAX_PEOPLE


def b1(f):
    """launch_connect_impl: the sort keys need more than 64 KiB of LDS (ensure_lds<connect_match_kernel>)"""
    return sort_keys(f["max_peaks"]) * 8 > 64 * 1024


def b2(f, keys=8192):
    """connect_match_limb: the bitonic sort's 8-pairs-per-thread path over `keys` keys (8192 or 16384)"""
    return any(keys_of(int(s)) == keys for s in f["survivors"])


def b3(f):
    """greedy scan: the second occupancy word on both sides, key fields above 64"""
    c = f["conn"]
    return len(c) > 0 and bool((c[:, 1] > 64).any() and (c[:, 2] > 64).any())


def b4(f):
    """the assemble kernel reads global memory: its LDS copy does not fit (and there are people to emit from it)"""
    return not assemble_preload(f["model"], f["max_peaks"]) and f["n"] > 0


def b5(f):
    """blk_off filled up to index 64: a limb with more than 63 blocks of 256 pairs"""
    return any(nA * nB > 16128 for nA, nB in f["limbs"])


def b7(f):
    """allowed_fail of the pair kernel's early exit, on a run with pairs to test (None: no pairs)"""
    return 10 - (f["thresholds"]["inter_min_above"] + 1) if any(nA * nB > 0 for nA, nB in f["limbs"]) else None


def b8(f):
    """emission: the max_people cap falls in a later 256-row chunk than the first"""
    return len(f["rows"]) > 256 and len(f["kept"]) >= MAX_PEOPLE and f["kept"][MAX_PEOPLE - 1] >= 256 and f["kept"][0] >= 256


def b9(f):
    """tiny caps: one or two peaks per part, more maxima than that in the map, pairs to connect"""
    return f["max_peaks"] <= 2 and bool((f["counts"] > f["max_peaks"]).all()) and any(nA * nB > 0 for nA, nB in f["limbs"]) and len(f["conn"]) > 0


def b10(f):
    """fused NMS: (a strip skipped whole, a strip with skipped and evaluated columns, a threshold <= 0)"""
    whole, mixed, _ = f.get("nms_skip", (0, 0, 0))
    return whole > 0, mixed > 0, "nms_skip" in f and f["thresholds"]["nms_threshold"] <= 0


# ------------------------------------------------------------------------------------------
# the input of test_gpu_parity.test_fused_postproc_from_lowres_bit_exact (that test calls this; the CPU file asks the oracle about the same maps)
# ------------------------------------------------------------------------------------------
def fused_case_input(model, W, H, N, start, gap, kind):
    h, w = H // 8, W // 8
    tabs = orc.model_tables(model)
    heat_channels = _dims(model)[2]
    if kind == "noise":
        return (_synth.smooth_field(N * heat_channels, h, w, seed=31, scale=1.0).reshape(N, heat_channels, h, w)
                + 0.25 * np.random.default_rng(7).standard_normal((N, heat_channels, h, w)).astype(np.float32))
    if kind.startswith("speople"):   # the same people at every scale, planted in each scale's crop window
        import _pincases as pincases
        return pincases.scaled_people(model, tabs, int(kind[7:]), h, w, 44, N, start, gap)
    low, _ = _synth.people_lowres(model, tabs, int(kind[6:]), h, w, seed=44, N=N)
    return low.reshape(N, heat_channels, h, w)

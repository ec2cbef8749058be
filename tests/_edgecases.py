"""The smallest and the widest nets the plan accepts — TEST INFRASTRUCTURE of tests/test_net_envelope_cpu.py and tests/test_net_envelope.py (numpy only).

build_plan takes any net_w x net_h that are multiples of 16, from 16x16 upward; the only upper bound is on the width (2736 accepted, 2752 refused:
the fused ImResize+Nms strip kernel keeps whole rows in LDS).  Here: the plans, the post-processing geometries and the inputs at both ends of that
envelope, and the strip rule of Builder::postproc_sizes restated in Python.

At 16x16 the 1/8 maps are 2x2: the 7x7 layers read almost only halo, every bicubic neighbour is a clamped one, NMS has 14 interior columns and one
64-column ballot block.  On the wide nets the strip kernel halves its strip height until its rows fit into 150 KiB:
  one scale       8 rows up to W = 1920, 4 rows from 1936, 2 rows from 2416
  several scales  16 rows up to W = 1360, 8 rows from 1376, then as for one scale
and its LDS carve (out, T, xt, colmax in T's last row, the ballots and their prefix in T) depends on both numbers."""
import functools
from collections import OrderedDict

import numpy as np

import _oracle as orc
import _postcases as pc

# ------------------------------------------------------------------------------------------
# plans: the columns of _convcheck.MATRIX  name -> (mode, model, W, H, num_scales, scale_gap, batch_frames, synthetic_seed)
# ------------------------------------------------------------------------------------------
CONV_EDGE = OrderedDict([
    ("mixed_coco_16x16", ("mixed", 0, 16, 16, 1, 0.3, 1, 1)),                  # 2x2 at 1/8: three stand-alone pooling steps, every pixel a border pixel
    ("mixed_mpi_16x16_3s_b3", ("mixed", 1, 16, 16, 3, 0.15, 3, 1)),            # nine images per launch, each far smaller than a tile
    ("fp32_coco_16x16", ("fp32", 0, 16, 16, 1, 0.3, 1, 1)),                    # conv k 3 cin_p 64 / 128 tile 64x64 rowb 256 passes 1 ring
    ("f16x3_coco_32x16", ("f16x3", 0, 32, 16, 1, 0.3, 1, 1)),                  # conv pair k 7 cin_p 128 tile 64x64 rowb 256 passes 3aw ring
    ("fp16_coco_16x32_b2", ("fp16", 0, 16, 32, 1, 0.3, 2, 1)),                 # portrait; conv k 3 cin_p 128 tile 64x64 rowb 256 passes 1 ring
    ("mixed_coco_16x512", ("mixed", 0, 16, 512, 1, 0.3, 1, 1)),                # two columns at 1/8: a tile wraps 32 rows
    ("mixed_coco_2736x16", ("mixed", 0, 2736, 16, 1, 0.3, 1, 1)),              # the widest net: two rows of 342 at 1/8
    ("mixed_coco_1936x16", ("mixed", 0, 1936, 16, 1, 0.3, 1, 1)),              # 4-row strips.  16 rows here and below, not 32: at 32 rows the two cases took
    ("mixed_coco_1376x16_2s", ("mixed", 0, 1376, 16, 2, 0.3, 1, 1)),           # 3.1 and 3.9 s, tests/test_conv_launches.py at 320x176 takes 1.9 (profiles/net_envelope_check.txt)
    ("fp32_coco_2736x16", ("fp32", 0, 2736, 16, 1, 0.3, 1, 1)),                # conv pair k 7 cin_p 192 tile 128x32 rowb 256 passes 1 ring
])

# full batches (the columns of _convcheck.BATCH_MATRIX): the batched plans above, and five 16x16 frames — an image far smaller than any tile,
# grids that are no multiple of 8
BATCH_EDGE = OrderedDict([(n, CONV_EDGE[n]) for n in ("mixed_mpi_16x16_3s_b3", "fp16_coco_16x32_b2")] +
                         [("mixed_coco_16x16_b5", ("mixed", 0, 16, 16, 1, 0.3, 5, 1))])

# the kernel classes that only these plans reach (_convcheck.key_str), and the entry each is reached by
EDGE_ONLY_CLASSES = OrderedDict([
    ("conv k 3 cin_p 64 tile 64x64 rowb 256 passes 1 ring", ["fp32_coco_16x16"]),
    ("conv k 3 cin_p 128 tile 64x64 rowb 256 passes 1 ring", ["fp32_coco_16x16", "fp16_coco_16x32_b2"]),
    ("conv pair k 7 cin_p 128 tile 64x64 rowb 256 passes 3aw ring", ["f16x3_coco_32x16"]),
    ("conv pair k 7 cin_p 192 tile 128x32 rowb 256 passes 1 ring", ["fp32_coco_2736x16"]),
])

# ------------------------------------------------------------------------------------------
# post-processing geometries: (model, W, H, num_scales, start_scale, scale_gap, input kind)
# ------------------------------------------------------------------------------------------
POST_WIDE_NOISE = [
    (0, 1920, 16, 1, 1.0, 0.3, "noise"),        # the last width with 8-row strips
    (0, 1936, 32, 1, 1.0, 0.3, "noise"),        # 4-row strips
    (0, 2416, 32, 1, 1.0, 0.3, "noise"),        # 2-row strips
    (0, 2736, 32, 1, 1.0, 0.3, "noise"),        # the widest net
    (0, 1376, 32, 2, 1.0, 0.3, "noise"),        # several scales: 8-row strips
    (0, 2736, 16, 3, 0.8, 0.15, "noise"),       # several scales on 2-row strips, cropped levels
]
POST_TINY_NOISE = [
    (0, 16, 16, 1, 1.0, 0.3, "noise"),          # 2x2 low-res maps: every neighbour clamped
    (0, 32, 16, 1, 1.0, 0.3, "noise"),
    (0, 48, 16, 2, 1.0, 0.3, "noise"),
]
POST_LAST_BEFORE_HALVING = [
    (0, 1360, 32, 2, 1.0, 0.3, "noise"),        # 16-row strips
    (0, 2400, 16, 1, 1.0, 0.3, "noise"),        # 4-row strips
]
POST_MPI = [(1, 2736, 16, 1, 1.0, 0.3, "noise")]
POST_ERANGE = (0, 16, 32, 1, 1.0, 0.3, "noise")   # portrait: the reference's connect CHECK-fails on a PAF sample coordinate (RTP_ERANGE)
POST_EDGE = POST_WIDE_NOISE + POST_TINY_NOISE + POST_LAST_BEFORE_HALVING + POST_MPI + [POST_ERANGE]

# the column-skip branch of the strip kernel at 4- and 2-row strips: (model, W, H, num_scales, start_scale, scale_gap, "straddle")
STRADDLE_EDGE = [
    (0, 1936, 48, 1, 1.0, 0.3, "straddle"),
    (0, 2416, 48, 1, 1.0, 0.3, "straddle"),
]
DISPLAY = (1280, 720)


def post_id(case):
    model, W, H, N, start, gap, kind = case
    return f"{'coco' if model == 0 else 'mpi'}_{W}x{H}_{N}s_{start}_{kind}"


def max_peaks(model):
    return 64 if model == 0 else 20


# ------------------------------------------------------------------------------------------
# the strip rule (plan.cpp Builder::postproc_sizes) and the LDS of nms_fused_strip_kernel (postproc.hip)
# ------------------------------------------------------------------------------------------
NMSF_TROWS = 8
STRIP_LDS_CAP = 150 * 1024
YTAB_ROWS = 24
MIN_W, MAX_W = 16, 2736


def strip_lds(rows, W):
    """dynamic LDS of the strip kernel: out [rows + 2][W], T [NMSF_TROWS][W] floats and the column table xt [W] of 8 bytes"""
    return (rows + 2 + NMSF_TROWS) * W * 4 + W * 8


def strip_rows(W, scales):
    """strip height the plan chooses for a net W wide, None where no height fits (the plan refuses that width)"""
    rows = 16 if scales > 1 else 8
    while rows > 2 and strip_lds(rows, W) > STRIP_LDS_CAP:
        rows //= 2
    return rows if strip_lds(rows, W) <= STRIP_LDS_CAP else None


def postproc_line(W, H, scales, model=0):
    """the `postproc` line of rtp_plan_summary as the rule above gives it"""
    rows = strip_rows(W, scales)
    _, num_limbs, _, _ = orc.model_tables(model)
    return f"postproc strip_rows {rows} nstrips {(H + rows - 1) // rows} max_rows {num_limbs * max_peaks(model)}"


def ballot_bytes(rows, W):
    """what the flag phase keeps in T: one 64-bit ballot per (row, 64-column block) and the int prefix in front of every group, + 1"""
    ng = (W + 63) // 64
    return 8 * rows * ng + 4 * (rows * ng + 1)


def summary_postproc(summary):
    """(strip_rows, nstrips, max_rows) of an rtp_plan_summary text; the line is never the first one"""
    lines = summary.splitlines()
    hits = [ln for ln in lines if ln.startswith("postproc ")]
    assert len(hits) == 1 and not lines[0].startswith("postproc "), hits
    w = hits[0].split()
    assert w[1::2] == ["strip_rows", "nstrips", "max_rows"], hits[0]
    return int(w[2]), int(w[4]), int(w[6])


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def straddle_lowres(model, h, w, t, seed=8):
    """_postcases._straddle at a given low-res size, for strips of a few rows: every part plane holds a background of +-b, and 1.95 * b is 3 % below the
    NMS threshold t in the left half of the columns and 3 % above it in the right half, times a factor in [0.9, 1] per pixel.  Gaussians of height 0.9
    cross the seam in every third part (planted by hand: _synth.people_lowres plants nothing on maps of a few rows).  So that strips of either plain
    kind occur too, part 1 holds the background 10 % lower (nothing reaches the bound: its strips are skipped whole) and part 2 holds it at full
    height 5 % higher (every column reaches the bound: its strips are evaluated in full).  PAF channels stay 0."""
    num_parts, _, C = pc._dims(model)
    rs = np.random.RandomState(seed)
    low = np.zeros((C, h, w), np.float32)
    b = np.where(np.arange(w) < w // 2, 0.97, 1.03).astype(np.float32) * np.float32(t / 1.95)
    sign = rs.choice([-1.0, 1.0], (num_parts, h, w))
    fac = rs.uniform(0.9, 1.0, (num_parts, h, w))
    fac[1] *= 0.9
    fac[2] = 1.05
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    for p in range(0, num_parts, 3):
        for g in range(3):
            cx, cy = w / 2 + rs.uniform(-2.5, 2.5), rs.uniform(0.5, h - 1.5)
            low[p] = np.maximum(low[p], 0.9 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 0.9 * 0.9)))
    low[:num_parts] += (sign * fac * b[None, None, :]).astype(np.float32)
    return np.ascontiguousarray(low.reshape(1, C, h, w), np.float32)


@functools.lru_cache(maxsize=None)
def post_input(case):
    """[N][C][H/8][W/8] low-res maps of a POST_EDGE / STRADDLE_EDGE case (read-only: shared by the tests)"""
    model, W, H, N, start, gap, kind = case
    if kind == "straddle":
        low = straddle_lowres(model, H // 8, W // 8, orc.default_thresholds(model)["nms_threshold"])
    else:
        low = np.ascontiguousarray(pc.fused_case_input(model, W, H, N, start, gap, kind), np.float32)
    low.setflags(write=False)
    return low


def stale_peaks(model):
    """what the peak buffer holds before a run: the slots the kernels do not write must keep it"""
    return np.full((pc._dims(model)[0], max_peaks(model) + 1, 3), -7.0, np.float32)


@functools.lru_cache(maxsize=None)
def post_reference(case):
    """(resized map, peaks, num_people or None where the oracle's connect refuses the input, joints[num_people]) of the oracle chain
    ImResize -> Nms -> connect at the default thresholds, computed once per process and never modified"""
    model, W, H, N, start, gap, kind = case
    thr = orc.default_thresholds(model)
    res = orc.imresize(post_input(case), W, H, start, gap)[0]
    peaks = orc.nms(res, pc._dims(model)[0], max_peaks(model), thr["nms_threshold"], stale_peaks(model))
    try:
        n, joints = orc.connect(model, res, peaks, max_peaks(model), W, H, DISPLAY[0], DISPLAY[1], thr)
        joints = joints[:n].copy()
    except AssertionError:          # orc.connect: "oracle connect failed"
        n, joints = None, None
    for a in (res, peaks, joints):
        if a is not None:
            a.setflags(write=False)
    return res, peaks, n, joints

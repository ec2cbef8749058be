"""4 to 16 scales and batches of up to 16 frames — TEST INFRASTRUCTURE of tests/test_many_scales.py (GPU), tests/test_many_scales_cpu.py and of
the many-image cases of tests/test_conv_launches.py / tests/test_batch_launches.py.

rtp_engine_create takes num_scales 1..16 and batch_frames up to 16: up to 256 images per convolution launch, four area-pad launches per
frame, scale loops of 16 in the post-processing kernels.  The rest of the suite stops at 3 scales (one pre-processing case at 4), 6 images per
launch and 5 frames per batch.  Here: the cases that go up to the accepted limits, the smallest shapes at which the code takes the paths in
between, and Python restatements of what each case is there for (the CPU file asserts them without a device).

Scale gaps follow one rule, gap(N) = min(0.3, round(0.9 / (N - 1), 3)): the last scale is 0.1 of the net from 4 scales on."""
import functools
from collections import OrderedDict

import numpy as np


def gap(N):
    return 0.3 if N < 2 else min(0.3, round(0.9 / (N - 1), 3))


# ------------------------------------------------------------------------------------------------------------
# 1. convolution launches with many images
# ------------------------------------------------------------------------------------------------------------
# name -> (mode, model, W, H, num_scales, scale_gap, batch_frames, synthetic_seed): the columns of _convcheck.MATRIX; run by the test bodies of
# tests/test_conv_launches.py (every launch alone against float64, one frame) ...
CONV_MATRIX = OrderedDict([
    ("f16x3_coco_64x48_13s", ("f16x3", 0, 64, 48, 13, gap(13), 1, 1)),          # 13 images of a net whose 1/8 map is smaller than one tile
    ("fp32_coco_160x96_7s", ("fp32", 0, 160, 96, 7, gap(7), 1, 1)),             # 7 images, exact-f32 plan
    ("mixed_coco_160x96_13s", ("mixed", 0, 160, 96, 13, gap(13), 1, 1)),        # 13 images, the default mode
    ("fp16_coco_96x64_5s_b2", ("fp16", 0, 96, 64, 5, gap(5), 2, 1)),            # 5 scales x batch_frames 2: the plan of 10 images per launch
])
# ... and of tests/test_batch_launches.py (full batches, bit for bit against the frames tapped alone, graph and eager)
BATCH_MATRIX = OrderedDict([
    ("fp16_coco_96x64_5s_b2", ("fp16", 0, 96, 64, 5, gap(5), 2, 1)),            # (a) 10 images per launch from many scales; ring 64x128
    ("mixed_coco_64x48_16s_b2", ("mixed", 0, 64, 48, 16, gap(16), 2, 1)),       # (b) 32 images per launch
    ("mixed_coco_64x48_b16", ("mixed", 0, 64, 48, 1, 0.3, 16, 1)),              # (c) batch_frames 16 at one scale: 47 frames, 15 in the partial batch
])
BATCH_FLOAT64 = ("fp16_coco_96x64_5s_b2", "mixed_coco_64x48_16s_b2")           # full batches that also run every launch against float64: images 8.. of a launch

# The kernel classes (mode, step kind, impl, tile, rowb, pass label, +pool) that no plan of _convcheck.MATRIX, _convcheck.BATCH_MATRIX or
# _customnets.CUSTOM_MATRIX runs, and the ONE case of CONV_MATRIX each is here for.  The planner picks the ring kernel's 64x128 tile
# (conv_ring.hip ring_launch_cfg, CFG_64x128: KSPLIT 2, 128-byte chunks) as soon as a launch holds about six images of a small net.
NEW_CLASSES = OrderedDict([
    (("f16x3", "conv", "ring", "128x64", 256, "3aw", False), "f16x3_coco_64x48_13s"),
    (("f16x3", "conv", "ring", "64x128", 128, "3aw", False), "f16x3_coco_64x48_13s"),
    (("fp32", "conv", "reg", "128x128", 128, "1", False), "fp32_coco_160x96_7s"),
    (("fp32", "conv", "ring", "64x128", 128, "1", False), "fp32_coco_160x96_7s"),
    (("mixed", "conv", "ring", "64x128", 128, "1", False), "mixed_coco_160x96_13s"),
    (("mixed", "conv", "ring", "64x128", 128, "2q", False), "mixed_coco_160x96_13s"),
    (("fp16", "conv", "ring", "64x128", 128, "1", False), "fp16_coco_96x64_5s_b2"),
])
IMAGE_COUNTS = {7, 10, 13, 16, 32}


def classes(mode, launches):
    return {(mode, L.kind, L.impl, "%dx%d" % L.tile, L.rowb, L.passes, L.pool) for L in launches if L.kind != "pool"}


# ------------------------------------------------------------------------------------------------------------
# 2. pre-processing on the device: more than one area-pad launch per frame
# ------------------------------------------------------------------------------------------------------------
# launch_area_pad (preproc.hip) issues one launch per group of four scales, with scale_base = 4 * group: 5 scales are 4 + 1, 9 are 4 + 4 + 1,
# 16 are 4 x 4.  All at net 160x96.  The display decides the KIND of every level (engine.cpp build_prep_tables):
#   160x96 == the net      level 0 is the display itself (identity), the later groups shrink by integer and by fractional factors
#   96x64 < the net        the levels above 96x64 are ENLARGED (cv::resize's bilinear kernel), 96x64 itself is an identity level in a later group
#   320x180                a plain down-scale, fractional on both axes at every level
PREP_NET = (160, 96)
PREP_SCALES = (5, 9, 16)
PREP_DISPLAYS = OrderedDict([("display_is_net", (160, 96)), ("display_below_net", (96, 64)), ("downscale", (320, 180))])
PREP_FRAME = (200, 150)        # the raw frame: warped to every display with a border (4:3 into 5:3 / 3:2 / 16:9)
PREP_CASES = [(name, N) for name in PREP_DISPLAYS for N in PREP_SCALES]   # (display name, num_scales)


def prep_geom(case):
    """(frame w, h, display w, h, net w, h, scales, start, gap): the columns of test_preprocess_cli.GEOMS"""
    name, N = case
    return PREP_FRAME + PREP_DISPLAYS[name] + PREP_NET + (N, 1.0, gap(N))


def level_sizes(W, H, N, start, scale_gap):
    """(tw, th) of every pyramid level, in the reference's float arithmetic (rtpose.cpp:360-361; test_preprocess_cli restates the same)"""
    out = []
    for i in range(N):
        s32 = np.float32(start - i * scale_gap)
        out.append((int(16 * np.ceil(np.float32(np.float32(W) * s32) / np.float32(16))), int(16 * np.ceil(np.float32(np.float32(H) * s32) / np.float32(16)))))
    return out


def level_kind(dw, dh, tw, th):
    """which branch of area_pad_kernel a level takes (engine.cpp build_prep_tables): identity / linear (an axis is enlarged) / fast (integer
    factors on both axes, cv::resize's is_area_fast) / area (the table path)"""
    if (tw, th) == (dw, dh):
        return "identity"
    if tw > dw or th > dh:
        return "linear"
    if dw % tw == 0 and dh % th == 0:
        return "fast"
    return "area"


def prep_kinds(case):
    """[(group, kind)] per level of a case"""
    fw, fh, dw, dh, W, H, N, start, g = prep_geom(case)
    return [(i // 4, level_kind(dw, dh, tw, th)) for i, (tw, th) in enumerate(level_sizes(W, H, N, start, g))]


def prep_frames(case):
    """the two frames of a case: synthetic content and noise (every rounding boundary), as test_device_preprocess_bit_exact has them"""
    import caffe_rtpose_amd as r
    fw, fh = PREP_FRAME
    img = r.synth_frame(fw, fh, 0, seed=11)
    return [img, np.random.default_rng(5).integers(0, 256, img.shape, dtype=np.uint8)]


# ------------------------------------------------------------------------------------------------------------
# 3. resize, fused NMS, connect over 4 to 16 scales
# ------------------------------------------------------------------------------------------------------------
# (model, W, H, N, start, gap): the columns of test_gpu_parity.RESIZE_CASES.  resize_kernel, the fused NMS kernels and the pair kernel loop over
# r.num scales with an LDS geo[16], accumulate in scale order and divide by num: divisors 4, 5, 7, 11, 13, 16 (none a power of two but 4 and 16),
# a start scale below 1, the MPI channel count, and crops of 2x2 low-res cells at the last scale (160x96 and 64x48 at 16 scales: padw = 9 of 20
# and 3 of 8 columns), where every neighbour clamp of axis_nb is active at every output pixel.
RESIZE_CASES = [
    (0, 160, 96, 4, 1.0, gap(4)),
    (0, 320, 176, 5, 1.0, gap(5)),
    (1, 160, 96, 7, 1.0, gap(7)),          # MPI: 44 channels
    (0, 160, 96, 11, 0.9, 0.08),           # start_scale below 1: scales 0.9 .. 0.1, the first level is padded too
    (0, 96, 64, 13, 1.0, gap(13)),
    (0, 160, 96, 16, 1.0, gap(16)),        # the last crop is 2x2 cells
    (0, 64, 48, 16, 1.0, gap(16)),         # 8x6 low-res map, 2x2 at the end
]
# (model, W, H, N, start, gap, kind): the columns of test_gpu_parity.FUSED_CASES, inputs from _postcases.fused_case_input
FUSED_CASES = [
    (0, 160, 96, 5, 1.0, gap(5), "people5"),
    (0, 160, 96, 9, 1.0, gap(9), "speople5"),
    (0, 160, 96, 16, 1.0, gap(16), "people5"),
    (0, 160, 96, 16, 1.0, gap(16), "speople5"),
    (0, 160, 96, 16, 1.0, gap(16), "noise"),
    (0, 320, 176, 5, 1.0, gap(5), "speople5"),
    (0, 320, 176, 9, 1.0, gap(9), "people5"),
    (0, 320, 176, 16, 1.0, gap(16), "noise"),
    (0, 320, 176, 16, 1.0, gap(16), "people5"),
    (0, 64, 48, 5, 1.0, gap(5), "noise"),
    (0, 64, 48, 9, 1.0, gap(9), "noise"),
    (0, 64, 48, 16, 1.0, gap(16), "noise"),
    (1, 160, 96, 9, 1.0, gap(9), "people5"),
    (1, 160, 96, 5, 0.9, 0.2, "speople5"),     # MPI, start_scale below 1
]


def scale_geo(w, h, W, H, start, scale_gap, n):
    """scale_geo of postproc.hip (imresize_layer.cu:99-131) in its float arithmetic: (padw, padh, ow, oh, offset_x, offset_y, fx, fy)"""
    f32 = np.float32
    k = f32(f32(f32(1) - f32(start)) + f32(f32(n) * f32(scale_gap)))
    padw, padh = int(np.floor(f32(w // 2) * k)), int(np.floor(f32(h // 2) * k))
    ow, oh = w - 2 * padw, h - 2 * padh
    off = lambda t, o: f32(np.float64(f32(f32(t) / f32(o)) / f32(2)) - 0.5)
    return padw, padh, ow, oh, off(W, ow), off(H, oh), f32(f32(ow) / f32(W)), f32(f32(oh) / f32(H))


def clamp_mask(W, H, start, scale_gap, n):
    """[H][W] bool: output pixels at which axis_nb clamps a neighbour of scale n's crop on either axis — the left neighbour of cell 0
    (xn1 - 1 < 0) or one of the two right neighbours (xn1 + 1 >= osize, xn2 + 1 >= osize)"""
    padw, padh, ow, oh, offx, offy, fx, fy = scale_geo(W // 8, H // 8, W, H, start, scale_gap, n)

    def axis(size, offset, f, osize):
        x_on = (np.arange(size, dtype=np.float32) - offset) * f
        xn1 = np.maximum((x_on.astype(np.float64) + 1e-5).astype(np.int64), 0)
        xn2 = np.where(xn1 + 1 >= osize, osize - 1, xn1 + 1)
        return (xn1 - 1 < 0) | (xn1 + 1 >= osize) | (xn2 + 1 >= osize)
    return axis(H, offy, fy, oh)[:, None] | axis(W, offx, fx, ow)[None, :]


@functools.lru_cache(maxsize=None)
def fused_reference(case):
    """the oracle chain of a FUSED case, computed once per process: dict(low, res, peaks, n, joints, cand, conn, rows)"""
    import _oracle as orc
    import _postcases as pc
    model, W, H, N, start, g, kind = case
    num_parts = orc.model_tables(model)[0]
    mp = 64 if model == 0 else 20
    thr = orc.default_thresholds(model)
    low = pc.fused_case_input(model, W, H, N, start, g, kind)
    res = orc.imresize(low, W, H, start, g)[0]
    peaks = orc.nms(res, num_parts, mp, thr["nms_threshold"])
    n, joints, cand, conn, rows = orc.connect_trace(model, res, peaks, mp, W, H, 1280, 720, thr)
    for a in (low, res, peaks, joints):
        a.setflags(write=False)
    return dict(low=low, res=res, peaks=peaks, n=n, joints=joints[:n], cand=cand, conn=conn, rows=rows, max_peaks=mp, num_parts=num_parts, thr=thr)


def peaks_in_clamp_region(case):
    """peaks of the oracle's NMS whose 7x7 window (the write kernel's centroid window, nms_layer.cu) overlaps the clamp region of the LAST scale"""
    model, W, H, N, start, g, kind = case
    ref = fused_reference(case)
    mask = clamp_mask(W, H, start, g, N - 1)
    hits = 0
    for p in range(ref["num_parts"]):
        for k in range(1, min(int(ref["peaks"][p, 0, 0]), ref["max_peaks"]) + 1):
            x, y = int(round(float(ref["peaks"][p, k, 0]))), int(round(float(ref["peaks"][p, k, 1])))
            hits += bool(mask[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4].any())
    return hits


def kept_paf_samples_in_clamp_region(case):
    """PAF samples of the oracle's ACCEPTED connections (its greedy picks) that lie in the clamp region of the last scale.  COCO at the default
    thresholds only: inter_min_above is 9 of 10 samples, so every sample of an accepted pair scored above inter_threshold and was summed.
    The sample coordinates restate rtpose.cpp:931-947 (postproc.hip connect_pairs): round(s + lm * d / 10) in float32, clamped to the map."""
    import _oracle as orc
    model, W, H, N, start, g, kind = case
    assert model == 0
    ref = fused_reference(case)
    assert ref["thr"]["inter_min_above"] == 9
    limb_seq = orc.model_tables(model)[2]
    mask = clamp_mask(W, H, start, g, N - 1)
    f32 = np.float32
    hits = 0
    for limb, i, j, score in ref["conn"]:
        a, b = ref["peaks"][limb_seq[2 * int(limb)], int(i)], ref["peaks"][limb_seq[2 * int(limb) + 1], int(j)]
        dx, dy = f32(b[0] - a[0]), f32(b[1] - a[1])
        for lm in range(10):
            mx = min(int(np.round(f32(a[0] + f32(f32(lm) * dx) / f32(10)))), W - 1)
            my = min(int(np.round(f32(a[1] + f32(f32(lm) * dy) / f32(10)))), H - 1)
            hits += bool(mask[my, mx])
    return hits

"""The full-batch checks of tests/test_batch_launches.py on the CPU: what their matrix reaches, and that they catch what they are for.

1. Coverage, from rtp_plan_summary (no device): the image counts, the (impl, tile) pairs and the (kind, impl, tile, rowb, passes, pool)
   classes of the batch plans bench.py times (test_precision.CONFIGS with batch_frames > 1), grids that are and are not a multiple of 8 (the
   q / r split of the XCD remap in decode_block) for each of the three MFMA kernels; the ABI surface of rtp_get_batch_blob.
2. The float64 checker over several images per launch: a correct kernel emulated on B * N DIFFERENT images (the first two stages of the 128x32
   plans with batch_frames 2 and 3, every pixel sampled) passes; defects of the kind only a batch can have fail in the images and the class
   they belong to — a frame computed from another frame's input, a grid one workgroup short, a 7x7 halo that reads the previous image's rows,
   two frames' low-res maps swapped; and, over TEN images, an image index that is wrong from the 8th image on (what only a launch of many
   images can have: tests/_manycases.py), sampled as sparsely as on the GPU.
3. The bitwise comparer (tests/_batchcheck.py) reports a single last-bit difference exactly where it was planted."""
import numpy as np
import pytest

import _batchcheck as bc
import _convcheck as cc
import _customnets as cn
import _manycases as mc
import _synth
import test_precision as tp

STOP = "Mconv7_stage2_L2"


def _r():
    import caffe_rtpose_amd as r
    return r


@pytest.fixture(scope="module")
def graphs():
    return {m: cc.builtin_graph(m) for m in (0, 1)}


@pytest.fixture(scope="module")
def batch_plans(graphs):
    r = _r()
    out = {}
    for name, (mode, model, w, h, n, gap, b, seed) in cc.BATCH_MATRIX.items():
        summary = r.plan_summary(cc.batch_config(name))
        out[name] = (mode, graphs[model], n * b, summary, cc.parse_plan(summary)[1])
    return out


def _classes(launches):
    return {(L.kind, L.impl, "%dx%d" % L.tile, L.rowb, L.passes, L.pool) for L in launches if L.kind != "pool"}


def _benched_batch_plans():
    r = _r()
    for cfg, (model, w, h, n, gap, b) in tp.CONFIGS.items():
        if b > 1:
            c = r.Config(model=model, net_w=w, net_h=h, num_scales=n, start_scale=tp.START.get(cfg, 1.0), scale_gap=gap, precision=r.PREC_MIXED,
                         frames_in_flight=b, batch_frames=b, synthetic_seed=tp.SEEDS.get(cfg, 1))
            yield cfg, cc.parse_plan(r.plan_summary(c))[1]


def test_batch_matrix_reaches_the_image_counts_tiles_and_grid_remainders_of_the_benched_batch_plans(batch_plans):
    assert {2, 3, 4, 5, 6} <= {images for _, _, images, _, _ in batch_plans.values()}
    assert all(cc.BATCH_MATRIX[n][6] >= 2 for n in cc.BATCH_MATRIX) and set(cc.BATCH_FLOAT64) <= set(cc.BATCH_MATRIX)
    pairs = {(L.impl, L.tile) for _, _, _, _, la in batch_plans.values() for L in la if L.kind in ("conv", "pw2")}
    mixed = set().union(*[_classes(la) for mode, _, _, _, la in batch_plans.values() if mode == "mixed"])
    benched, benched_cfgs = set(), []
    for cfg, la in _benched_batch_plans():
        benched_cfgs.append(cfg)
        missing = {(L.impl, L.tile) for L in la if L.kind in ("conv", "pw2")} - pairs
        assert not missing, (cfg, missing)
        benched |= _classes(la)
    assert {"coco_1s_b2", "coco_3s_b2", "mpi_1s_b2", "mpi_1s_b5"} <= set(benched_cfgs)
    print(f"\n{len(benched)} classes in the benched batch plans, {len(mixed)} in the mixed cases of the batch matrix")
    assert not benched - mixed, benched - mixed
    # the class the first nine cases do not reach is what the last one is there for
    lone = ("conv", "ring", "128x128", 128, "1", False)
    first_nine = set().union(*[_classes(batch_plans[n][4]) for n in list(cc.BATCH_MATRIX)[:9] if batch_plans[n][0] == "mixed"])
    assert lone in benched and benched - first_nine == {lone} and lone in _classes(batch_plans["mixed_coco_192x304_3s_b2"][4])
    # grids that are and are not a multiple of 8 workgroups, per kernel: the q / r split of the XCD remap
    for impl in ("ring", "reg", "pw2"):
        rem = {L.wgs % 8 == 0 for _, _, _, _, la in batch_plans.values() for L in la if L.impl == impl}
        assert rem == {True, False}, (impl, rem)
    # what the issue names per case
    la = {n: p[4] for n, p in batch_plans.items()}
    assert any(L.tile == (128, 128) for L in la["mixed_coco_176x320_2s_b2"])
    assert any(L.kind == "pool" for L in la["mixed_mpi_96x64_b5"]) and any(L.kind == "pw2" and L.wgs % 8 for L in la["mixed_mpi_96x64_b5"])
    assert any(L.impl == "reg" and L.wgs % 8 and L.passes in ("3aw", "2w") for L in la["f16x3_coco_144x80_b2"])
    assert {(64, 128), (64, 64), (128, 64)} <= {L.tile for L in la["fp32_coco_160x96_2s_b2"] if L.impl == "reg"}


def test_batch_tap_is_exported_and_refuses_a_null_engine():
    """the ABI surface of rtp_get_batch_blob without a GPU"""
    import ctypes as C
    from caffe_rtpose_amd import _lib
    r = _r()
    assert hasattr(_lib.lib, "rtp_get_batch_blob") and "rtp_get_batch_blob" in _lib.SIGNATURES
    assert hasattr(r.Engine, "get_batch_blob")
    shape, tags, nf = (C.c_int * 4)(), (C.c_uint64 * 4)(), C.c_int(-7)
    assert _lib.lib.rtp_get_batch_blob(None, 0, b"concat_stage7", None, 0, shape, tags, C.byref(nf)) == r.RTP_EINVAL
    assert _lib.lib.rtp_get_batch_blob(None, 0, None, None, 0, None, None, None) == r.RTP_EINVAL
    assert nf.value == -7 and list(shape) == [0, 0, 0, 0]          # a refused call writes nothing
    assert _lib.lib.rtp_get_blob(None, b"concat_stage7", None, 0, shape) == r.RTP_EINVAL


# ------------------------------------------------------------------------------------------------------------
# the float64 checker over the images of a batch
# ------------------------------------------------------------------------------------------------------------
class _BatchToy:
    """the first stages of a built-in plan with batch_frames B on B DIFFERENT one-image frames, emulated launch by launch"""
    def __init__(self, graph, mode, B, W=128, H=32, stop=STOP):
        r = _r()
        self.graph, self.B = graph, B
        prec = {"f16x3": r.PREC_F16X3, "fp16": r.PREC_FP16, "mixed": r.PREC_MIXED}[mode]
        self.summary = r.plan_summary(r.Config(net_w=W, net_h=H, precision=prec, frames_in_flight=B, batch_frames=B))
        last = list(graph.convs).index(stop)
        self.weights = {n: r.synth_weights(1, n, c["cout"], graph.channels[c["bottom"]], c["k"]) for n, c in list(graph.convs.items())[:last + 1]}
        self.frame = np.concatenate([_synth.random_frame(1, H, W, seed=3 + j) for j in range(B)])
        assert not np.array_equal(self.frame[0], self.frame[1])
        self.em = cc.Emulation(self.summary, graph, self.weights, self.frame, stop_after=stop)
        self.launch = {n: L for L in self.em.launches for n in L.layers + L.layers2}
        self.levels = self.em.levels

    def check(self, only=None, n_interior=10 ** 9):
        names = list(self.weights) + list(self.graph.pools) if only is None else only
        return cc.check_plan(self.summary, self.graph, self.weights, self.em.blob, n_interior=n_interior, only=names, images_per_launch=self.B)

    def plant(self, name, v, **kw):
        L = self.launch[name]
        assert L.kind in ("conv", "first")
        self.em.finish(L, name, v)
        rep = self.check([name], **kw)
        self.em.finish(L, name, self.em.pre[name])
        assert len(rep) == 1 and self.check([name])[0].nfail == 0
        return rep[0]


@pytest.fixture(scope="module")
def toys(graphs):
    made = {}

    def get(mode, B, **kw):
        key = (mode, B, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = _BatchToy(graphs[0], mode, B, **kw)
        return made[key]
    return get


@pytest.mark.parametrize("mode,B", [("mixed", 2), ("f16x3", 3)])
def test_emulated_correct_kernel_passes_every_launch_of_a_batch_of_different_images(toys, mode, B):
    t = toys(mode, B)
    reps = t.check()
    assert len(reps) == 24 and all(rep.nchecked > 0 for rep in reps)
    for rep in reps:      # every pixel of every image of the batch
        if rep.launch.kind != "pool":
            lvl = t.graph.level[t.graph.convs[rep.launch.layers[0]]["bottom"]]
            hh, ww, _ = t.levels[lvl]
            assert rep.npixels == B * len(rep.launch.layers) * (hh * ww // (4 if rep.launch.pool else 1)), rep.launch
    print(f"\n[{mode} b{B}] worst |err|/tol {max(rep.worst for rep in reps):.3f}")
    bad = [str(f) for rep in reps for f in rep.failures]
    assert not bad, bad[:5]


def test_planted_frame_computed_from_the_input_of_frame_0(toys):
    """image index taken modulo N: the launch computes every frame's images from frame 0's"""
    t = toys("f16x3", 3)
    name = "conv2_1"
    v = t.em.pre[name].copy()
    v[1:] = v[:1]
    rep = t.plant(name, v)
    assert rep.nfail > 0 and {f.img for f in rep.failures} == {1, 2} and all(f.layer == name for f in rep.failures), [str(f) for f in rep.failures]


def test_planted_grid_one_workgroup_short(toys):
    """the last tile of the last image keeps what an earlier batch left there.  Shape: 64x112, where a 128-pixel tile of the 1/4-resolution level spans
    seven rows, so that the last tile begins above the rows that are checked in full — only its own end pixels can see it there"""
    t = toys("f16x3", 2, W=64, H=112, stop="conv3_3")
    found = None
    for name, L in t.launch.items():
        if L.kind != "conv" or L.pool:
            continue
        hh, ww, halo = t.levels[t.graph.level[t.graph.convs[name]["bottom"]]]
        ends, nt = cc.plain_tile_ends(hh, ww, halo, L.tile[0])
        y0, x0 = ends[-2]
        if y0 < hh - cc.BORDER and cc.BORDER <= x0 < ww - cc.BORDER:
            found = (name, L, hh, ww, halo, nt, (y0, x0))
            break
    assert found, "no launch of this plan whose last tile begins outside the border rows"
    name, L, hh, ww, halo, nt, first = found
    Wp = ww + halo
    m = np.arange((nt - 1) * L.tile[0], hh * Wp)
    m = m[(m % Wp >= halo) & (m % Wp < halo + ww)]
    ys, xs = m // Wp, m % Wp - halo
    v = t.em.pre[name].copy()
    v[-1][:, ys, xs] = t.em.pre[name][0][:, ys, xs] + np.float32(0.5)          # stale: the previous batch's values
    rep = t.plant(name, v, n_interior=0)                                        # borders and tile ends only, as on the GPU
    tile = set(zip(ys.tolist(), xs.tolist()))
    assert rep.nfail > 0 and {f.img for f in rep.failures} == {t.B - 1} and all((f.y, f.x) in tile for f in rep.failures), [str(f) for f in rep.failures]
    by_class = {cls: nf for (dest, cls), (n, nf, worst) in rep.by_class.items()}
    # Report.failures keeps the worst eight per image: the class counts say where the rest fell.  Above the border rows the tile's first pixel is the
    # only pixel of the tile that is sampled, and it is sampled as a tile end: 0 < failures there <= its channels
    assert first[0] < hh - cc.BORDER and 0 < by_class["tile end"] <= t.graph.convs[name]["cout"] and by_class["border"] > 0 and "interior" not in by_class


def test_planted_7x7_halo_rows_read_from_the_previous_image(toys):
    """images are adjacent in the arena: a 7x7 layer whose zero rows above image n were missing reads the bottom rows of image n - 1"""
    t = toys("f16x3", 3)
    name = "Mconv1_stage2_L1"
    L = t.launch[name]
    assert L.k == 7 and L.passes == "3aw"
    a_hi, a_lo = t.em.operand(t.graph.convs[name]["bottom"])
    ext = lambda a: np.concatenate([np.concatenate([np.zeros_like(a[:1, :, -3:]), a[:-1, :, -3:]]), a], axis=2)     # the previous image's last 3 rows on top
    wrong = t.em.gemm(name, "3aw", ext(a_hi), ext(a_lo))[:, :, 3:]
    v = t.em.pre[name].copy()
    v[:, :, :3] = wrong[:, :, :3]
    v[0] = t.em.pre[name][0]                                 # image 0 has zeros above it either way
    rep = t.plant(name, v)
    assert rep.nfail > 0 and {f.img for f in rep.failures} == {1, 2} and {f.cls for f in rep.failures} == {"border"}, [str(f) for f in rep.failures]
    assert all(f.layer == name and f.y < 3 for f in rep.failures)


def test_planted_image_index_wrong_from_the_8th_image_on(toys):
    """img = (tile / tiles_per_img) & 7: images 8 and 9 of a launch of ten are computed from images 0 and 1.  Nothing below nine images per launch
    can show it — the matrices of tests/test_batch_launches.py stopped at six.  Sampled as on the GPU (128 // images interior pixels per image)."""
    B = 10
    t = toys("fp16", B, W=64, H=32, stop="conv2_2")
    assert t.frame.shape[0] == B and all(not np.array_equal(t.frame[i], t.frame[i & 7]) for i in (8, 9))
    reps = t.check(only=list(t.weights) + [p for p in t.graph.pools if p in t.em.hi], n_interior=128 // B)
    print([repr(rep.launch) for rep in reps])
    assert len(reps) >= 4 and not [str(f) for rep in reps for f in rep.failures]      # conv1_1 .. conv2_2 and the pooling that the plan has materialised
    for name in ("conv1_1", "conv2_1"):
        v = t.em.pre[name].copy()
        v[8:] = v[:2]
        rep = t.plant(name, v, n_interior=128 // B)
        assert rep.nfail > 0 and {f.img for f in rep.failures} == {8, 9} and all(f.layer == name for f in rep.failures), [str(f) for f in rep.failures]
        v = t.em.pre[name].copy()
        v[:8] = np.roll(v[:8], 1, axis=0)                                              # (the first eight alone: a defect the older matrices could see)
        rep = t.plant(name, v, n_interior=128 // B)
        assert rep.nfail > 0 and {f.img for f in rep.failures} == set(range(8))
    # the bitwise comparer names the first wrong image of such a batch too
    blob = t.em.blob("conv2_1")
    singles = [blob[i:i + 1] for i in range(B)]
    bad = blob.copy()
    bad[8:] = bad[:2]
    d = bc.compare_blob("conv2_1", bad, singles, 1)
    assert d is not None and (d.frame, d.image) == (8, 8) and bc.compare_blob("conv2_1", blob, singles, 1) is None


def test_many_image_batch_cases_are_what_they_are_named_for():
    """tests/_manycases.py BATCH_MATRIX: (a) at least 10 images per launch from many scales at batch_frames 2, on the ring kernel's 64x128 tile;
    (b) 32 images per launch; (c) batch_frames 16 at one scale — and the float64 cases are among them"""
    r = _r()
    t = mc.BATCH_MATRIX
    plans = {n: cc.parse_plan(r.plan_summary(cc.batch_config(n, matrix=t)))[1] for n in t}
    a, b, c = t["fp16_coco_96x64_5s_b2"], t["mixed_coco_64x48_16s_b2"], t["mixed_coco_64x48_b16"]
    assert a[4] * a[6] >= 10 and a[6] == 2 and any(L.impl == "ring" and L.tile == (64, 128) for L in plans["fp16_coco_96x64_5s_b2"])
    assert (b[4], b[6]) == (16, 2) and (c[4], c[6]) == (1, 16) and b[2:4] == c[2:4] == (64, 48)
    assert set(mc.BATCH_FLOAT64) <= set(t) and len(t) == 3
    for n, la in plans.items():               # every launch of a case holds all its images: wgs is a multiple of the image count
        assert all(L.wgs % (t[n][4] * t[n][6]) == 0 for L in la if L.kind != "pool"), n


def test_planted_swap_of_the_low_res_maps_of_two_frames():
    """the planar low-res store of frame 1 at frame 0's offset and the other way round: every tensor is right, the final maps are not"""
    r = _r()
    gname, mode, B = "pw", "mixed", 2
    graph = cn.net(gname)[1]
    summary = r.plan_summary(cn.config(gname, mode, 64, 48, 1, B))
    weights = {n: r.synth_weights(1, n, c["cout"], graph.channels[c["bottom"]], c["k"]) for n, c in graph.convs.items()}
    frame = np.concatenate([_synth.random_frame(1, 48, 64, seed=3 + j) for j in range(B)])
    em = cc.Emulation(summary, graph, weights, frame)
    names = list(weights) + list(graph.pools)
    check = lambda blob: cc.check_plan(summary, graph, weights, blob, n_interior=10 ** 9, only=names, images_per_launch=B)
    assert not [str(f) for rep in check(em.blob) for f in rep.failures]
    reps = check(lambda nm: em.blob(nm)[::-1] if nm == graph.lowres else em.blob(nm))
    fails = [f for rep in reps for f in rep.failures]
    assert fails and {f.dest for f in fails} == {graph.lowres} and {f.img for f in fails} == {0, 1}, [str(f) for f in fails[:5]]
    assert all(rep.launch.lowres for rep in reps if rep.nfail)


# ------------------------------------------------------------------------------------------------------------
# the bitwise comparer
# ------------------------------------------------------------------------------------------------------------
def test_bitwise_comparer_reports_one_planted_last_bit():
    rs = np.random.RandomState(5)
    N, B = 2, 3
    singles = [{"a": rs.randn(N, 5, 6, 7).astype(np.float32), "low": rs.randn(N, 3, 2, 4).astype(np.float32)} for _ in range(B)]
    blobs = {k: np.concatenate([s[k] for s in singles]) for k in ("a", "low")}
    assert bc.compare_batch(blobs, singles, N) == ([], {"a": 0, "low": 0})
    bad = blobs["a"].copy()
    bad[3, 4, 1, 6] = np.nextafter(bad[3, 4, 1, 6], np.float32(np.inf))          # one unit in the last place, in frame 1's second image
    diffs, counts = bc.compare_batch({"a": bad, "low": blobs["low"]}, singles, N)
    assert counts == {"a": 1, "low": 0} and len(diffs) == 1
    d = diffs[0]
    assert (d.blob, d.frame, d.image, d.channel, d.y, d.x, d.count) == ("a", 1, 3, 4, 1, 6, 1)
    assert d.got == float(bad[3, 4, 1, 6]) and d.want == float(singles[1]["a"][1, 4, 1, 6]) and d.got != d.want
    assert "frame 1 image 3 channel 4 pixel (y 1, x 6)" in str(d)
    # several differences: the first in memory order is reported, all are counted, per blob
    bad2 = bad.copy()
    bad2[5, 0, 0, 0] += 1.0
    low2 = blobs["low"].copy()
    low2[0, 0, 0, 0] = np.nan
    diffs, counts = bc.compare_batch({"a": bad2, "low": low2}, singles, N)
    assert counts == {"a": 2, "low": 1} and [(d.blob, d.frame, d.image) for d in diffs] == [("a", 1, 3), ("low", 0, 0)]
    # equal as numbers, different bits: -0.0 against 0.0 is a difference here; the same NaN bits on both sides still are (np.array_equal's answer)
    z = [{"a": np.zeros((1, 1, 1, 2), np.float32)}]
    neg = np.array([[[[0.0, -0.0]]]], np.float32)
    assert bc.compare_batch({"a": neg}, z, 1)[1] == {"a": 1}
    nan = [{"a": np.full((1, 1, 1, 1), np.nan, np.float32)}]
    assert bc.compare_batch({"a": nan[0]["a"].copy()}, nan, 1)[1] == {"a": 1}
    with pytest.raises(AssertionError):       # a batch blob with the wrong image count
        bc.compare_blob("a", blobs["a"][:-1], [s["a"] for s in singles], N)

"""Per-launch check of the convolution stack against float64, element by element — TEST INFRASTRUCTURE (numpy / torch-CPU only).

What is checked.  rtp_plan_summary lists one `step` line per kernel launch.  Every launch is taken ALONE: its input is the
engine's own blob (read back after one forward; the export returns hi + lo / fp8 parts summed), converted to float64, so the
error of everything upstream never enters the tolerance.  At a sparse set of output pixels (all channels) the launch is
recomputed in float64 — one gather of input patches, one matmul — and every destination blob of the launch (its own tensor,
the concat slices at their channel offset, the pooled blob, the final low-res maps) is compared element by element with

    r = relu(b + sum a*w)            S = |b| + sum |a||w|
    tol = u_out*|r| + (c_acc*2^-24 + e_op)*S + e_abs + a_min

Sampled pixels, per image: every pixel of the first and last 4 rows and columns (the 7x7 halo is 3), the first and last
pixel of EVERY workgroup's tile (plan.h: plain_tiles_per_img over the flat H x Wp walk; the 2-row x BM/2 walk with pitch
pool_wq of the pooling epilogue, restated from tests/test_design_invariants.py), and a seeded random interior set.

The constants, each with its derivation (u = 2^-24, the fp32 unit roundoff):

u_out / a_min — how the stored value differs from the kernel's fp32 value v (conv_common.h conv_store_dst):
  fp32 plan              u_out 2^-24 (bias add / final rounding), a_min 2^-126 per K term is folded into e_abs (flushed subnormals)
  fp16 tensor, hi only   u_out 2^-11 (round to nearest, 11 significant bits), a_min 2^-24 (smallest fp16 subnormal)
  ... with a lo part     the export returns hi + fp16(v - hi): |v - hi| <= 2^-11|v| rounded to 11 bits -> 2^-22|v|, plus the fp32 add
                         of the export 2^-24|v|: u_out 2^-22 + 2^-24, a_min 2^-24 (lo below the fp16 normal range)
  ... with a q part      hi + e4m3(lo * 2^12) / 2^12: 3 mantissa bits -> 2^-4 of |lo| <= 2^-11|v|: u_out 2^-15 + 2^-23, a_min 2^-22 (half an
                         e4m3 subnormal step 2^-9 / 2^12 / 2); lo * 2^12 saturates at 448 for |v| > 224: there the hi-only bound applies
  ... with lo AND q      (a tensor read by a register-staged 1x1 layer, label 3aw, and by a ring layer, label 2q) the export returns hi + lo
                         (kernels.h launch_export: the q block is added only where there is no lo block): u_out and a_min of the lo case
  final low-res maps     fp32 planar stores of v itself: u_out 2^-24 — whether a concat of convolutions or ONE convolution is what ImResize reads
  Which parts a tensor carries follows from its consumers' pass labels (plan.cpp propagate_split): a consumer with `q` needs the q
  block, one with `a` the lo block; a pooling layer hands its output's needs to its input.

c_acc — fp32 roundings on the longest accumulation chain of one output element.  An MFMA adds the sum of its K products to the
accumulator: one rounding of the running sum per instruction (bounded by u*S each), and the roundings INSIDE the instructions, whatever their
order, are bounded by (K-1)*u times the instruction's own terms, i.e. by (K-1)*u*S summed over all instructions.
  conv_ring.hip / conv_igemm.hip   taps (k_eff^2) x chunks of one pass (cin_p*elem/rowb) x passes x (rowb/32)/KSPLIT instructions per chunk
                                   [fp16: v_mfma_f32_32x32x16_f16, one per 32-byte k-group; fp32: four 32x32x2 per k-group; a q chunk: one fp8
                                   32x32x64 per two k-groups], + 15 inside the fp16 instructions (16 exact products) / + 2 for fp32 (product and
                                   pair sum) / + 1 for the fp8 instructions (63 roundings on terms 2^-11 of S), + KSPLIT-1 for the reduction of
                                   the k-split partials in the epilogue, + 1 for the bias add.  KSPLIT: 128x128 1, 64x128 / 128x64 / 128x32 2,
                                   64x64 4 (2 for the fp8-compensated ring kernel with 128-byte chunks)  [ring_launch_cfg, launch_cfg]
                                   a 1x1 layer on the register-staged kernel (conv_igemm.hip launch_cfg<T, 1, 128>): one tap, cin_p/64 chunks of 128
                                   bytes, 4 / 2 / 1 instructions per chunk and wave on 128x128 / 64x128 / 64x64 (KSPLIT 1 / 2 / 4), e.g. cin_p 192
                                   label 3aw: 3 chunks x 3 passes x (4 | 2 | 1) = 36 | 18 | 9, + 15 + (0 | 1 | 3) + 1 = 52 | 35 | 28
  conv_first.hip                   2 instructions (K = 32 taps, 27 real) starting from the bias as the initial accumulator, + 15
  conv_pw2.hip                     GEMM1: 8 instructions (K = 128) x passes + 15 + 1 (bias); GEMM2: (mid/128) x 8 x passes + 15 + 1 (bias)

e_op — what the operands of the launch differ from the reference's (pass label of the summary):
  `1`                  reference operands ARE the kernel's: float16(w) and float16(a) on fp16 plans (a tensor's lo part is not read), fp32 as is: 0
  `w` (2w, 3aw)        reference uses the fp32 master weights; the kernel W_hi + fp16(W - W_hi): residue 2^-22|W| (+ 2^-25 per term where W_lo is subnormal: e_abs)
  `a` (2a, 3aw)        reference uses the exported hi + lo, an fp32 sum: 2^-24|a|
  `aw`                 + the dropped a_lo x W_lo product: 2^-11 * 2^-11 = 2^-22
  `2q`                 DESIGN.md section 2: a_hi*W_hi + l8*Q(W_hi) + Qa(a_hi)*Q(W_lo) with l8 the stored e4m3(lo*2^12)/2^12 (the export returns
                       a_hi + l8), Q(x) = e4m3(x*2^t)/2^t resp. 2^(t+11), Qa(x) = e4m3(4x)/4, t = floor(log2(448 / max|W| of the launch)).
                       reference - kernel = l8*(W_hi - Q(W_hi)) + (a_hi - Qa(a_hi))*W_lo + Qa(a_hi)*(W_lo - Q(W_lo)) + l8*W_lo, with |l8| <= 2^-11|a|,
                       |W_lo| <= 2^-11|W|, e4m3 relative error 2^-4 and half a subnormal step 2^-10 in the scaled domain:
                       (2^-15 + 2^-15 + (1 + 2^-4)*2^-15 + 2^-22)|a||W| = (3*2^-15 + 2^-19 + 2^-22)|a||W| ~ 2^-13.4, times (1 + 2^-10) for |a_hi|, |W_hi|
                       against |a|, |W|; e_abs = (2 + 2^-4)*2^-21-t * sum|a| + 2^-23 * sum|W|.  Qa saturates at |a| = 112: checked, not assumed.
  `2q` on a lo + q input  the export returns a_hi + lo, the kernel reads l8: reference - kernel gains (lo - l8)*W.  Both round the same d = v - a_hi,
                       |d| <= 2^-11|v|: |lo - d| <= 2^-11|d| + 2^-25, |l8 - d| <= 2^-4|d| + 2^-22, and the export's fp32 sum a_hi + lo rounds once
                       (2^-24|a|): e_op + (2^-15 + 2^-22 + 2^-24)(1 + 2^-10), e_abs + (2^-22 + 2^-25) * sum|W|

Beyond the e4m3 ranges (saturating=True; `2q` launches only).  The assertion |a| < 112 is replaced by four per-element terms, each computed from
the launch's actual operands and each exactly 0 where the condition it is named for does not occur, so that every case inside the ranges keeps
its bound bit for bit.  In the decomposition of the `2q` line above:
  activation saturation   e4m3(4x) ends at 448, the clamp in front of the conversion holds larger values there: Qa(a_hi) = +-112 for |a_hi| >= 112 and
                       a_hi - Qa(a_hi) = +-(|a_hi| - 112) instead of at most 2^-4|a_hi|.  The dropped part of the a_hi*W_lo correction is therefore
                       relu(|a_hi| - 112) @ |W - f16(W)|  (the true W_lo, no bound on it).  a_hi is not exported, a = a_hi + l8 (or + lo) is:
                       |l8| <= half a step of a_hi, so f16(a) = a_hi unless a lies exactly midway between two fp16 values; then a_hi is f16(a) or its
                       mirror image 2a - f16(a), and the larger magnitude of the two is taken (_abs_hi).  The other terms of the 2q line only get
                       smaller (|Qa(a_hi)| <= 112 < |a_hi|).
  a lo + q input          the export returns a_hi + lo, the kernel reads l8 = e4m3(clamp(d * 2^12)) / 2^12, d = v - a_hi: beyond |d| = 448 / 4096 (from
                       |v| = 256 on, where half a step of fp16 is 1/8) |l8 - d| = |d| - 448/4096 instead of 2^-4|d|.  x = |a - f16(a)| is |lo| up to the
                       rounding of the export's fp32 sum (2^-24|a|), and |lo - d| <= 2^-11|d| + 2^-25: |d| <= (x + 2^-24|a| + 2^-25)(1 + 2^-10) =: d+.
                       Added: relu(d+ - 448/4096) @ |W|.  The slack inside d+ (2^-10 x + 2^-24|a| + 2^-25) acts only where x is within 2^-9 of
                       448/4096, i.e. from |a| = 256 on: 0 below.
  fp16-subnormal W_hi     the 2q line takes |W_lo| <= 2^-11|W|; below the fp16 normal range (|W| < 2^-14) W_lo = W - f16(W) is up to 2^-25 whatever |W| is.
                       With E = relu(|W - f16(W)| - 2^-11|W|) (0 for every normal weight: the spacing of fp16 is a power of two times 2^-10) the three
                       terms that hold W_lo gain (2^-4 + (1 + 2^-4)*2^-4 + 2^-11)(1 + 2^-10) |a| @ E.  (A He weight set holds a few weights below 2^-14: on it
                       this term moves a launch's bound by 2 parts in 10^6; the other three are exactly 0 there.)
  W_lo8 saturation        e4m3(W_lo * 2^(t+11)) ends at 448.  |W_lo| <= 2^-11 max|W| <= 448 * 2^-(t+11) holds while some W_hi of the launch is normal and t is
                       not clamped; with every weight below 2^-14, or t clamped at 40 (max|W| < 448 * 2^-41: W_hi = 0, W_lo = W), it does not.  Added:
                       min((1 + 2^-4)|a_hi|, 112) @ relu(|W - f16(W)| - 448 * 2^-(t+11)).  (W_hi8 = e4m3(W_hi * 2^t) cannot saturate: t is chosen for it;
                       t clamped at -20 needs max|W| > 2^28, which this project does not support.)
The output side needs nothing new: out_rounding bounds a q block above |v| = 224 by the hi part alone.  All of this holds below the fp16 overflow:
a value beyond 65504 is stored as infinity, and what the engine computes from there on is outside every bound here.

`+pool` launches: the kernel takes the maximum of the four fp32 sums, then bias / ReLU / rounding (monotone); |max x~ - max x| <= max |x~ - x|,
so the accumulation part of the tolerance is the largest of the four.  Stand-alone pooling steps move values: they must be EQUAL.
`pw2` launches: the middle blob never leaves LDS; h = relu(b1 + x*w1) is recomputed with its own bound t1 (u = 2^-11, or 2^-22 where the
second GEMM reads a lo part), and the second stage's bound is computed on |h| + t1 with t1 * sum|w2| added.
"""
import re
from collections import OrderedDict

import numpy as np

U32 = 2.0 ** -24
BORDER = 4            # rows / columns at every image edge that are checked in full (the 7x7 halo is 3)
CHUNK = 4096          # sampled pixels per gather + matmul


# ------------------------------------------------------------------------------------------------------------
# the graph, from the deploy prototxt of the built-in model
# ------------------------------------------------------------------------------------------------------------
class Graph:
    def __init__(self, text):
        self.convs = OrderedDict()   # name -> dict(bottom, cout, k, relu)
        self.pools = OrderedDict()   # top -> bottom
        self.concats = OrderedDict() # top -> [bottoms]
        self.lowres = None
        self.input = re.search(r'^input:\s*"([^"]+)"', text, re.M).group(1)
        for body in self._layers(text):
            f = lambda key: re.findall(r'\b%s:\s*"?([^"\s]+)"?' % key, body)
            name, typ, bottoms, tops = f("name")[0], f("type")[0], f("bottom"), f("top")
            if typ == "Convolution":
                self.convs[name] = dict(bottom=bottoms[0], cout=int(f("num_output")[0]), k=int(f("kernel_size")[0]), relu=False)
                assert tops == [name]
            elif typ == "ReLU":
                assert bottoms == tops and bottoms[0] in self.convs
                self.convs[bottoms[0]]["relu"] = True
            elif typ == "Pooling":
                self.pools[tops[0]] = bottoms[0]
            elif typ == "Concat":
                self.concats[tops[0]] = bottoms
            elif typ == "ImResize":
                self.lowres = bottoms[0]
        self.channels, self.level = {self.input: 3}, {self.input: 0}
        for body in self._layers(text):   # blob shapes, in layer order
            name = re.findall(r'\bname:\s*"([^"]+)"', body)[0]
            if name in self.convs:
                c = self.convs[name]
                self.channels[name], self.level[name] = c["cout"], self.level[c["bottom"]]
            elif name in self.concats:
                self.channels[name] = sum(self.channels[b] for b in self.concats[name])
                self.level[name] = self.level[self.concats[name][0]]
            for top, bot in self.pools.items():
                if bot in self.level and top not in self.level:
                    self.channels[top], self.level[top] = self.channels[bot], self.level[bot] + 1

    @staticmethod
    def _layers(text):
        out, depth, start = [], 0, None
        for m in re.finditer(r"layer\s*\{|\{|\}", text):
            tok = m.group(0)
            if tok.startswith("layer") and depth == 0:
                depth, start = 1, m.end()
            elif tok == "{":
                depth += 1
            elif tok == "}" and depth:
                depth -= 1
                if depth == 0:
                    out.append(text[start:m.start()])
        return out

    def dests(self, conv):
        """[(blob, channel offset)] a convolution's output goes to, reference channel order: its own blob, then every concat that lists it."""
        d = [(conv, 0)]
        for top, bots in self.concats.items():
            off = 0
            for b in bots:
                if b == conv:
                    d.append((top, off))
                off += self.channels[b]
        return d


def builtin_graph(model):
    import os
    import tempfile
    import caffe_rtpose_amd as r
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "net.prototxt")
        r.write_builtin_prototxt(model, p)
        with open(p) as f:
            return Graph(f.read())


# ------------------------------------------------------------------------------------------------------------
# the plan, from rtp_plan_summary
# ------------------------------------------------------------------------------------------------------------
class Launch:
    def __init__(self, **kw):
        self.pool = False; self.layers2 = []; self.mid = 0; self.dsts = 1; self.lowres = 0; self.impl = "-"; self.rowb = 0
        self.tile = (0, 0); self.cin_p = 0; self.k = 0; self.passes = "1"; self.wgs = 0; self.coutp = 0
        self.__dict__.update(kw)

    @property
    def key(self):
        """The kernel instantiation: step kind, single / paired, +pool, k, cin_p, tile, rowb, pass label, ring / reg, several destinations, low-res output (+ mid for pw2)."""
        return (self.kind, len(self.layers), self.pool, self.k, self.cin_p, "%dx%d" % self.tile, self.rowb, self.passes, self.impl, self.dsts > 1, bool(self.lowres), self.mid)

    def __repr__(self):
        return f"{self.kind} {' + '.join(self.layers)}" + (f" -> {' + '.join(self.layers2)}" if self.layers2 else "")


def key_str(key):
    kind, n, pool, k, cin_p, tile, rowb, passes, impl, multi, low, mid = key
    return (f"{kind}{' pair' if n == 2 else ''}{' +pool' if pool else ''} k {k} cin_p {cin_p}" + (f" mid {mid}" if mid else "") +
            f" tile {tile} rowb {rowb} passes {passes} {impl}{' dsts>1' if multi else ''}{' lowres' if low else ''}")


def parse_plan(summary):
    """(levels [(H, W, halo)], launches) of an rtp_plan_summary text.  `step pack` is no launch of its own here: it feeds the 1x1 route of conv1_1."""
    levels, launches = [], []
    for ln in summary.splitlines():
        w = ln.split()
        if ln.startswith("level "):
            levels.append((int(w[3]), int(w[5]), int(w[7])))
        if not ln.startswith("step ") or w[1] == "pack":
            continue
        val = lambda name: w[w.index(name) + 1]
        if w[1] == "first":
            launches.append(Launch(kind="first", layers=[w[2]], k=3, cin_p=3, passes=val("passes"), wgs=int(val("wgs"))))
        elif w[1] == "pool":
            launches.append(Launch(kind="pool", layers=[], pool_in=w[2], pool_out=w[4]))
        elif w[1] == "pw2":
            arrow, kpos = w.index("->"), w.index("k")
            names = lambda part: [t for t in part if t != "+"]
            tile = int(val("tile"))
            launches.append(Launch(kind="pw2", layers=names(w[2:arrow]), layers2=names(w[arrow + 1:kpos]), k=1, cin_p=int(val("cin_p")), mid=int(val("mid")),
                                   passes=val("passes"), tile=(tile, 64), coutp=64, wgs=int(val("wgs")), lowres=int(val("lowres")), impl="pw2"))
        else:
            kpos = w.index("k")
            names = [t for t in w[2:kpos] if t not in ("+", "+pool")]
            bm, bn = val("tile").split("x")
            launches.append(Launch(kind="conv", layers=names, pool="+pool" in w[2:kpos], k=int(val("k")), cin_p=int(val("cin_p")), coutp=int(val("coutp")),
                                   tile=(int(bm), int(bn)), rowb=int(val("rowb")), passes=val("passes"), impl=val("impl"), wgs=int(val("wgs")),
                                   dsts=int(val("dsts")), lowres=int(val("lowres"))))
    return levels, launches


def plan_keys(summary, graph=None):
    """instantiation keys of a plan (pw2 launches: several destinations where the graph says so)"""
    _, launches = parse_plan(summary)
    for L in launches:
        if L.kind == "pw2" and graph is not None:
            L.dsts = _pw2_dsts(graph, L)
    return {L.key for L in launches}


def _pw2_dsts(graph, L):
    """tensors the second layer of a pw2 launch stores to: its own and the concat slices (the low-res maps are no tensor)"""
    return 1 + len([d for d in graph.dests(L.layers2[0])[1:] if d[0] != graph.lowres])


def tensor_parts(graph, launches):
    """blob -> 'lo' / 'q' / 'lo+q' / '' : which split-precision blocks its tensor carries, from the consumers' pass labels (plan.cpp propagate_split)."""
    need = {}
    for L in launches:
        if L.kind in ("conv", "pw2", "first"):
            lab = L.passes.split("/")[0]
            for name in L.layers:
                bottom = graph.convs[name]["bottom"]
                if "q" in lab:
                    need.setdefault(bottom, set()).add("q")
                elif "a" in lab[1:]:
                    need.setdefault(bottom, set()).add("lo")
    for top, bot in reversed(list(graph.pools.items())):
        if need.get(top):
            need.setdefault(bot, set()).update(need[top])
    return {b: "+".join(sorted(n)) for b, n in need.items()}


# ------------------------------------------------------------------------------------------------------------
# tile walks (plan.h) and the sample set
# ------------------------------------------------------------------------------------------------------------
def plain_tile_ends(H, W, halo, BM):
    """first and last interior pixel (y, x) of every tile of BM flat pixels over H x Wp, and the tile count (plan.h plain_tiles_per_img)."""
    Wp = W + halo
    ntiles = (H * Wp + BM - 1) // BM
    m = np.arange(H * Wp)
    ok = (m % Wp >= halo) & (m % Wp < halo + W)
    ends = []
    for t in range(ntiles):
        v = m[t * BM:(t + 1) * BM][ok[t * BM:(t + 1) * BM]]
        if len(v):
            ends += [(int(v[0] // Wp), int(v[0] % Wp - halo)), (int(v[-1] // Wp), int(v[-1] % Wp - halo))]
    return ends, ntiles


def pool_tile_ends(H, W, k, BM):
    """first and last POOLED pixel (y, x) of every tile of the pooling epilogue's walk: 2 image rows x BM/2 pixels with pitch pool_wq
    (conv_common.h conv_epilogue_pool; tests/test_design_invariants.py restates the same walk)."""
    HALF = BM // 2
    Wq = (W + k // 2 + 1) & ~1
    ntiles = ((H // 2) * Wq + HALF - 1) // HALF
    ends = []
    for t in range(ntiles):
        v = []
        for j in range(HALF // 2):
            pair, x = divmod(t * HALF + 2 * j, Wq)
            if pair < H // 2 and x < W:
                v.append((pair, x // 2))
        if v:
            ends += [v[0], v[-1]]
    return ends, ntiles


def sample_pixels(H, W, tile_ends, n_interior, rs):
    """(ys, xs, cls) with cls 0 border / 1 tile end / 2 interior; every pixel once, the first class that names it wins."""
    cls = np.full((H, W), -1, np.int8)
    if n_interior >= H * W:
        cls[:] = 2
    elif n_interior > 0:
        idx = rs.choice(H * W, size=n_interior, replace=False)
        cls.reshape(-1)[idx] = 2
    for y, x in tile_ends:
        cls[y, x] = 1
    b = min(BORDER, H, W)
    cls[:b, :] = 0; cls[-b:, :] = 0; cls[:, :b] = 0; cls[:, -b:] = 0
    ys, xs = np.nonzero(cls >= 0)
    return ys, xs, cls[ys, xs]


CLASS_NAMES = ("border", "tile end", "interior")


# ------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------
def n_fp16_passes(label):
    return 1 if "q" in label else int(label[0])


def ksplit_of(L):
    bm, bn = L.tile
    if (bm, bn) == (128, 128):
        return 1
    if (bm, bn) == (64, 64):
        return 2 if (L.impl == "ring" and L.rowb == 128 and "q" in L.passes) else 4
    assert (bm, bn) in ((64, 128), (128, 64), (128, 32)), f"no k-split on record for tile {L.tile}"
    return 2


def c_acc_conv(L, fp32):
    """fp32 roundings on the longest accumulation chain of a conv_ring / conv_igemm launch (module docstring)."""
    elem = 4 if fp32 else 2
    k_eff = 1 if (L.cin_p == 32 and L.k == 3 and L.impl == "reg") else L.k   # the input layer through the im2col pack is a 1x1 layer on 32 channels (a 3x3 layer on a 32-channel fp32 tensor runs on the ring kernel)
    ks = ksplit_of(L)
    ncp = L.cin_p * elem // L.rowb
    gpw = (L.rowb // 32) // ks
    assert ncp >= 1 and gpw >= 1 and L.cin_p * elem % L.rowb == 0
    per_tap = ncp * gpw * n_fp16_passes(L.passes) * (4 if fp32 else 1)
    inside = 2 if fp32 else 15
    if "q" in L.passes:
        per_tap += ncp * gpw // 2
        inside += 1
    return k_eff * k_eff * per_tap + inside + (ks - 1) + 1


def c_acc_first():
    return 2 + 15


def c_acc_pw2(label, chunks):
    return chunks * 8 * int(label[0]) + 15 + 1


def e_op_of(label, fp32, in_part=""):
    """e_op relative to |a||w| (module docstring); the absolute terms are added where the patches are at hand (_check_conv, _q_abs).
    in_part: the blocks of the INPUT tensor (a 2q launch on a lo + q tensor: the export returns the lo block, the kernel reads the q block)"""
    if fp32 or label == "1":
        return 0.0
    if "q" in label:
        if "lo" in in_part:
            return (3 * 2.0 ** -15 + 2.0 ** -19 + 2.0 ** -22 + 2.0 ** -15 + 2.0 ** -22 + 2.0 ** -24) * (1 + 2.0 ** -10)
        return (3 * 2.0 ** -15 + 2.0 ** -19 + 2.0 ** -22) * (1 + 2.0 ** -10)
    e = 0.0
    if "w" in label:
        e += 2.0 ** -22
    if "a" in label[1:]:
        e += 2.0 ** -24
    if "w" in label and "a" in label[1:]:
        e += 2.0 ** -22
    return e


def out_rounding(part, fp32, r):
    """(u_out * |r| + a_min) elementwise for a destination tensor carrying `part`"""
    a = np.abs(r)
    if fp32 or part == "f32":
        return U32 * a + 2.0 ** -149
    if "lo" in part:   # lo, or lo + q: the export returns hi + lo
        return (2.0 ** -22 + 2.0 ** -24) * a + 2.0 ** -24
    if part == "q":
        return np.where(a < 224.0, (2.0 ** -15 + 2.0 ** -23) * a + 2.0 ** -22, 2.0 ** -11 * a + 2.0 ** -24)
    return 2.0 ** -11 * a + 2.0 ** -24


def f16(x):
    return _round16(x).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------
# the sparse float64 reference
# ------------------------------------------------------------------------------------------------------------
def _patches(a_nhwc_padded, n, ys, xs, k):
    """[P][k*k*C] float64 input patches of output pixels (ys, xs) of image n; the tensor is zero-padded by k//2 already"""
    d = np.arange(k)
    p = a_nhwc_padded[n, ys[:, None, None] + d[None, :, None], xs[:, None, None] + d[None, None, :], :]
    return p.reshape(len(ys), -1)


def _wmat(w):
    """[k*k*cin][cout] float64, in the patch order (dy, dx, c)"""
    cout = w.shape[0]
    return np.ascontiguousarray(np.asarray(w, np.float64).transpose(2, 3, 1, 0).reshape(-1, cout))


class Failure:
    def __init__(self, launch, layer, dest, img, y, x, ch, cls, got, ref, ratio):
        self.launch, self.layer, self.dest, self.img, self.y, self.x, self.ch, self.cls, self.got, self.ref, self.ratio = launch, layer, dest, img, y, x, ch, cls, got, ref, ratio

    def __str__(self):
        return (f"{self.layer} [{key_str(self.launch.key)}] -> {self.dest} image {self.img} pixel (y {self.y}, x {self.x}) channel {self.ch} "
                f"class {self.cls}: got {self.got:.9g} ref {self.ref:.9g} |err|/tol {self.ratio:.3g}")


class Report:
    """result of one launch: worst |err|/tol, the failures (worst first per layer / destination), what was sampled"""
    def __init__(self, launch):
        self.launch, self.worst, self.failures, self.nfail, self.nchecked, self.npixels, self.tiles = launch, 0.0, [], 0, 0, 0, 0
        self.by_class = {}   # (destination, pixel class) -> [elements, failures, worst ratio]: a bug sits at seams, borders or one channel, a gap in the derivation everywhere

    def add(self, layer, dest, imgs, ys, xs, cls, got, ref, tol, ch0=0):
        err = np.abs(got - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = err / tol
        ratio[~np.isfinite(got)] = np.inf
        self.nchecked += ratio.size
        if ratio.size:
            self.worst = max(self.worst, float(ratio.max()))
        bad = ~(ratio <= 1.0)
        nb = int(bad.sum())
        self.nfail += nb
        for c in np.unique(cls):
            sel = cls == c
            ent = self.by_class.setdefault((dest, CLASS_NAMES[c] if c >= 0 else "all"), [0, 0, 0.0])
            ent[0] += int(sel.sum()) * ratio.shape[1]
            ent[1] += int(bad[sel].sum())
            ent[2] = max(ent[2], float(ratio[sel].max()))
        if nb:
            pi, ci = np.nonzero(bad)
            order = np.argsort(-ratio[pi, ci])[:8]
            for o in order:
                p, c = pi[o], ci[o]
                self.failures.append(Failure(self.launch, layer, dest, int(imgs[p]), int(ys[p]), int(xs[p]), ch0 + int(c), CLASS_NAMES[cls[p]] if cls[p] >= 0 else "all",
                                             float(got[p, c]), float(ref[p, c]), float(ratio[p, c])))


def _nhwc_padded(a, pad):
    a = np.asarray(a, np.float64).transpose(0, 2, 3, 1)
    return np.pad(a, ((0, 0), (pad, pad), (pad, pad), (0, 0)))


def check_plan(summary, graph, weights, blob, fp32=False, n_interior=256, seed=0, only=None, max_samples=None, images_per_launch=None, saturating=False):
    """Check every launch of a plan (or those whose layers intersect `only`).  saturating: bound `2q` launches beyond the e4m3 ranges instead of asserting
    |a| < 112 (module docstring); True / False, or a function of the Launch.

    weights: name -> (w [cout][cin][k][k] float32, b); blob(name) -> [N][C][H][W] float32 as rtp_get_blob returns it (the input blob under the
    graph's input name, the final maps under graph.lowres).  Returns [Report]."""
    levels, launches = parse_plan(summary)
    parts = tensor_parts(graph, launches)
    rs = np.random.RandomState(seed)
    reports = []
    for L in launches:
        if only is not None and not (set(L.layers) | set(L.layers2) | {getattr(L, "pool_out", None)}) & set(only):
            continue
        rep = Report(L)
        reports.append(rep)
        if L.kind == "pool":
            _check_pool_step(L, rep, blob)
            continue
        lvl = graph.level[graph.convs[L.layers[0]]["bottom"]]
        H, W, halo = levels[lvl]
        if L.kind == "pw2":
            L.dsts = _pw2_dsts(graph, L)
        # ---- the sample set (pooled coordinates for +pool)
        if L.pool:
            ends, ntiles = pool_tile_ends(H, W, L.k, L.tile[0])
            sh, sw = H // 2, W // 2
        elif L.kind == "first":
            ends, ntiles = [(y, x) for y in range(H) for x in (0, W - 1)], H     # a workgroup per image row
            sh, sw = H, W
        else:
            ends, ntiles = plain_tile_ends(H, W, halo, L.tile[0])
            sh, sw = H, W
        ni = n_interior
        if max_samples is not None:   # shrink the interior sample only
            fixed = len(sample_pixels(sh, sw, ends, 0, np.random.RandomState(0))[0])
            ni = max(0, min(ni, max_samples - fixed))
        ys, xs, cls = sample_pixels(sh, sw, ends, ni, rs)
        rep.tiles = ntiles
        assert {(y, x) for y, x in ends} <= set(zip(ys.tolist(), xs.tolist())), "a workgroup without a sampled pixel"
        for bi, name in enumerate(L.layers):
            g = graph.convs[name]
            a = blob(g["bottom"])
            N = a.shape[0]
            assert a.shape[1:] == (graph.channels[g["bottom"]], H, W), (name, a.shape)
            if bi == 0:
                nprob, nt = len(L.layers), (L.coutp // L.tile[1] if L.kind != "first" else 1)
                ni_plan = images_per_launch or L.wgs // (ntiles * nprob * nt)
                assert L.wgs == ntiles * nprob * nt * ni_plan, f"{L}: the tile walk here gives {ntiles} tiles per image, the plan {L.wgs} workgroups"
            rep.npixels += N * len(ys)
            if L.kind == "pw2":
                _check_pw2(L, rep, graph, weights, blob, parts, name, L.layers2[bi], a, ys, xs, cls)
            else:
                _check_conv(L, rep, graph, weights, blob, parts, fp32, name, a, ys, xs, cls, saturating=saturating(L) if callable(saturating) else saturating)
    return reports


def _operands(label, fp32, a, w, first=False):
    """the reference's operands for a pass label (module docstring, e_op)"""
    if fp32:
        return np.asarray(a, np.float64), np.asarray(w, np.float64)
    a64 = np.asarray(a, np.float64) if ("a" in label[1:] or "q" in label) else f16(a)
    w64 = np.asarray(w, np.float64) if ("w" in label or "q" in label) else f16(w)
    return a64, w64


def _q_abs(label, w_launch, sum_a, sum_w, in_part=""):
    """absolute terms of the 2q bound (e4m3 subnormals in the scaled domain), t as the engine derives it from the launch's weights"""
    if "q" not in label:
        return 0.0
    t = _wq_t(w_launch)
    e = (2 + 2.0 ** -4) * 2.0 ** (-21 - t) * sum_a + 2.0 ** -23 * sum_w
    return e + (2.0 ** -22 + 2.0 ** -25) * sum_w if "lo" in in_part else e


def _abs_hi(a64):
    """|a_hi| of an exported a = a_hi + l8 (or + lo): |f16(a)|, or the larger of f16(a) and its mirror image where a is exactly midway between two fp16 values"""
    h = f16(a64)
    m = 2.0 * a64 - h
    tie = (m != h) & (f16(m) == m)
    return np.where(tie, np.maximum(np.abs(h), np.abs(m)), np.abs(h))


def _wq_t(w_launch):
    """the fp8 weight exponent of a 2q launch, as engine.cpp compute_wq_exp derives it from the launch's weights"""
    mx = max(float(np.abs(w).max()) for w in w_launch)
    t = int(np.floor(np.log2(448.0 / mx))) if mx > 0 else 0
    return max(-20, min(t, 40))


class _Saturation:
    """the per-element terms of a 2q launch beyond the e4m3 ranges (module docstring): padded NHWC operands and weight matrices, applied patch by patch"""
    SUBNORMAL_W = True      # (a test switches the fp16-subnormal W_hi term off to show that the other three are exactly 0 inside the ranges)

    def __init__(self, a64, w64, w_launch, in_part, pad):
        ah = _abs_hi(a64)
        self.k = w64.shape[2]
        self.sat_a = _nhwc_padded(np.maximum(ah - 112.0, 0.0), pad)
        self.qa = _nhwc_padded(np.minimum((1 + 2.0 ** -4) * ah, 112.0), pad)
        self.abs_a = _nhwc_padded(np.abs(a64), pad)
        wlo = np.abs(_wmat(w64) - _wmat(f16(w64)))
        self.wlo, self.wabs = wlo, np.abs(_wmat(w64))
        self.sub_w = np.maximum(wlo - 2.0 ** -11 * self.wabs, 0.0)
        self.sat_w = np.maximum(wlo - 448.0 * 2.0 ** -(_wq_t(w_launch) + 11), 0.0)
        self.sat_l = None
        if "lo" in in_part:
            x = np.abs(a64 - f16(a64))
            dp = (x + 2.0 ** -24 * np.abs(a64) + 2.0 ** -25) * (1 + 2.0 ** -10)
            self.sat_l = _nhwc_padded(np.maximum(dp - 448.0 / 4096.0, 0.0), pad)
        self.c_sub = (2.0 ** -4 + (1 + 2.0 ** -4) * 2.0 ** -4 + 2.0 ** -11) * (1 + 2.0 ** -10)

    def tol(self, n, ys, xs):
        t = _patches(self.sat_a, n, ys, xs, self.k) @ self.wlo
        if self.SUBNORMAL_W and self.sub_w.any():
            t = t + self.c_sub * (_patches(self.abs_a, n, ys, xs, self.k) @ self.sub_w)
        if self.sat_w.any():
            t = t + _patches(self.qa, n, ys, xs, self.k) @ self.sat_w
        if self.sat_l is not None:
            t = t + _patches(self.sat_l, n, ys, xs, self.k) @ self.wabs
        return t


def _check_conv(L, rep, graph, weights, blob, parts, fp32, name, a, ys, xs, cls, saturating=False):
    g = graph.convs[name]
    w, b = weights[name]
    k, pad = g["k"], g["k"] // 2
    label = L.passes
    a64, w64 = _operands(label, fp32, a, w)
    if "q" in label and not saturating:
        assert np.abs(a64).max() < 112.0, f"{name}: |activation| >= 112 saturates e4m3(a_hi * 4): the 2q bound does not cover it"
    ap = _nhwc_padded(a64, pad)
    wm = _wmat(w64)
    wabs = np.abs(wm)
    sum_w = wabs.sum(axis=0)[None, :]
    b64 = np.asarray(b, np.float64)[None, :]
    c_acc = c_acc_first() if L.kind == "first" else c_acc_conv(L, fp32)
    in_part = parts.get(g["bottom"], "")
    e_rel = c_acc * U32 + e_op_of(label, fp32, in_part)
    e_abs_a = 2.0 ** -25 if ("w" in label and not fp32) else 0.0            # subnormal W_lo: half an fp16 subnormal step per term
    flush = 2.0 ** -126 * wm.shape[0] if fp32 else 0.0
    w_launch = [weights[n][0] for n in L.layers]
    sat = _Saturation(a64, w64, w_launch, parts.get(g["bottom"], ""), pad) if ("q" in label and saturating) else None
    dests = graph.dests(name)
    N = a.shape[0]
    if L.pool:   # the un-pooled blob is never written: the destination is the pooled blob
        dests = [([t for t, bsrc in graph.pools.items() if bsrc == name][0], 0)]
    got_blobs = {d: blob(d) for d, _ in dests}
    cout = g["cout"]
    for n in range(N):
        for s in range(0, len(ys), CHUNK):
            yy, xx, cc = ys[s:s + CHUNK], xs[s:s + CHUNK], cls[s:s + CHUNK]
            if L.pool:
                pre, acc_tol = None, None
                for dy in (0, 1):
                    for dx in (0, 1):
                        p = _patches(ap, n, 2 * yy + dy, 2 * xx + dx, k)
                        v = p @ wm + b64
                        pa = np.abs(p)
                        S = pa @ wabs + np.abs(b64)
                        t = e_rel * S + e_abs_a * pa.sum(axis=1, keepdims=True) + _q_abs(label, w_launch, pa.sum(axis=1, keepdims=True), sum_w, in_part) + flush
                        if sat is not None:
                            t = t + sat.tol(n, 2 * yy + dy, 2 * xx + dx)
                        pre = v if pre is None else np.maximum(pre, v)
                        acc_tol = t if acc_tol is None else np.maximum(acc_tol, t)
            else:
                p = _patches(ap, n, yy, xx, k)
                pre = p @ wm + b64
                pa = np.abs(p)
                S = pa @ wabs + np.abs(b64)
                acc_tol = e_rel * S + e_abs_a * pa.sum(axis=1, keepdims=True) + _q_abs(label, w_launch, pa.sum(axis=1, keepdims=True), sum_w, in_part) + flush
                if sat is not None:
                    acc_tol = acc_tol + sat.tol(n, yy, xx)
            r = np.maximum(pre, 0.0) if g["relu"] else pre
            imgs = np.full(len(yy), n)
            for d, off in dests:
                part = "f32" if d == graph.lowres else parts.get(d, "")
                got = np.asarray(got_blobs[d][n, off:off + cout][:, yy, xx], np.float64).T
                rep.add(name, d, imgs, yy, xx, cc, got, r, out_rounding(part, fp32, r) + acc_tol)


def _check_pw2(L, rep, graph, weights, blob, parts, name1, name2, a, ys, xs, cls):
    g1, g2 = graph.convs[name1], graph.convs[name2]
    (w1, b1), (w2, b2) = weights[name1], weights[name2]
    lab1, lab2 = L.passes.split("/")
    a64, w1_64 = _operands(lab1, False, a, w1)
    _, w2_64 = _operands(lab2, False, a[:, :1, :1, :1], w2)
    ap = _nhwc_padded(a64, 0)
    wm1, wm2 = _wmat(w1_64), _wmat(w2_64)
    chunks = L.mid // 128
    e1 = c_acc_pw2(lab1, 1) * U32 + e_op_of(lab1, False)
    e2 = c_acc_pw2(lab2, chunks) * U32 + e_op_of(lab2, False)
    abs1 = 2.0 ** -25 if "w" in lab1 else 0.0
    abs2 = 2.0 ** -25 if "w" in lab2 else 0.0
    h_lo = "a" in lab2[1:]                                  # the second GEMM reads a lo part of the middle blob (conv_pw2.hip h_lo)
    dests = graph.dests(name2)
    got_blobs = {d: blob(d) for d, _ in dests}
    for n in range(a.shape[0]):
        for s in range(0, len(ys), CHUNK):
            yy, xx, cc = ys[s:s + CHUNK], xs[s:s + CHUNK], cls[s:s + CHUNK]
            p = _patches(ap, n, yy, xx, 1)
            pa = np.abs(p)
            pre1 = p @ wm1 + np.asarray(b1, np.float64)[None]
            S1 = pa @ np.abs(wm1) + np.abs(np.asarray(b1, np.float64))[None]
            h = np.maximum(pre1, 0.0) if g1["relu"] else pre1
            t1 = e1 * S1 + abs1 * pa.sum(axis=1, keepdims=True) + out_rounding("lo" if h_lo else "", False, h)
            r = h @ wm2 + np.asarray(b2, np.float64)[None]
            hb = np.abs(h) + t1
            carried = t1 @ np.abs(wm2)                      # the first stage's bound through sum |w2|
            S2 = hb @ np.abs(wm2) + np.abs(np.asarray(b2, np.float64))[None]
            acc_tol = e2 * S2 + abs2 * hb.sum(axis=1, keepdims=True) + carried
            if g2["relu"]:
                r = np.maximum(r, 0.0)
            imgs = np.full(len(yy), n)
            for d, off in dests:
                part = "f32" if d == graph.lowres else parts.get(d, "")
                got = np.asarray(got_blobs[d][n, off:off + g2["cout"]][:, yy, xx], np.float64).T
                rep.add(name2, d, imgs, yy, xx, cc, got, r, out_rounding(part, False, r) + acc_tol)


def _check_pool_step(L, rep, blob):
    """a stand-alone pooling launch moves values: every element of the pooled blob EQUALS the maximum of its four inputs"""
    a, got = blob(L.pool_in), blob(L.pool_out)
    N, C, H, W = a.shape
    ref = a.reshape(N, C, H // 2, 2, W // 2, 2).max(axis=(3, 5))
    assert got.shape == ref.shape
    bad = ~(got == ref)
    rep.nchecked, rep.npixels = ref.size, N * (H // 2) * (W // 2)
    rep.nfail = int(bad.sum())
    rep.worst = 0.0 if not rep.nfail else float("inf")
    for n, c, y, x in list(zip(*np.nonzero(bad)))[:8]:
        b = min(BORDER, H // 2, W // 2)
        border = y < b or x < b or y >= H // 2 - b or x >= W // 2 - b
        rep.failures.append(Failure(L, f"{L.pool_in} -> {L.pool_out}", L.pool_out, int(n), int(y), int(x), int(c), "border" if border else "interior",
                                    float(got[n, c, y, x]), float(ref[n, c, y, x]), float("inf")))


def summarize(reports):
    """instantiation key -> worst |err|/tol over the launches that run it"""
    out = {}
    for r in reports:
        out[r.launch.key] = max(out.get(r.launch.key, 0.0), r.worst)
    return out


# ------------------------------------------------------------------------------------------------------------
# a correct kernel, emulated on the CPU: operands rounded to fp16, float32 accumulation, output rounded to fp16 (+ lo part)
# ------------------------------------------------------------------------------------------------------------
def _round16(v32):
    """float32 -> nearest fp16 -> float32 (torch's conversion where it is installed: numpy's is scalar code, 40 ms per 7x7 layer)"""
    v32 = np.ascontiguousarray(v32, np.float32)
    try:
        import torch
        return torch.from_numpy(v32).half().float().numpy()
    except ImportError:
        return v32.astype(np.float16).astype(np.float32)


def _e4m3(x32):
    """float32 -> nearest OCP e4m3 (saturating at 448, like the clamp in front of v_cvt_pk_fp8_f32) -> float32"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.clip(x32, -448.0, 448.0), np.float32)).to(torch.float8_e4m3fn).float().numpy()


def _split16(v32):
    hi = _round16(v32)
    return hi, _round16(np.asarray(v32, np.float32) - hi)


class Emulation:
    """Runs the launches of an fp16 / F16X3 / mixed plan (pass labels 1, 2w, 2a, 3aw, 2q) the way the kernels do, launch by launch, each on the previous
    launches' stored outputs.  pre[layer] keeps the fp32 value of every convolution before ReLU / pooling / rounding so that a test can plant a
    defect there and store the result again (restore).  The conversions (e4m3, r16), the exponents the fp8 weights are packed and descaled with (wq_pack,
    WLO_EXP) and the ordering of the stand-alone q pooling (pool_value) are methods, so that a subclass can plant a defect in any of them
    (tests/test_conv_ranges_cpu.py).  hi / lo / q8 hold a blob's fp16 value, its fp16 rounding error and that error as the
    stored e4m3(lo * 2^12) / 2^12 — each kept where a tensor the blob is stored to carries that block."""

    def __init__(self, summary, graph, weights, frame, stop_after=None):
        self.graph, self.weights = graph, weights
        self.levels, self.launches = parse_plan(summary)
        self.parts = tensor_parts(graph, self.launches)
        self.wq_exp = {}    # fp8-compensated launches: the weight scale t, shared by the branches of a launch (engine.cpp compute_wq_exp)
        self.hi, self.lo, self.q8, self.pre, self.lowres_part = {graph.input: np.asarray(frame, np.float32)}, {}, {}, {}, {}
        for L in self.launches:
            self.run(L)
            if stop_after in L.layers + L.layers2:   # (the network has 52 M weights: a test that needs the first stages only stops there)
                break

    WLO_EXP = 11        # W_lo8 = e4m3(W_lo * 2^(t + 11)), descaled by the E8M0 scale 127 - t - WLO_EXP (conv_ring.hip sb_odd)

    def e4m3(self, x32):
        return _e4m3(x32)

    def r16(self, v32):
        return _round16(v32)

    def split16(self, v32):
        hi = self.r16(v32)
        return hi, self.r16(np.asarray(v32, np.float32) - hi)

    def mfma_in(self, x16):
        """an fp16 operand as the MFMA reads it: subnormals included"""
        return x16

    def wq_pack(self, name):
        """the exponent layer `name`'s fp8 weights are packed with: the launch's (the kernel descales with wq_exp[name])"""
        return self.wq_exp[name]

    def pool_value(self, hi, part):
        """what the stand-alone pooling step orders by: the whole value (maxpool_q_kernel: hi, ties broken by the q byte)"""
        return hi + part

    def blob(self, name):
        """what rtp_get_blob returns: hi + lo in fp32, concat blobs assembled from their inputs, the final maps in fp32"""
        if name == self.graph.lowres:
            return np.concatenate([self.lowres_part[b] for b in self.graph.concats[name]], axis=1) if name in self.graph.concats else self.lowres_part[name]
        if name not in self.graph.concats and name not in self.hi:
            raise KeyError(f"blob {name} is not materialised")
        part = self.parts.get(name, "")          # the export adds the lo block where there is one, else the q block (kernels.h launch_export)
        hi, lo = self.operand(name)
        return hi + lo if "lo" in part else hi + self.operand_q(name) if part else hi

    @staticmethod
    def conv32(a, w, pad):
        """stride-1 'same' cross-correlation in float32: im2col + one float32 matmul (fp32 products, fp32 accumulation)"""
        a = np.asarray(a, np.float32)
        N, C, H, W = a.shape
        k = w.shape[2]
        ap = np.pad(a, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
        win = np.lib.stride_tricks.sliding_window_view(ap, (k, k), axis=(2, 3))          # [N][C][H][W][k][k]
        cols = np.ascontiguousarray(win.transpose(0, 2, 3, 1, 4, 5)).reshape(N * H * W, C * k * k)
        out = cols @ np.ascontiguousarray(np.asarray(w, np.float32).reshape(w.shape[0], -1).T)
        return np.ascontiguousarray(out.reshape(N, H, W, -1).transpose(0, 3, 1, 2))

    def gemm(self, name, label, a_hi, a_lo, skip=()):
        """fp32 value of one convolution: the passes a_hi*W_hi [+ a_lo*W_hi] [+ a_hi*W_lo] + bias.  skip: passes left out (planted defects)"""
        w, b = self.weights[name]
        w_hi, w_lo = self.split16(np.asarray(w, np.float32))
        pad = w.shape[2] // 2
        v = self.conv32(self.mfma_in(a_hi), self.mfma_in(w_hi), pad)
        if "q" in label:   # a_lo is the stored e4m3(lo * 2^12) / 2^12 here; the fp8 products are exact, the scales powers of two
            t, tp = self.wq_exp[name], self.wq_pack(name)
            v = v + self.conv32(a_lo, self.e4m3(w_hi * np.float32(2.0 ** tp)) * np.float32(2.0 ** -t), pad)
            v = v + self.conv32(self.e4m3(a_hi * np.float32(4)) * np.float32(0.25), self.e4m3((np.asarray(w, np.float32) - w_hi) * np.float32(2.0 ** (tp + 11))) * np.float32(2.0 ** -(t + self.WLO_EXP)), pad)
            return v + np.asarray(b, np.float32)[None, :, None, None]
        if "a" in label[1:] and "a" not in skip:
            v = v + self.conv32(self.mfma_in(a_lo), self.mfma_in(w_hi), pad)
        if "w" in label and "w" not in skip:
            v = v + self.conv32(self.mfma_in(a_hi), self.mfma_in(w_lo), pad)
        return v + np.asarray(b, np.float32)[None, :, None, None]

    def operand(self, name):
        if name in self.graph.concats:   # a concat tensor: its slices were stored by their producers, each with the parts the concat's consumers need
            bots = self.graph.concats[name]
            have = next(self.hi[b] for b in bots if b in self.hi)
            zeros = lambda b: np.zeros((have.shape[0], self.graph.channels[b]) + have.shape[2:], np.float32)   # a slice nobody has written yet
            hi = np.concatenate([self.hi[b] if b in self.hi else zeros(b) for b in bots], axis=1)
            lo = np.concatenate([self.lo[b] if b in self.lo else zeros(b) for b in bots], axis=1)
            return hi, lo
        return self.hi[name], self.lo.get(name, np.zeros_like(self.hi[name]))

    def operand_q(self, name):
        """the q block of a tensor, as values: e4m3(lo * 2^12) / 2^12 per channel"""
        if name in self.graph.concats:
            bots = self.graph.concats[name]
            have = next(self.hi[b] for b in bots if b in self.hi)
            zeros = lambda b: np.zeros((have.shape[0], self.graph.channels[b]) + have.shape[2:], np.float32)
            return np.concatenate([self.q8[b] if b in self.q8 else zeros(b) for b in bots], axis=1)
        return self.q8.get(name, np.zeros_like(self.hi[name]))

    def store(self, name, v, dest=None):
        """ReLU, rounding to fp16 (+ the lo and q blocks that the tensors it is stored to carry), under the blob name `dest`"""
        g = self.graph.convs[name]
        if g["relu"]:
            v = np.maximum(v, np.float32(0))
        hi, lo = self.split16(v.astype(np.float32))
        dest = dest or name
        self.hi[dest] = hi
        wants = "+".join([self.parts.get(dest, "")] + [self.parts.get(c, "") for c, bots in self.graph.concats.items() if dest in bots])
        if "lo" in wants:
            self.lo[dest] = lo
        else:
            self.lo.pop(dest, None)
        if "q" in wants:
            self.q8[dest] = self.e4m3((v.astype(np.float32) - hi) * np.float32(4096)) * np.float32(1.0 / 4096)
        else:
            self.q8.pop(dest, None)
        if dest == self.graph.lowres or dest in self.graph.concats.get(self.graph.lowres, ()):
            self.lowres_part[dest] = v.astype(np.float32)

    def finish(self, L, name, v, pool3=False):
        """epilogue of convolution `name` of launch L on the fp32 values v (pooled in the epilogue where the plan says so)"""
        if L.pool:
            N, C, H, W = v.shape
            q = v.reshape(N, C, H // 2, 2, W // 2, 2)
            v = np.maximum(np.maximum(q[:, :, :, 0, :, 0], q[:, :, :, 0, :, 1]), q[:, :, :, 1, :, 0]) if pool3 else q.max(axis=(3, 5))
            self.store(name, v, dest=[t for t, b in self.graph.pools.items() if b == name][0])
        else:
            self.store(name, v)

    def run(self, L):
        if L.kind == "pool":
            hi, lo = self.operand(L.pool_in)
            q8 = self.operand_q(L.pool_in)
            in_part, out_part = self.parts.get(L.pool_in, ""), self.parts.get(L.pool_out, "")
            N, C, H, W = hi.shape
            val = self.pool_value(hi, lo if "lo" in in_part else q8).reshape(N, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
            sel = val.argmax(axis=-1)[..., None]
            take = lambda t: np.take_along_axis(t.reshape(N, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4), sel, -1)[..., 0]
            self.hi[L.pool_out] = take(hi)
            if "lo" in out_part:
                self.lo[L.pool_out] = take(lo)
            if "q" in out_part:
                self.q8[L.pool_out] = take(q8)
            return
        lab1 = L.passes.split("/")[0]
        if "q" in lab1:
            for n in L.layers:
                self.wq_exp[n] = _wq_t([self.weights[m][0] for m in L.layers])
        for bi, name in enumerate(L.layers):
            a_hi, a_lo = self.operand(self.graph.convs[name]["bottom"])
            if "q" in lab1:
                a_lo = self.operand_q(self.graph.convs[name]["bottom"])
            v = self.gemm(name, lab1, a_hi, a_lo)
            self.pre[name] = v
            if L.kind != "pw2":
                self.finish(L, name, v)
                continue
            lab2 = L.passes.split("/")[1]
            if self.graph.convs[name]["relu"]:
                v = np.maximum(v, np.float32(0))
            h_hi, h_lo = self.split16(v)
            name2 = L.layers2[bi]
            v2 = self.gemm(name2, lab2, h_hi, h_lo)
            self.pre[name2] = v2
            self.store(name2, v2)


# ------------------------------------------------------------------------------------------------------------
# the configurations of tests/test_conv_launches.py (enumerated on the CPU: every instantiation the benchmarked plans run, plus geometry edges)
# ------------------------------------------------------------------------------------------------------------
MATRIX = OrderedDict([   # name -> (mode, model, W, H, num_scales, scale_gap, batch_frames, synthetic_seed)
    ("mixed_coco_656x368_b2_wseed5", ("mixed", 0, 656, 368, 1, 0.3, 2, 5)),    # bench.py's default plan, on weights other than the default set
    ("mixed_coco_656x368_b1", ("mixed", 0, 656, 368, 1, 0.3, 1, 1)),           # 128x32 and 64x64 pair tiles
    ("mixed_coco_656x368_3s", ("mixed", 0, 656, 368, 3, 0.15, 1, 1)),          # 128x64 and 128x128 pairs, three images per launch: image seams
    ("mixed_mpi_496x368", ("mixed", 1, 496, 368, 1, 0.3, 1, 1)),               # cout 28 tails, a stand-alone pooling step
    ("mixed_coco_656x368_3s_b2", ("mixed", 0, 656, 368, 3, 0.15, 2, 1)),       # six images per launch: 128x64 tiles with 128-byte chunks for the stage-entry pairs,
    ("mixed_mpi_496x368_b2", ("mixed", 1, 496, 368, 1, 0.3, 2, 1)),            # conv4_4_CPM on 128x128 — plans bench.py times that the eight above do not reach
    ("mixed_coco_320x176", ("mixed", 0, 320, 176, 1, 0.3, 1, 1)),
    ("mixed_coco_176x320", ("mixed", 0, 176, 320, 1, 0.3, 1, 1)),              # portrait: 22-pixel rows at 1/8, several row wraps per tile
    ("mixed_coco_144x80", ("mixed", 0, 144, 80, 1, 0.3, 1, 1)),
    ("mixed_coco_64x48", ("mixed", 0, 64, 48, 1, 0.3, 1, 1)),                  # a whole 1/8 image is smaller than one tile
    ("f16x3_coco_656x368", ("f16x3", 0, 656, 368, 1, 0.3, 1, 1)),              # 3aw, 2w on the reg kernel
    ("fp16_coco_656x368", ("fp16", 0, 656, 368, 1, 0.3, 1, 1)),                # plain passes on production tiles
    ("fp32_coco_160x96_2s", ("fp32", 0, 160, 96, 2, 0.3, 1, 1)),
])


def matrix_config(name, matrix=None):
    """the engine configuration of a MATRIX entry (or of an entry of a sibling matrix with the same columns: tests/_manycases.py)"""
    import caffe_rtpose_amd as r
    mode, model, W, H, N, gap, B, wseed = (MATRIX if matrix is None else matrix)[name]
    prec = {"fp16": r.PREC_FP16, "fp32": r.PREC_FP32, "mixed": r.PREC_MIXED, "f16x3": r.PREC_F16X3}[mode]
    return r.Config(model=model, net_w=W, net_h=H, num_scales=N, scale_gap=gap, precision=prec, frames_in_flight=B, batch_frames=B, synthetic_seed=wseed)


# ------------------------------------------------------------------------------------------------------------
# the configurations of tests/test_batch_launches.py: FULL batches of different frames through rtp_submit / rtp_collect, read back with
# rtp_get_batch_blob.  What is under test is decided by the image count and the grid (the XCD remap of the block index and its q / r split
# where the grid is no multiple of 8, img = tile / tiles_per_img for the images of the frames behind the first, the seam between two frames'
# images in the arena, the partial-batch graphs), not by the image size: the shapes are the smallest that reach the tile classes of the
# benched batch plans (tests/test_batch_launches_cpu.py asserts which).  The last entry is there for ONE class, `conv ring 128x128 rowb 128
# passes 1` without a pooling epilogue (conv4_3_CPM / conv4_4_CPM of the benched batch plans): the planner gives a 3x3 layer at 1/8 resolution
# 128x128 tiles only where the launch still has enough workgroups, and the first nine cases are too small for that.  Searched with
# rtp_plan_summary over every multiple-of-16 shape up to 656x368, 1-3 scales, batch_frames 2-6: with batch_frames 2 the fewest pixels per launch
# that reach it are 192x304 at three scales (350208; 512x368 at one scale: 376832).  Only more frames per batch go lower (32x304, three scales,
# batch_frames 6: 175104 pixels, 1/8 maps four pixels wide, 17 frames to tap).  It runs the bitwise test like every case; that test needs no
# float64 reference.
# ------------------------------------------------------------------------------------------------------------
BATCH_MATRIX = OrderedDict([   # name -> (mode, model, W, H, num_scales, scale_gap, batch_frames, synthetic_seed)
    ("mixed_coco_64x48_b2", ("mixed", 0, 64, 48, 1, 0.3, 2, 1)),               # a 1/8 image smaller than one tile
    ("mixed_coco_144x80_b3", ("mixed", 0, 144, 80, 1, 0.3, 3, 1)),             # odd image count
    ("mixed_coco_176x320_2s_b2", ("mixed", 0, 176, 320, 2, 0.3, 2, 1)),        # portrait, 4 images, 128x128 tiles
    ("mixed_coco_160x96_3s_b2", ("mixed", 0, 160, 96, 3, 0.15, 2, 1)),         # 6 images, like coco_3s_b2
    ("mixed_coco_320x176_b2", ("mixed", 0, 320, 176, 1, 0.3, 2, 1)),           # tile set of the default plan
    ("mixed_mpi_96x64_b5", ("mixed", 1, 96, 64, 1, 0.3, 5, 1)),                # 5 images like bench.py --model mpi; cout 28 tails; stand-alone pool; pw2 grid no multiple of 8
    ("f16x3_coco_144x80_b2", ("f16x3", 0, 144, 80, 1, 0.3, 2, 1)),             # 3aw / 2w, register-staged kernel with a grid that is no multiple of 8
    ("fp16_coco_144x80_b3", ("fp16", 0, 144, 80, 1, 0.3, 3, 1)),
    ("fp32_coco_160x96_2s_b2", ("fp32", 0, 160, 96, 2, 0.3, 2, 1)),            # 64x128 / 64x64 / 128x64 reg tiles
    ("mixed_coco_192x304_3s_b2", ("mixed", 0, 192, 304, 3, 0.15, 2, 1)),       # conv ring 128x128 rowb 128 passes 1 without a pooling epilogue
])
BATCH_FLOAT64 = ("mixed_coco_160x96_3s_b2", "mixed_mpi_96x64_b5", "fp32_coco_160x96_2s_b2")   # cases that also run every launch of the full batch against float64


def batch_config(name, exec_mode=None, contexts=2, matrix=None):
    """the engine configuration of a BATCH_MATRIX entry (or of a sibling matrix, tests/_manycases.py): `contexts` full batches in flight"""
    import caffe_rtpose_amd as r
    mode, model, W, H, N, gap, B, wseed = (BATCH_MATRIX if matrix is None else matrix)[name]
    prec = {"fp16": r.PREC_FP16, "fp32": r.PREC_FP32, "mixed": r.PREC_MIXED, "f16x3": r.PREC_F16X3}[mode]
    kw = {} if exec_mode is None else dict(exec_mode=exec_mode)
    return r.Config(model=model, net_w=W, net_h=H, num_scales=N, scale_gap=gap, precision=prec, frames_in_flight=contexts * B, batch_frames=B, synthetic_seed=wseed, **kw)

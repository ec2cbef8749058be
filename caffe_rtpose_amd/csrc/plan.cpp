// plan.cpp — build_plan: (graph, resolution, scales, batch, precision mode, split rules, keep_blobs) -> Plan, on the host alone.
//
// The passes are the methods of Builder, run in order by build_plan below them.  Also here: what a config means for the plan
// (plan_input_from_config, load_netdef), workgroups per launch, the context count and the text of rtp_plan_summary (describe_plan).
// No HIP runtime call.
#include "plan.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

namespace rtp {

// ---- split-precision policy ------------------------------------------------------------------
// Default RTP_PREC_MIXED set, from tools/sim_precision.py (error of the final maps vs an fp32 run, per layer and per
// rounded operand): the fp16 rounding of weights and activations contributes about equally in every layer, and the
// final-map error is dominated by the trunk from conv2 on, the last two refinement stages and (cheaply fixed) all 1x1
// layers; the first refinement stages are attenuated by each later stage's re-injection of conv4_4_CPM.
// Measured (tests/test_precision.py; tools/sim_precision.py reproduces the rms to 3 digits): final maps normalised to max 1,
//   fp16 everywhere                          rms 3.5e-4   max 2.0-2.6e-3
//   conv2-4, stages 5-6, 1x1 (2.08x MFMA)    rms 1.36e-4  max 0.8-1.03e-3   <- no margin on the +-1e-3 tolerance
//   + stage 4 (this default, 2.35x MFMA)     rms 1.03e-4  max <= 0.8e-3
//   every layer (RTP_PREC_F16X3, 3x MFMA)    rms 1.6e-6   max 1e-5
const char* const kDefaultSplit = "conv2_,conv3_,conv4_,*_stage4_,*_stage5_,*_stage6_,@1x1";
void layer_split(const PlanInput& in, int prec, const ConvOp& c, bool* w, bool* a, bool* x) {
  *w = *a = false;
  if (x) *x = false;
  if (prec != 0) return;
  if (in.mode == RTP_PREC_F16X3) { *w = *a = true; return; }
  if (in.mode != RTP_PREC_MIXED) return;
  const std::string& rules = in.split_rules;
  size_t pos = 0;
  while (pos <= rules.size()) {
    size_t c2 = rules.find(',', pos);
    std::string tok = rules.substr(pos, c2 == std::string::npos ? std::string::npos : c2 - pos);
    pos = c2 == std::string::npos ? rules.size() + 1 : c2 + 1;
    if (tok.empty()) continue;
    bool tw = true, ta = true, tx = false;
    if (tok.size() > 2 && tok[tok.size() - 2] == ':') {
      const char k = tok.back();
      tok.resize(tok.size() - 2);
      if (k == 'w') ta = false;
      else if (k == 'a') tw = false;
      else if (k == 'x') tx = true;   // both operands, corrections as two more fp16 passes (what RTP_PREC_F16X3 runs everywhere)
    }
    bool hit;
    if (tok == "@all") hit = true;
    else if (tok == "@1x1") hit = c.k == 1;
    else if (tok[0] == '*') hit = c.name.find(tok.substr(1)) != std::string::npos;
    else hit = c.name.compare(0, tok.size(), tok) == 0;
    if (hit) { *w = *w || tw; *a = *a || ta; if (x) *x = *x || tx; }
  }
}

namespace {
const int GUARD_PIX = 192;  // pixels of slack before/after each tensor (strip over-read of the last tile)

int fail(std::string* err, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  *err = buf;
  return code;
}

// The plan under construction and what one pass leaves for a later one
struct Builder {
  const PlanInput& in;
  const NetDef& net;
  std::string* err;
  Plan plan;
  struct ConcatInfo { std::vector<std::string> inputs; };
  std::map<std::string, ConcatInfo> concats;   // concat blob -> its inputs
  std::vector<int> level_halo = std::vector<int>(8, 0);
  int max_level = 0;
  struct PoolTmp { std::string in, out; };
  std::vector<std::pair<int, int>> order;  // (kind 1 conv / 2 pool, index)
  std::vector<PoolTmp> pools;
  int packed_tensor = -1;  // packed im2col input
  std::map<std::string, std::vector<std::pair<std::string, int>>> concat_slices;  // concat -> (input, internal offset)

  Builder(const PlanInput& i, std::string* e) : in(i), net(*i.net), err(e) {
    plan.prec = in.mode == RTP_PREC_FP32 ? 1 : 0; plan.elem = plan.prec ? 4 : 2; plan.NI = in.N * in.B;
  }
  // the passes, in the order build_plan runs them
  int walk_graph(), lay_geometry();
  void make_tensors();
  int wire_convs();
  void make_steps();
  int choose_tile(size_t si_), tile_overrides(const ConvOp& A, const std::vector<int>& cands, bool ring_ok, int maxcout, int* best);
  void propagate_split(), fuse_pools(), direct_first_layer(), fuse_pw2(), lay_arenas();
  int postproc_sizes();
};

int Builder::walk_graph() {
  if (net.inputs.empty()) return fail(err, RTP_EINVAL, "prototxt declares no input blob");
  const std::string in_name = net.inputs[0];
  plan.blob_dims[in_name] = {3, 0};
  std::map<std::string, int> producer_conv;  // blob -> conv index
  bool have_resize = false, have_nms = false;
  for (size_t li = 0; li < net.layers.size(); ++li) {
    const LayerDef& L = net.layers[li];
    if (L.type == "Convolution") {
      if (L.bottoms.size() != 1 || L.tops.size() != 1) return fail(err, RTP_EINVAL, "layer %s: expected 1 bottom/1 top", L.name.c_str());
      auto it = plan.blob_dims.find(L.bottoms[0]);
      if (it == plan.blob_dims.end()) return fail(err, RTP_EINVAL, "layer %s: unknown bottom %s", L.name.c_str(), L.bottoms[0].c_str());
      if (L.stride != 1 || !(L.kernel == 1 || L.kernel == 3 || L.kernel == 7) || L.pad != (L.kernel - 1) / 2 || !L.bias_term)
        return fail(err, RTP_EINVAL, "layer %s: only stride-1 'same' convolutions with k in {1,3,7} and a bias are on the linevec path", L.name.c_str());
      ConvOp c;
      c.name = L.name; c.k = L.kernel; c.k_eff = L.kernel; c.cin = it->second.first; c.cout = L.num_output;
      c.level = it->second.second;
      c.first = (L.bottoms[0] == in_name);
      if (c.first && !(c.cin == 3 && c.k == 3)) return fail(err, RTP_EINVAL, "layer %s: the input convolution must be 3x3 on 3 channels", L.name.c_str());
      if (c.first) c.k_eff = 1;
      c.widx = (int)plan.convs.size();
      level_halo[c.level] = std::max(level_halo[c.level], c.k_eff / 2);
      plan.blob_dims[L.tops[0]] = {c.cout, c.level};
      producer_conv[L.tops[0]] = (int)plan.convs.size();
      order.push_back({1, (int)plan.convs.size()});
      plan.convs.push_back(c);
    } else if (L.type == "ReLU") {
      if (L.bottoms.size() != 1 || L.tops.size() != 1 || L.bottoms[0] != L.tops[0] || !producer_conv.count(L.bottoms[0]))
        return fail(err, RTP_EINVAL, "layer %s: ReLU must be in-place on a convolution output", L.name.c_str());
      if (L.negative_slope != 0.f) return fail(err, RTP_EINVAL, "layer %s: negative_slope != 0 unsupported", L.name.c_str());
      plan.convs[producer_conv[L.bottoms[0]]].relu = true;
    } else if (L.type == "Pooling") {
      auto it = plan.blob_dims.find(L.bottoms.empty() ? "" : L.bottoms[0]);
      if (it == plan.blob_dims.end()) return fail(err, RTP_EINVAL, "layer %s: unknown bottom", L.name.c_str());
      if (L.pool_method != "MAX" || L.pool_kernel != 2 || L.pool_stride != 2 || L.pool_pad != 0)
        return fail(err, RTP_EINVAL, "layer %s: only MAX 2x2 stride 2 pooling is on the linevec path", L.name.c_str());
      plan.blob_dims[L.tops[0]] = {it->second.first, it->second.second + 1};
      max_level = std::max(max_level, it->second.second + 1);
      pools.push_back({L.bottoms[0], L.tops[0]});
      order.push_back({2, (int)pools.size() - 1});
    } else if (L.type == "Concat") {
      if (L.axis != 1) return fail(err, RTP_EINVAL, "layer %s: only channel concat", L.name.c_str());
      int C = 0, lvl = -1;
      for (auto& b : L.bottoms) {
        auto it = plan.blob_dims.find(b);
        if (it == plan.blob_dims.end()) return fail(err, RTP_EINVAL, "layer %s: unknown bottom %s", L.name.c_str(), b.c_str());
        if (!producer_conv.count(b)) return fail(err, RTP_EINVAL, "layer %s: concat inputs must be convolution outputs", L.name.c_str());
        if (lvl >= 0 && lvl != it->second.second) return fail(err, RTP_EINVAL, "layer %s: concat inputs at different resolutions", L.name.c_str());
        lvl = it->second.second;
        C += it->second.first;
      }
      plan.blob_dims[L.tops[0]] = {C, lvl};
      concats[L.tops[0]] = ConcatInfo{L.bottoms};
    } else if (L.type == "ImResize") {
      if (!plan.blob_dims.count(L.bottoms[0])) return fail(err, RTP_EINVAL, "resize: unknown bottom");
      if (L.factor != 8.f) return fail(err, RTP_EINVAL, "resize: only factor 8 (the net's total stride) is supported");
      plan.lowres_blob = L.bottoms[0];
      have_resize = true;
    } else if (L.type == "Nms") {
      plan.num_parts = L.num_parts;
      plan.max_peaks = L.max_peaks;
      have_nms = true;
    } else if (L.type == "Split") {
      return fail(err, RTP_EINVAL, "layer %s: explicit Split layers are not expected in a deploy prototxt", L.name.c_str());
    } else {
      return fail(err, RTP_EINVAL, "layer %s: type %s is not on the linevec hot path", L.name.c_str(), L.type.c_str());
    }
  }
  if (!have_resize || !have_nms) return fail(err, RTP_EINVAL, "graph must end in ImResize + Nms layers");
  if (plan.num_parts == 18) plan.model = RTP_MODEL_COCO_18;
  else if (plan.num_parts == 15) plan.model = RTP_MODEL_MPI_15;
  else return fail(err, RTP_EINVAL, "Unknown number of parts (%d)! Couldn't set model", plan.num_parts);  // rtpose.cpp:227
  plan.num_limbs = plan.model == 0 ? 19 : 14;
  if (plan.max_peaks < 1 || plan.max_peaks > 127) return fail(err, RTP_EINVAL, "max_peaks %d out of range [1,127]", plan.max_peaks);
  plan.heat_channels = plan.blob_dims[plan.lowres_blob].first;
  if (plan.blob_dims[plan.lowres_blob].second != 3) return fail(err, RTP_EINVAL, "resize input must be at 1/8 resolution");
  {
    const int need = (plan.model == 0 ? 57 : 44);
    if (plan.heat_channels != need) return fail(err, RTP_EINVAL, "resize input has %d channels, model needs %d", plan.heat_channels, need);
  }
  return RTP_OK;
}

int Builder::lay_geometry() {
  plan.nlevels = max_level + 1;
  if ((in.net_w % 16) || (in.net_h % 16) || in.net_w < 16 || in.net_h < 16)
    return fail(err, RTP_EINVAL, "net_resolution %dx%d must be positive multiples of 16", in.net_w, in.net_h);
  for (int l = 0; l < plan.nlevels; ++l) {
    Geom g;
    g.N = plan.NI; g.H = in.net_h >> l; g.W = in.net_w >> l; g.halo = level_halo[l];
    // ONE zero gap of `halo` pixels between consecutive rows serves as the right halo of row y and the left halo of row y+1
    // (flat addressing: pixel p's tap (r,s) is p + (r-pad)*Wp + (s-pad), so x+pad past the row end lands in the gap and x-pad
    // before the row start lands in the previous row's gap).  Wp = W + halo instead of W + 2*halo: 3.4 % fewer GEMM rows at
    // 1/8 resolution (85 instead of 88 per row) and 31 instead of 32 M-tiles of 128 per 46x82 image — a launch of the paired
    // 7x7 layers at batch_frames = 2 is 248 workgroups, not 256: it no longer needs EVERY CU at once.
    // The last pixel's far corner tap reads 2 pixels past Hp*Wp: the next image's top halo / the tensor's zero guard.
    static const char* sh = RTP_EXP_ENV("RTP_HALO_SHARED");  // experiments: 0 = a halo on both sides of every row
    const bool shared = !(sh && sh[0] == '0');
    g.Hp = g.H + 2 * g.halo; g.Wp = g.W + (shared ? 1 : 2) * g.halo; g.img_pix = (long)g.Hp * g.Wp;
    plan.geom[l] = g;
  }
  plan.low_w = in.net_w / 8;
  plan.low_h = in.net_h / 8;
  return RTP_OK;
}

// every blob a convolution or pooling layer reads or writes gets a tensor; concat inputs become channel slices of the concat tensor
void Builder::make_tensors() {
  const int CALIGN = 128 / plan.elem;
  auto new_tensor = [&](const std::string& name, int C, int level) {
    Tensor t;
    t.name = name; t.C = C; t.level = level;
    t.Cp = round_up(C, CALIGN);
    t.chmap.resize(C);
    for (int i = 0; i < C; ++i) t.chmap[i] = i;
    plan.tensors.push_back(t);
    return (int)plan.tensors.size() - 1;
  };
  {  // packed im2col input
    Tensor t;
    t.name = "__im2col_input"; t.C = 27; t.level = 0; t.Cp = 32;
    t.chmap.resize(27);
    for (int i = 0; i < 27; ++i) t.chmap[i] = i;
    plan.tensors.push_back(t);
    packed_tensor = 0;
  }
  for (auto& c : plan.convs) plan.blob_tensor[c.name] = new_tensor(c.name, c.cout, c.level);
  for (auto& p : pools) plan.blob_tensor[p.out] = new_tensor(p.out, plan.blob_dims[p.out].first, plan.blob_dims[p.out].second);
  // concat tensors (those read by convolutions); aligned inputs first
  for (auto& kv : concats) {
    if (kv.first == plan.lowres_blob) continue;
    const auto& ins = kv.second.inputs;
    std::vector<int> ord(ins.size());
    for (size_t i = 0; i < ins.size(); ++i) ord[i] = (int)i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
      const bool ua = (plan.blob_dims[ins[a]].first % 8) != 0, ub = (plan.blob_dims[ins[b]].first % 8) != 0;
      return (int)ua < (int)ub;
    });
    std::vector<int> internal_off(ins.size());
    int off = 0;
    for (int i : ord) { internal_off[i] = off; off += plan.blob_dims[ins[i]].first; }
    {  // every slice on an 8-channel boundary where the pad channels of the tensor pay for it (concat_stageK: conv4_4_CPM at 0, L1 at 128, L2 at
       // 168 instead of 166, 192 channels either way): the producers' epilogues then write the slice with 16-byte stores instead of one 2-byte
       // store + two fp8 byte stores per channel (conv_common.h conv_store_dst) — the branch tails' epilogue was 4.1 us of an 11 us workgroup
       // for that reason.  The skipped channels are pad channels like the tail's: zero activations, zero weights (chmap never points at them).
      std::vector<int> aligned(ins.size());
      int a = 0;
      for (int i : ord) { a = round_up(a, 8); aligned[i] = a; a += plan.blob_dims[ins[i]].first; }
      if (round_up(a, CALIGN) == round_up(off, CALIGN)) internal_off = aligned;
    }
    const int tid = new_tensor(kv.first, plan.blob_dims[kv.first].first, plan.blob_dims[kv.first].second);
    plan.blob_tensor[kv.first] = tid;
    int refc = 0;
    for (size_t i = 0; i < ins.size(); ++i) {
      const int C = plan.blob_dims[ins[i]].first;
      for (int c = 0; c < C; ++c) plan.tensors[tid].chmap[refc + c] = internal_off[i] + c;
      refc += C;
      concat_slices[kv.first].push_back({ins[i], internal_off[i]});
    }
  }
  for (auto& p : pools) plan.pools.push_back({plan.blob_tensor.at(p.in), plan.blob_tensor.at(p.out), plan.tensors[plan.blob_tensor.at(p.out)].C});
}

int Builder::wire_convs() {
  for (auto& c : plan.convs) {
    const LayerDef* L = nullptr;
    for (auto& l : net.layers) if (l.type == "Convolution" && l.name == c.name) L = &l;
    if (c.first) c.in_tensor = packed_tensor;
    else {
      auto it = plan.blob_tensor.find(L->bottoms[0]);
      if (it == plan.blob_tensor.end()) return fail(err, RTP_EINVAL, "layer %s: bottom %s has no tensor", c.name.c_str(), L->bottoms[0].c_str());
      c.in_tensor = it->second;
    }
    c.dsts.push_back({plan.blob_tensor[c.name], 0});
    for (auto& cs : concat_slices)
      for (auto& sl : cs.second)
        if (sl.first == c.name) c.dsts.push_back({plan.blob_tensor[cs.first], sl.second});
    if ((int)c.dsts.size() > RTP_MAX_DST) return fail(err, RTP_EINVAL, "layer %s feeds %d tensors (max %d)", c.name.c_str(), (int)c.dsts.size(), RTP_MAX_DST);
    // low-res output (the blob ImResize reads), reference channel order
    if (c.name == plan.lowres_blob) { c.to_lowres = true; c.lowres_coff = 0; }
    else if (concats.count(plan.lowres_blob)) {
      int off = 0;
      for (auto& src : concats[plan.lowres_blob].inputs) {
        if (src == c.name) { c.to_lowres = true; c.lowres_coff = off; }
        off += plan.blob_dims[src].first;
      }
    }
    const Tensor& ti = plan.tensors[c.in_tensor];
    c.Cin_p = ti.Cp;
    c.rowb = (c.Cin_p * plan.elem >= 128) ? 128 : 64;
    if ((c.Cin_p * plan.elem) % c.rowb) return fail(err, RTP_EINVAL, "layer %s: internal channel padding error", c.name.c_str());
    c.nchunk = c.Cin_p * plan.elem / c.rowb;
  }
  return RTP_OK;
}

// split precision: which layers (which tensors must carry a lo / q block follows from the FINAL flags, propagate_split); then one step
// per launch, in layer order: the independent L1 / L2 branch convolutions of a stage, split alike, are paired into one
void Builder::make_steps() {
  for (auto& c : plan.convs) {
    layer_split(in, plan.prec, c, &c.split_w, &c.split_a, &c.no_h8);
    if (c.first) c.split_a = false;  // the image (u8/256 - 0.5) is exact in fp16: its lo part is zero
  }
  plan.steps.push_back({0, -1, -1});
  for (size_t oi = 0; oi < order.size(); ++oi) {
    if (order[oi].first == 2) { plan.steps.push_back({2, order[oi].second, -1}); continue; }
    const int a = order[oi].second;
    int b = -1;
    if (oi + 1 < order.size() && order[oi + 1].first == 1) {
      const int cand = order[oi + 1].second;
      const ConvOp& A = plan.convs[a];
      const ConvOp& B = plan.convs[cand];
      bool dep = false;
      for (auto& d : A.dsts) if (d.first == B.in_tensor) dep = true;
      if (!dep && A.split_a == B.split_a && A.split_w == B.split_w && A.k_eff == B.k_eff && A.Cin_p == B.Cin_p && A.level == B.level && A.relu == B.relu && A.rowb == B.rowb &&
          round_up(A.cout, 64) == round_up(B.cout, 64) && plan.tensors[A.in_tensor].Cp == plan.tensors[B.in_tensor].Cp)
        b = cand;
    }
    plan.steps.push_back({1, a, b});
    if (b >= 0) ++oi;
  }
}

// the tile of conv step si_ (both branches of a pair run the same kernel)
int Builder::choose_tile(size_t si_) {
  const Step& s = plan.steps[si_];
  const ConvOp& A = plan.convs[s.a];
  const Geom& g = plan.geom[A.level];
  // a pooling layer follows and reads only this blob: tiles the POOL kernel exists for save its launch (fusion pass below)
  const bool pool_next = s.b < 0 && si_ + 1 < plan.steps.size() && plan.steps[si_ + 1].type == 2 && A.dsts.size() == 1 &&
                         pools[plan.steps[si_ + 1].a].in == A.name && (g.H % 2) == 0 && (g.W % 2) == 0 && g.W >= 128 && !in.keep_blobs;
  const int nprob = s.b >= 0 ? 2 : 1;
  const int maxcout = std::max(A.cout, s.b >= 0 ? plan.convs[s.b].cout : 0);
  // Tile choice by a time model of the ring kernel (cycles; the constants are measured):
  //   one K step (tap x chunk) of a workgroup = max(MFMA time, L2->LDS time) + barrier:
  //     MFMA:  BM*BN*channels_per_chunk / (4 consumer waves * 32*32*16) instructions per wave at ~43 cycles on real operands
  //     DMA:   the weight tile (BN rows) + 1/k of the (BM+k-1)-pixel strip, at ~56 B/clk/CU
  //   a workgroup = steps * that + ~4500 cycles of prologue / epilogue; a launch = workgroups / 256 CUs rounds, where a partial
  //   round of fill f costs 0.5 + 0.5 f of a full one (fewer busy CUs clock higher and wait less for L2: 372 workgroups of the
  //   dominant shape take 1.70x the time of 248, not 2x), + ~6000 cycles of dispatch per launch.  (Two co-resident workgroups of
  //   the small-LDS 64x64 kernel share one matrix pipe: no credit for them.)
  // Replaces round 2's "fewest bytes among the tiles with >= 224 workgroups", which left plans whose M does not fill the chip
  // (MPI 46x62 maps at batch_frames 2: 192 workgroups of 128x64) on half-size tiles in two rounds.
  const bool ring_ok = !A.first && (A.k_eff == 3 || A.k_eff == 7);
  const int row_bytes_all = A.Cin_p * plan.elem;
  std::vector<int> cands;
  if (A.rowb == 64) cands = {CFG_128x64};
  else if (maxcout <= 32 && ring_ok && row_bytes_all % 256 == 0) cands = {CFG_128x32, CFG_128x64, CFG_64x64};
  else if (maxcout <= 64) cands = {CFG_128x64, CFG_64x64};
  else if (ring_ok && row_bytes_all % 256 == 0) {
    cands = {CFG_128x128, CFG_64x128, CFG_128x64, CFG_64x64, CFG_128x32};
    // CFG_256x64 (round 5): twice the pixels per workgroup for the 7x7 layers.  Alone at batches of 4 it is 12-14 % faster per image than the
    // 128x64 tile at batches of 2; in the PIPELINE it changes nothing (B = 4: 1012 vs 1006 frames/s against 128x128 tiles, MPI B = 5: 1209 vs
    // 1207; profiles/r05_experiments.txt), so the production plans keep round 4's measured tiles and the candidate exists in the experiments
    // build only (RTP_TILE_256=1: let the time model choose it; RTP_DOM_256 forces it).
    static const char* t256 = RTP_EXP_ENV("RTP_TILE_256");
    if (plan.prec == 0 && A.k_eff == 7 && maxcout >= 64 && ((t256 && t256[0] == '1') || RTP_EXP_ENV("RTP_DOM_256"))) cands.push_back(CFG_256x64);   // (chosen by the model where 128-pixel tiles would need two rounds: batches of >= 4 images)
  }
  else if (ring_ok) cands = {CFG_128x128, CFG_64x128, CFG_128x64, CFG_64x64};
  else cands = {CFG_128x128, CFG_64x128, CFG_64x64};
  int best = cands.back();
  double best_t = 1e300, best_bytes = 1e300;
  static const char* tm = RTP_EXP_ENV("RTP_TILE_RULE");  // experiments: "r2" = round 2's rule
  const bool rule_r2 = tm && !strcmp(tm, "r2");
  long best_wg = -1;
  bool chosen = false;
  const int passes = (A.split_a || A.split_w) ? ((in.split_fp8 && in.mode == RTP_PREC_MIXED && A.split_a && A.split_w && !A.no_h8 && ring_ok) ? 2 : 1 + (A.split_a ? 1 : 0) + (A.split_w ? 1 : 0)) : 1;
  for (int cf : cands) {
    const ConvCfgInfo ci = conv_cfg_info(cf);
    const long wg = conv_workgroups(plain_tiles_per_img(g, ci.BM), plan.NI, round_up(maxcout, ci.BN), ci.BN, nprob);
    const double bytes = (double)wg * (ci.BN + (double)(ci.BM + A.k_eff - 1) / A.k_eff);
    if (rule_r2) {
      if (wg >= 224) { if (!chosen || bytes < best_bytes) { best = cf; best_bytes = bytes; chosen = true; } }
      else if (!chosen && wg > best_wg) { best = cf; best_wg = wg; }
      continue;
    }
    const int chb = (ring_ok && (cf == CFG_64x64 || cf == CFG_128x64 || cf == CFG_128x32) && row_bytes_all % 256 == 0) ? 256 : std::min(128, row_bytes_all);
    const double chc = (double)chb / plan.elem;                                     // channels per chunk
    const double t_mfma = (double)ci.BM * ci.BN * chc / (4.0 * 32 * 32 * 16) * (plan.prec ? 4 * 43.0 : 43.0);
    const double t_dma = ((double)ci.BN * chb + (double)(ci.BM + A.k_eff - 1) * chb / A.k_eff) / 56.0;
    const double steps = (double)A.k_eff * A.k_eff * (row_bytes_all / (double)chb) * passes;
    const double t_wg = steps * (std::max(t_mfma, t_dma) + 60.0) + 4500.0;
    const double full = std::floor((double)wg / 256.0), frac = (double)wg / 256.0 - full;
    double t = (full + (frac > 0 ? 0.5 + 0.5 * frac : 0.0)) * t_wg + 6000.0;
    if (pool_next && !(plan.prec == 0 && A.k_eff == 3 && chb == 128 && (cf == CFG_128x64 || cf == CFG_128x128)))  // the stand-alone pooling launch: ~5 B per cycle and CU
      t += 8000.0 + (double)plan.NI * g.H * g.W * plan.tensors[A.dsts[0].first].stride() * plan.elem * 1.25 / (256.0 * 9.0);
    if (t < best_t * 0.98 || (t < best_t * 1.02 && bytes < best_bytes)) { best = cf; best_t = std::min(t, best_t); best_bytes = bytes; }
  }
  // Half-chip launches.  The runtime's hardware queues run two conv stacks at a time, so two launches of <= 128
  // workgroups share the chip: each workgroup moves half the weight bytes per MFMA and one stack's launch gaps are covered by the
  // other's kernel.  Measured in the pipeline, same box (profiles/r03_tile_model.txt): 128x128 tiles (124 workgroups at batch_frames 2)
  // for every k x k layer at 1/8 resolution +2.7 % frames/s, for all of them except the dominant shape +1.5..3 %.  A launch alone then
  // fills half the chip, which is what a per-launch roofline reports (0.16 instead of 0.23 for the dominant 7x7 128->128 pair).
  // RTP_HALF_CHIP: 1 (default) = where a 128x128 tile gives 100..128 workgroups and the model's choice 129..256, except the dominant
  // shape (whose per-launch efficiency is the figure this path is judged on); 2 = the dominant shape too; 0 = the model alone.
  if (!rule_r2 && ring_ok) {
    static const char* hc = RTP_EXP_ENV("RTP_HALF_CHIP");
    const int mode = hc ? atoi(hc) : 1;
    const ConvCfgInfo cb = conv_cfg_info(best);
    const long wg_best = conv_workgroups(plain_tiles_per_img(g, cb.BM), plan.NI, round_up(maxcout, cb.BN), cb.BN, nprob);
    const long wg_128 = conv_workgroups(plain_tiles_per_img(g, 128), plan.NI, round_up(maxcout, 128), 128, nprob);
    const bool has128 = std::find(cands.begin(), cands.end(), (int)CFG_128x128) != cands.end();
    const bool dominant = A.k_eff == 7 && A.cin == 128;
    if (mode > 0 && has128 && best != CFG_128x128 && wg_best > 128 && wg_best <= 256 && wg_128 >= 100 && wg_128 <= 128 && (mode >= 2 || !dominant))
      best = CFG_128x128;
  }
  if (int rc = tile_overrides(A, cands, ring_ok, maxcout, &best)) return rc;
  // tile, padded output channels and kernel (register-staged / ring with its chunk size) of the step's convolutions
  const ConvCfgInfo ci = conv_cfg_info(best);
  const char* force = RTP_EXP_ENV("RTP_CONV_IMPL");
  const bool allow_ring = !(force && !strcmp(force, "v1"));
  for (int idx : {s.a, s.b}) {
    if (idx < 0) continue;
    ConvOp& c = plan.convs[idx];
    c.cfg = best;
    c.CoutP = round_up(maxcout, ci.BN);
    c.impl = 0;
    if (allow_ring && !c.first && (c.k_eff == 3 || c.k_eff == 7)) {
      const int row_bytes = c.Cin_p * plan.elem;
      static const char* f128 = RTP_EXP_ENV("RTP_RING_CHB128");
      int chb = ((best == CFG_64x64 || best == CFG_128x64 || best == CFG_128x32) && row_bytes % 256 == 0 && !(f128 && f128[0] == '1')) ? 256 : 128;
      if (best == CFG_128x32 && chb != 256) { best = CFG_64x64; c.cfg = best; c.CoutP = round_up(maxcout, 64); chb = 128; }
      if (row_bytes % chb == 0) {
        c.impl = 1;
        c.rowb = chb;
        c.nchunk = row_bytes / chb;
      }
    }
  }
  return RTP_OK;
}

// experiments build: tiles forced from the environment
int Builder::tile_overrides(const ConvOp& A, const std::vector<int>& cands, bool ring_ok, int maxcout, int* best) {
  {
    static const char* d256 = RTP_EXP_ENV("RTP_DOM_256");   // experiments: 1 = 256x64 tiles for the 7x7 layers whatever the batch (half-chip launches of double-size workgroups at batch_frames 2); 2 = the dominant shape only
    if (d256 && ring_ok && A.k_eff == 7 && std::find(cands.begin(), cands.end(), (int)CFG_256x64) != cands.end() && (d256[0] == '1' || (d256[0] == '2' && A.cin == 128))) *best = CFG_256x64;
  }
  if (const char* ov = RTP_EXP_ENV("RTP_TILE_OVERRIDE")) {  // experiments: "conv2_1=3,conv3_1=3" forces tile ids (kernels.h ConvCfg) per layer
    const std::string key = A.name + "=";
    for (const char* hit = strstr(ov, key.c_str()); hit; hit = strstr(hit + 1, key.c_str())) {  // "Mconv2_1=.." also contains "conv2_1=": take the entry that starts at a boundary
      if (!(hit == ov || hit[-1] == ',')) continue;
      const int v = atoi(hit + key.size());
      if (std::find(cands.begin(), cands.end(), v) == cands.end())
        return fail(err, RTP_EINVAL, "RTP_TILE_OVERRIDE: tile id %d is not a candidate for layer %s", v, A.name.c_str());
      *best = v;
      break;
    }
  }
  {
    static const char* fc = RTP_EXP_ENV("RTP_FORCE_CFG");  // experiments only: force a tile for the k x k layers at 1/8 resolution
    static const char* kd = RTP_EXP_ENV("RTP_FORCE_CFG_KEEP_DOM");  // 1: ... except the dominant shape (7x7, 128 input channels)
    if (fc && ring_ok && A.level == 3 && maxcout > 64 && !(kd && kd[0] == '1' && A.k_eff == 7 && A.cin == 128)) {
      const int v = atoi(fc);
      if (std::find(cands.begin(), cands.end(), v) == cands.end())
        return fail(err, RTP_EINVAL, "RTP_FORCE_CFG: tile id %d is not a candidate for layer %s", v, A.name.c_str());
      *best = v;
    }
  }
  return RTP_OK;
}

// fp8 compensation where the kernel supports it: ring kernels whose waves own >= 64 bytes of K per chunk
void Builder::propagate_split() {
  for (auto& c : plan.convs) {
    // k-split of the kernel that would run it (conv_ring.hip; q layers on the 64x64 tile with 128-byte chunks get a 2-way split)
    const int ksplit = c.cfg == CFG_128x128 ? 1 : (c.cfg == CFG_64x64 ? (c.rowb == 128 ? 2 : 4) : 2);
    const int gpw = (c.rowb / 32) / ksplit;
    c.h8 = in.split_fp8 && in.mode == RTP_PREC_MIXED && plan.prec == 0 && c.impl == 1 && c.split_a && c.split_w && !c.no_h8 && gpw >= 2 && gpw % 2 == 0;
  }
  for (auto& s : plan.steps)  // both branches of a pair run the same kernel
    if (s.type == 1 && s.b >= 0 && plan.convs[s.a].h8 != plan.convs[s.b].h8)
      for (int idx : {s.a, s.b}) plan.convs[idx].h8 = false;
  for (auto& c : plan.convs)  // which operand blocks the input tensors must carry, from the FINAL flags
    if (c.split_a) { if (c.h8) plan.tensors[c.in_tensor].need_q = true; else plan.tensors[c.in_tensor].need_lo = true; }
  for (size_t pi = plan.pools.size(); pi-- > 0;) {  // a pool output with lo / q parts needs them in its input
    if (plan.tensors[plan.pools[pi].out_tensor].need_lo) plan.tensors[plan.pools[pi].in_tensor].need_lo = true;
    if (plan.tensors[plan.pools[pi].out_tensor].need_q) plan.tensors[plan.pools[pi].in_tensor].need_q = true;
  }
  // The branches of a pair share ONE description of their input (ConvParams: pixel pitch in_cstride, the q block's offset jump_delta / row_back).
  // Where the two input tensors carry different blocks — one of them has a further reader that runs other passes — the pair runs as two launches
  // on the tile chosen for it.  (The built-in graphs pair layers that read the same concat, or blobs with a single reader.)
  for (size_t si = 0; si < plan.steps.size(); ++si) {
    Step& s = plan.steps[si];
    if (s.type != 1 || s.b < 0) continue;
    const Tensor& ta = plan.tensors[plan.convs[s.a].in_tensor];
    const Tensor& tb = plan.tensors[plan.convs[s.b].in_tensor];
    if (ta.need_lo == tb.need_lo && ta.need_q == tb.need_q) continue;
    const int b = s.b;
    s.b = -1;
    plan.steps.insert(plan.steps.begin() + (long)si + 1, Step{1, b, -1});
  }
}

// 2x2 max pooling inside the producing convolution's epilogue: the pooling layer's input blob has no other consumer, the layer
// runs on a ring kernel with 128-pixel tiles of 128-byte chunks (the trunk's conv1_2 / conv2_2 / conv3_4), even resolution.
// The un-pooled blob is then never written (rtp_config.keep_blobs = 1 keeps every blob tappable and pools in its own launch).
void Builder::fuse_pools() {
  static const char* fp = RTP_EXP_ENV("RTP_FUSE_POOL");  // experiments: 0 = stand-alone pooling launches
  for (size_t si = 1; si < plan.steps.size() && !in.keep_blobs && !(fp && fp[0] == '0'); ++si) {
    if (plan.steps[si].type != 2 || plan.steps[si - 1].type != 1 || plan.steps[si - 1].b >= 0) continue;
    const int pi = plan.steps[si].a;
    ConvOp& A = plan.convs[plan.steps[si - 1].a];
    const PoolOp& po = plan.pools[pi];
    const Geom& g = plan.geom[A.level];
    bool ok = plan.prec == 0 && A.impl == 1 && A.k_eff == 3 && A.rowb == 128 && (A.cfg == CFG_128x64 || A.cfg == CFG_128x128) && !A.to_lowres &&
              A.dsts.size() == 1 && A.dsts[0].first == po.in_tensor && (g.H % 2) == 0 && (g.W % 2) == 0 && g.W >= 128 /* one wrap per tile at most */ && A.level + 1 < plan.nlevels;
    for (auto& c : plan.convs) if (c.in_tensor == po.in_tensor) ok = false;  // somebody convolves the un-pooled blob
    if (!ok) continue;
    A.pool = pi;
    A.dsts[0] = {po.out_tensor, 0};
    plan.tensors[po.in_tensor].written = false;
    plan.steps.erase(plan.steps.begin() + (long)si);
    --si;
  }
}

// the input convolution without the im2col tensor: fp16 storage, 64 channels, one plain destination
void Builder::direct_first_layer() {
  static const char* fd = RTP_EXP_ENV("RTP_FIRST_DIRECT");  // experiments: 0 = the pack + 1x1 route
  for (size_t si = 0; si + 1 < plan.steps.size() && !(fd && fd[0] == '0'); ++si) {
    const Step& s1 = plan.steps[si];
    if (s1.type != 1 || s1.b >= 0 || !plan.convs[s1.a].first) continue;
    ConvOp& c = plan.convs[s1.a];
    const Tensor& to = plan.tensors[c.dsts[0].first];
    if (plan.prec != 0 || c.cout != 64 || c.split_w || c.dsts.size() != 1 || c.to_lowres || to.need_lo || to.need_q || plan.steps[0].type != 0) break;
    if (((size_t)3 * (plan.geom[0].W + 2) * 3 + 8) * 2 > 64 * 1024) break;
    c.direct_first = true;
    plan.steps[0] = Step{4, s1.a, -1};
    plan.steps.erase(plan.steps.begin() + (long)si);
    break;
  }
}

// branch tails: 1x1 (ReLU) -> 1x1 with nobody else reading the middle blob become ONE launch (conv_pw2.hip)
void Builder::fuse_pw2() {
  static const char* nf = RTP_EXP_ENV("RTP_FUSE_1X1");
  const bool allow = plan.prec == 0 && !(nf && nf[0] == '0');
  for (size_t si = 0; allow && si + 1 < plan.steps.size(); ++si) {
    Step& s1 = plan.steps[si];
    const Step& s2 = plan.steps[si + 1];
    if (s1.type != 1 || s2.type != 1 || (s1.b >= 0) != (s2.b >= 0)) continue;
    auto chain = [&](int ia, int ic) {
      const ConvOp& A = plan.convs[ia];
      const ConvOp& C = plan.convs[ic];
      return A.k == 1 && C.k == 1 && !A.first && A.Cin_p == 128 && A.cout % 128 == 0 && A.cout <= 512 /* conv_pw2.hip PW_MAXMID */ && C.cin == A.cout && A.dsts.size() == 1 &&
             C.in_tensor == A.dsts[0].first && C.cout <= 64 && plan.tensors[A.dsts[0].first].C == A.cout;
    };
    if (!chain(s1.a, s2.a) || (s1.b >= 0 && !chain(s1.b, s2.b))) continue;
    if (s1.b >= 0 && (plan.convs[s1.a].cout != plan.convs[s1.b].cout)) continue;
    s1.type = 3; s1.a2 = s2.a; s1.b2 = s2.b;
    // the middle blob (Mconv6_stageK / conv5_4_CPM) lives in LDS between the two GEMMs; nobody reads it from memory: it is written only
    // when every blob must stay tappable (keep_blobs) — 32-128 KB of stores per workgroup and ~0.9 us of its ~11 us otherwise
    for (int idx : {s1.a, s1.b}) {
      if (idx < 0 || in.keep_blobs) continue;
      const int mid = plan.convs[idx].dsts[0].first;
      bool read_elsewhere = false;
      for (auto& c2 : plan.convs) if (c2.in_tensor == mid && &c2 != &plan.convs[idx == s1.a ? s1.a2 : s1.b2]) read_elsewhere = true;
      for (auto& po : plan.pools) if (po.in_tensor == mid) read_elsewhere = true;
      if (!read_elsewhere) plan.tensors[mid].written = false;
    }
    for (int idx : {s1.a, s1.b}) if (idx >= 0) { ConvOp& A = plan.convs[idx]; A.fused = 1; A.fused_chunks = A.cout / 128; A.CoutP = A.cout; }
    for (int idx : {s1.a2, s1.b2}) if (idx >= 0) { ConvOp& C = plan.convs[idx]; C.fused = 2; C.fused_chunks = C.cin / 128; C.CoutP = 64; }
    plan.steps.erase(plan.steps.begin() + si + 1);
  }
}

// activation arena of a context, weight arena of the engine
void Builder::lay_arenas() {
  size_t off = 0;
  for (auto& t : plan.tensors) {
    if (!t.written) { t.offset = 0; continue; }  // fused away (its convolution pools in the epilogue): never read, never written, no space
    const Geom& g = plan.geom[t.level];
    const size_t pix_bytes = (size_t)t.stride() * plan.elem;
    off = round_up_sz(off, 256);
    off += GUARD_PIX * pix_bytes;
    off = round_up_sz(off, 256);
    t.offset = off;
    off += (size_t)plan.NI * g.img_pix * pix_bytes + GUARD_PIX * pix_bytes;
  }
  plan.arena_bytes = round_up_sz(off, 256) + (4u << 20);  // tail pad: the ring kernel's dummy prefetches read past the last strip
  // weight arena
  size_t woff = 0;
  for (auto& c : plan.convs) {
    c.ncp = c.nchunk;   // K chunks: one pass = ncp chunks of rowb bytes; split layers run 2-3 passes (h8: hi chunks + q chunks)
    c.nchunk = c.ncp * c.passes();
    c.w_bytes = (size_t)c.k_eff * c.k_eff * c.nchunk * c.CoutP * c.rowb;
    if (c.fused == 1) c.w_bytes = (size_t)c.fused_chunks * (c.split_w ? 2 : 1) * 128 * 256;
    if (c.fused == 2) c.w_bytes = (size_t)c.fused_chunks * (c.split_w ? 2 : 1) * 64 * 256;
    if (c.direct_first) c.w_bytes = 2 * 2 * 64 * 16;
    woff = round_up_sz(woff, 256);
    c.w_off = woff;
    woff += c.w_bytes;
    woff = round_up_sz(woff, 256);
    c.b_off = woff;
    woff += (size_t)c.CoutP * sizeof(float);
  }
  plan.weights_bytes = round_up_sz(woff, 256) + (1u << 20);  // tail pad: dummy weight-tile prefetches of the last layer
  // dominant conv step for the roofline probe: the first paired 7x7 step whose input is not a concat
  for (size_t si = 0; si < plan.steps.size(); ++si) {
    const Step& s = plan.steps[si];
    static const char* dq = RTP_EXP_ENV("RTP_DOMINANT_Q");  // profiling: 1 = probe the first fp8-compensated launch of that shape instead (stage 4)
    if (s.type == 1 && plan.convs[s.a].k == 7 && plan.convs[s.a].cin == 128 && (!(dq && dq[0] == '1') || plan.convs[s.a].h8)) { plan.dominant_step = (int)si; break; }
  }
}

int Builder::postproc_sizes() {
  plan.strip_rows = in.N > 1 ? 16 : 8;  // several scales: the row interpolations of a strip are the larger share, taller strips amortise them (+3 % frames/s at 3 scales)
  if (const char* sr = RTP_EXP_ENV("RTP_NMS_STRIP_ROWS")) { const int v = atoi(sr); if (v >= 2 && v <= 16) plan.strip_rows = v; }  // experiments
  // the strip kernel keeps (strip_rows + 2 + NMSF_TROWS) rows of W floats + a W x 8-byte column table in LDS (postproc.hip, 150 KiB cap)
  while (plan.strip_rows > 2 && ((size_t)(plan.strip_rows + 2 + 8 /* NMSF_TROWS */) * in.net_w * 4 + (size_t)in.net_w * 8) > 150 * 1024) plan.strip_rows /= 2;
  if (((size_t)(plan.strip_rows + 2 + 8 /* NMSF_TROWS */) * in.net_w * 4 + (size_t)in.net_w * 8) > 150 * 1024)
    return fail(err, RTP_EINVAL, "net_resolution width %d is too large for the fused ImResize+Nms strip kernel", in.net_w);
  plan.nstrips = (in.net_h + plan.strip_rows - 1) / plan.strip_rows;
  plan.max_rows = plan.num_limbs * plan.max_peaks;
  {
    // connect kernels: sort keys hold 7-bit peak ordinals; the subset table is int16 in LDS
    const size_t lds2 = (size_t)plan.max_rows * (sizeof(double) + sizeof(short) + sizeof(short) * plan.num_parts);
    if (plan.max_peaks > 127 || lds2 > 150 * 1024) return fail(err, RTP_EINVAL, "max_peaks %d out of range [1,127]", plan.max_peaks);
  }
  return RTP_OK;
}

}  // namespace

int build_plan(const PlanInput& in, Plan* out, std::string* err) {
  Builder b(in, err);
  int rc;
  if ((rc = b.walk_graph()) || (rc = b.lay_geometry())) return rc;
  b.make_tensors();
  if ((rc = b.wire_convs())) return rc;
  b.make_steps();
  for (size_t si = 0; si < b.plan.steps.size(); ++si)
    if (b.plan.steps[si].type == 1 && (rc = b.choose_tile(si))) return rc;
  b.propagate_split(); b.fuse_pools(); b.direct_first_layer(); b.fuse_pw2(); b.lay_arenas();
  if ((rc = b.postproc_sizes())) return rc;
  *out = std::move(b.plan);
  return RTP_OK;
}

PlanInput plan_input_from_config(const rtp_config& cfg, const NetDef* net) {
  const char* sr = RTP_EXP_ENV("RTP_SPLIT_LAYERS");  // experiments: override the split set of RTP_PREC_MIXED
  const char* f8 = RTP_EXP_ENV("RTP_SPLIT_FP8");
  return {net, cfg.net_w, cfg.net_h, cfg.num_scales, cfg.batch_frames < 1 ? 1 : cfg.batch_frames, cfg.precision,
          sr ? sr : (cfg.split_layers ? cfg.split_layers : kDefaultSplit), !(f8 && f8[0] == '0'), cfg.keep_blobs};
}

int load_netdef(const char* proto_path, int model, bool name_file, NetDef* net, std::string* err) {
  if (proto_path) {
    std::ifstream f(proto_path);
    if (!f) return fail(err, RTP_EIO, "cannot open prototxt %s", proto_path);
    std::stringstream ss;
    ss << f.rdbuf();
    std::string perr;
    if (!parse_prototxt(ss.str(), net, &perr))
      return name_file ? fail(err, RTP_EIO, "prototxt %s: %s", proto_path, perr.c_str()) : fail(err, RTP_EIO, "%s", perr.c_str());
  } else {
    if (model != RTP_MODEL_COCO_18 && model != RTP_MODEL_MPI_15) return fail(err, RTP_EINVAL, "unknown model %d", model);
    *net = build_linevec(model);
  }
  return RTP_OK;
}

long conv_tiles_per_img(const Plan& p, const ConvOp& c) {
  const Geom& g = p.geom[c.level];
  const int BM = conv_cfg_info(c.cfg).BM;
  return c.pool >= 0 ? tiles_of((long)(g.H / 2) * pool_wq(g, c), BM / 2) : plain_tiles_per_img(g, BM);
}

long step_workgroups(const Plan& p, const Step& s) {
  if (s.type != 1 && s.type != 3 && s.type != 4) return 0;
  const ConvOp& A = p.convs[s.a];
  const int nprob = s.b >= 0 ? 2 : 1;
  if (s.type == 4) return (long)p.geom[A.level].H * p.NI;   // conv_first.hip: a workgroup per image row
  if (s.type == 3) return conv_workgroups(plain_tiles_per_img(p.geom[A.level], 64), p.NI, 64, 64, nprob);   // conv_pw2.hip: 64 pixels, every output channel
  return conv_workgroups(conv_tiles_per_img(p, A), p.NI, A.CoutP, conv_cfg_info(A.cfg).BN, nprob);
}

int plan_contexts(int frames_in_flight, int B) { return (frames_in_flight + B - 1) / B + (B > 1 ? 1 : 0); }

// F frames in flight hold the fewest slots of the most contexts when the oldest batch has one frame left and the newest has one frame in:
// B - 1 empty slots in all, so ceil((F + B - 1) / B) contexts.  open_slot opens the LOWEST idle context, so with in-order collects the
// contexts from this number on are never opened (tests/test_hwq_placement.py simulates the loop); they exist for out-of-order callers.
int plan_busy_contexts(int frames_in_flight, int B) { return std::min(plan_contexts(frames_in_flight, B), (frames_in_flight + 2 * B - 2) / B); }

const char* plan_stream_arrangement(int frames_in_flight, int B, int hw_queues) {
  return (plan_contexts(frames_in_flight, B) <= hw_queues || B == 1) ? "one_per_context" : "per_frame_chains";
}

// The busy contexts fit the queues and the allocated ones do not; batches of 2 (a conv stream and one chain stream per queue: the candidate
// pool of engine.cpp place_streams is sized for that), no unused pad streams in between
bool plan_queue_placement(int frames_in_flight, int B, int hw_queues, int pad_streams) {
  const int busy = plan_busy_contexts(frames_in_flight, B);
  return B > 1 && busy <= hw_queues && hw_queues < plan_contexts(frames_in_flight, B) && pad_streams == 0 && B <= 2 && hw_queues <= 16;
}

// Streams that ran alone on their queue in a pair probe are on different queues; `share[a * n + b]` says that candidates a and b waited for
// each other (1), ran side by side (0) or that the probe could not tell (-1).  Picks `busy` groups of `per` candidates each such that every
// group shares one queue and no two groups share one: pick[g * per + j] = candidate index.  False when the map does not allow it.
bool plan_pick_queue_groups(const std::vector<int>& share, int n, int busy, int per, std::vector<int>* pick) {
  pick->clear();
  if (n <= 0 || (int)share.size() != n * n || busy < 1 || per < 1) return false;
  std::vector<int> cls(n, -1);   // queue class of every candidate: the lowest candidate it shares a queue with
  for (int a = 0; a < n; ++a) {
    for (int b = 0; b < a && cls[a] < 0; ++b) {
      if (share[a * n + b] < 0) return false;
      if (share[a * n + b] == 1) cls[a] = cls[b];
    }
    if (cls[a] < 0) cls[a] = a;
  }
  for (int a = 0; a < n; ++a)      // the relation must be an equivalence: anything else is a mis-measurement
    for (int b = 0; b < a; ++b)
      if (share[a * n + b] < 0 || (share[a * n + b] == 1) != (cls[a] == cls[b])) return false;
  for (int rep = 0; rep < n && (int)pick->size() < busy * per; ++rep) {
    if (cls[rep] != rep) continue;
    std::vector<int> members;
    for (int a = rep; a < n && (int)members.size() < per; ++a) if (cls[a] == rep) members.push_back(a);
    if ((int)members.size() == per) pick->insert(pick->end(), members.begin(), members.end());
  }
  if ((int)pick->size() != busy * per) { pick->clear(); return false; }
  return true;
}

}  // namespace rtp

// The stream rules above for the tests (host only; not part of the public header).  out = {contexts, busy contexts, 1 where every context
// has one stream, 1 where the busy contexts' streams are placed on queues of their own}
extern "C" int rtp_internal_stream_rules(int frames_in_flight, int B, int hw_queues, int pad_streams, int out[4]) {
  if (frames_in_flight < 1 || B < 1 || hw_queues < 1 || !out) return RTP_EINVAL;
  out[0] = rtp::plan_contexts(frames_in_flight, B);
  out[1] = rtp::plan_busy_contexts(frames_in_flight, B);
  out[2] = !strcmp(rtp::plan_stream_arrangement(frames_in_flight, B, hw_queues), "one_per_context");
  out[3] = rtp::plan_queue_placement(frames_in_flight, B, hw_queues, pad_streams);
  return RTP_OK;
}
// plan_pick_queue_groups: share = n x n ints (1 one queue, 0 side by side, -1 unknown), pick = busy * per ints; returns 1 / 0
extern "C" int rtp_internal_pick_queue_groups(const int* share, int n, int busy, int per, int* pick) {
  if (!share || !pick || n < 1 || n > 64) return RTP_EINVAL;
  std::vector<int> got;
  if (!rtp::plan_pick_queue_groups(std::vector<int>(share, share + (size_t)n * n), n, busy, per, &got)) return 0;
  std::copy(got.begin(), got.end(), pick);
  return 1;
}

namespace rtp {

std::string describe_plan(const Plan& p, int N, int B, int frames_in_flight, int hw_queues) {
  std::ostringstream o;
  o << "model " << p.model << " parts " << p.num_parts << " max_peaks " << p.max_peaks << " heat_channels " << p.heat_channels << "\n";
  for (int l = 0; l < p.nlevels; ++l)
    o << "level " << l << " H " << p.geom[l].H << " W " << p.geom[l].W << " halo " << p.geom[l].halo << "\n";
  o << "postproc strip_rows " << p.strip_rows << " nstrips " << p.nstrips << " max_rows " << p.max_rows << "\n";   // Builder::postproc_sizes
  o << "arena_bytes " << p.arena_bytes << " weights_bytes " << p.weights_bytes << " tensors " << p.tensors.size() << "\n";
  {  // which streams a batch context gets (alloc_ctx; "hardware queues" above): one for everything when the runtime's hardware queues suffice
    const int nctx = plan_contexts(frames_in_flight, B);
    // busy: the contexts an in-order caller ever opens (plan_busy_contexts); where they fit the queues and the allocated ones do not, the
    // per-frame chains are placed on their own context's queue (engine.cpp place_streams)
    o << "streams contexts " << nctx << " hw_queues " << hw_queues << " arrangement " << plan_stream_arrangement(frames_in_flight, B, hw_queues)
      << " busy " << plan_busy_contexts(frames_in_flight, B) << "\n";
  }
  double gflop = 0, mfma_gflop = 0;
  for (auto& s : p.steps) {
    if (s.type == 0) o << "step pack\n";
    else if (s.type == 4) {
      const ConvOp& c = p.convs[s.a];
      o << "step first " << c.name << " k 3 cin 3 cout " << c.cout << " relu " << c.relu << " passes 1 wgs " << step_workgroups(p, s) << "\n";
    } else if (s.type == 2) o << "step pool " << p.tensors[p.pools[s.a].in_tensor].name << " -> " << p.tensors[p.pools[s.a].out_tensor].name << "\n";
    else if (s.type == 3) {
      const ConvOp& A = p.convs[s.a];
      const ConvOp& C = p.convs[s.a2];
      o << "step pw2 " << A.name;
      if (s.b >= 0) o << " + " << p.convs[s.b].name;
      o << " -> " << C.name;
      if (s.b2 >= 0) o << " + " << p.convs[s.b2].name;
      o << " k 1 cin_p " << A.Cin_p << " mid " << A.cout << " cout " << C.cout << " passes " << A.passes() << (A.split_a ? "a" : "") << (A.split_w ? "w" : "") << "/"
        << C.passes() << (C.split_a ? "a" : "") << (C.split_w ? "w" : "") << " tile 64 wgs " << step_workgroups(p, s)
        << " lowres " << C.to_lowres << "\n";
    } else {
      const ConvOp& A = p.convs[s.a];
      const ConvCfgInfo ci = conv_cfg_info(A.cfg);
      o << "step conv " << A.name;
      if (A.pool >= 0) o << " +pool";
      if (s.b >= 0) o << " + " << p.convs[s.b].name;
      o << " k " << A.k << " cin_p " << A.Cin_p << " cout " << A.cout << " coutp " << A.CoutP << " relu " << A.relu << " tile " << ci.BM << "x" << ci.BN
        << " rowb " << A.rowb << " passes " << A.passes() << (A.h8 ? "q" : "") << (!A.h8 && A.split_a ? "a" : "") << (!A.h8 && A.split_w ? "w" : "") << " impl " << (A.impl ? "ring" : "reg") << " wgs " << step_workgroups(p, s) << " dsts " << A.dsts.size() << " lowres " << A.to_lowres << "\n";
    }
    for (int idx : {s.a, s.b, s.a2, s.b2}) if (idx >= 0 && s.type != 0 && s.type != 2) {   // every convolution of the step, at the step's resolution
      const ConvOp& c = p.convs[idx];
      const Geom& g = p.geom[p.convs[s.a].level];
      const double gf = 2.0 * c.cout * c.cin * c.k * c.k * (double)g.H * g.W * N * 1e-9;
      gflop += gf;
      mfma_gflop += gf * c.passes();
    }
  }
  o << "conv_gflop " << gflop << "\n";
  o << "mfma_gflop " << mfma_gflop << "\n";
  return o.str();
}

}  // namespace rtp

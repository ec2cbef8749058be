// plan.h — the static execution plan: what is computed ONCE per (graph, resolution, scales, batch, precision mode, split rules,
// keep_blobs) on the host, without a device.  build_plan() is a pure function PlanInput -> Plan (plan.cpp); the engine (engine.cpp)
// holds one Plan, materialises it (arenas, packed weights, contexts, graphs) and launches its steps.
#pragma once

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rtpose_mi355x.h"
#include "kernels.h"
#include "netdef.h"

namespace rtp {

inline int round_up(int v, int a) { return (v + a - 1) / a * a; }
inline size_t round_up_sz(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Tensor {
  std::string name;
  int C = 0, Cp = 0, level = 0;
  size_t offset = 0;        // byte offset of padded pixel 0 of image 0 inside a context arena
  std::vector<int> chmap;   // reference channel -> internal channel
  // split precision: [0, Cp) hi; need_lo: [Cp, 2Cp) lo = T(v - float(T(v))) (consumers running three fp16 passes);
  // need_q: a further Cp elements = 2*Cp bytes of fp8 compensation operands (consumers running the fp8 passes, ConvDst::q_off)
  bool need_lo = false, need_q = false;
  bool written = true;      // false: the blob was fused away (a convolution pools in its epilogue and writes only the pooled tensor)
  int stride() const { return Cp * (1 + (need_lo ? 1 : 0) + (need_q ? 1 : 0)); }  // channels (elements) per pixel in memory
  int lo_off() const { return need_lo ? Cp : 0; }
  int q_off() const { return need_q ? Cp * (need_lo ? 2 : 1) : 0; }
};

struct ConvOp {
  std::string name;
  int widx = 0;             // index into engine weights
  int in_tensor = -1;
  int k = 1, k_eff = 1;     // k_eff = 1 for the im2col-packed first layer
  int cin = 0, cout = 0;
  bool relu = false, first = false;
  std::vector<std::pair<int, int>> dsts;  // (tensor, channel offset)
  bool to_lowres = false;
  int lowres_coff = 0;
  int level = 0;
  int Cin_p = 0, rowb = 128, nchunk = 1, CoutP = 0, cfg = 0;
  int impl = 0;             // 0 = register-staged kernel (conv_igemm.hip), 1 = LDS-DMA ring (conv_ring.hip)
  bool direct_first = false;  // conv1_1 straight from the NCHW input (conv_first.hip): no im2col tensor, no pack step
  // split precision (RTP_PREC_MIXED / F16X3): the K loop runs the passes [a_hi x W_hi] [a_lo x W_hi] [a_hi x W_lo]
  bool split_a = false, split_w = false;
  bool no_h8 = false;       // rule suffix ":x": the corrections of this layer run as fp16 passes even where the fp8 chunk exists (no e4m3 range limits)
  int ncp = 1;              // chunks of ONE pass (nchunk = ncp * passes)
  bool h8 = false;          // the two correction passes run as ONE fp8 chunk per channel group (MX-scaled MFMA, 2x the fp16 rate)
  int wq_exp = 0;           // h8: fp8(W * 2^wq_exp), fp8(W_lo * 2^(wq_exp + 11)).  The ONE plan field that depends on the weights:
                            // build_plan leaves it 0, the engine fills it when it packs them (engine.cpp compute_wq_exp)
  int passes() const { return h8 ? 2 : 1 + (split_a ? 1 : 0) + (split_w ? 1 : 0); }  // in units of one fp16 pass of MFMA time
  int wrap_at() const { return h8 ? 0 : (split_w ? (split_a ? 2 * ncp : ncp) : 0); }
  int last_phys() const { return h8 ? ncp - 1 : (split_w ? ncp - 1 : (split_a ? 2 * ncp - 1 : ncp - 1)); }
  int pool = -1;            // >= 0: this convolution's only consumer is pooling layer `pool`; it pools in its epilogue (conv_ring.hip POOL)
  int fused = 0;            // 1 / 2: first / second 1x1 of a conv_pw2 step (weights packed for that kernel)
  int fused_chunks = 0;     // middle channels / 128
  size_t w_off = 0, b_off = 0, w_bytes = 0;
};

struct Step {
  int type;  // 0 pack, 1 conv, 2 pool, 3 two chained 1x1 convolutions in one launch (conv_pw2.hip), 4 input convolution from the NCHW image (conv_first.hip)
  int a = -1, b = -1;    // conv (a) [+ the other branch's conv (b)]; pool index for type 2
  int a2 = -1, b2 = -1;  // type 3: the second 1x1 of each branch
};

struct PoolOp { int in_tensor, out_tensor, C; };

// Everything build_plan produces, and nothing else
struct Plan {
  int model = 0, prec = 0, elem = 2;   // prec selects the kernels' element type (0 fp16, 1 fp32), elem = its bytes
  int num_parts = 18, max_peaks = 64, heat_channels = 57, num_limbs = 19;
  int low_w = 0, low_h = 0;
  int NI = 1;   // images per conv launch at a full batch = N * B
  Geom geom[8];
  int nlevels = 0;
  std::vector<Tensor> tensors;
  std::map<std::string, int> blob_tensor;                 // blob name -> tensor (NHWC blobs)
  std::map<std::string, std::pair<int, int>> blob_dims;   // blob name -> (C, level)
  std::string lowres_blob;
  std::vector<ConvOp> convs;
  std::vector<Step> steps;
  std::vector<PoolOp> pools;
  size_t arena_bytes = 0, weights_bytes = 0;
  int dominant_step = -1;
  int nstrips = 0, strip_rows = 8, max_rows = 0;
};

// Everything the plan depends on (besides the RTP_EXP_ENV knobs of the experiments build, read where the decisions are)
struct PlanInput {
  const NetDef* net = nullptr;
  int net_w = 0, net_h = 0;
  int N = 1;    // images per frame (num_scales)
  int B = 1;    // frames per batch
  int mode = 0; // RTP_PREC_*
  std::string split_rules;
  bool split_fp8 = true;    // RTP_SPLIT_FP8=0: split layers run three fp16 passes everywhere
  int keep_blobs = 0;
};

extern const char* const kDefaultSplit;
// which operands of layer c the rules split (x: corrections as fp16 passes); prec = the plan's element type
void layer_split(const PlanInput& in, int prec, const ConvOp& c, bool* w, bool* a, bool* x = nullptr);

// Always starts from a fresh Plan; on failure *out is untouched, *err has the message and the RTP_E* code is returned
int build_plan(const PlanInput& in, Plan* out, std::string* err);

// rtp_config -> PlanInput, and the NetDef of a config: the prototxt file, or the built-in graph of `model` when proto_path is null.
// name_file: a parse error names the file (engine creation does, the summary does not)
PlanInput plan_input_from_config(const rtp_config& cfg, const NetDef* net);
int load_netdef(const char* proto_path, int model, bool name_file, NetDef* net, std::string* err);

// ---- workgroups per launch: the one definition (tile model, launches, summary; tests/test_design_invariants.py restates the POOL walk)
inline long tiles_of(long pixels, int BM) { return (pixels + BM - 1) / BM; }
// M-tiles of one image: H x Wp flat pixels in tiles of BM
inline long plain_tiles_per_img(const Geom& g, int BM) { return tiles_of((long)g.H * g.Wp, BM); }
// POOL: pitch of the tile walk = W + pad rounded up to even, so that every tile starts on an even x
inline int pool_wq(const Geom& g, const ConvOp& c) { return (g.W + c.k_eff / 2 + 1) & ~1; }
// ... of convolution c as planned: POOL walks tiles of 2 image rows x BM/2 pixels
long conv_tiles_per_img(const Plan& p, const ConvOp& c);
inline long conv_workgroups(long tiles_per_img, int NI, int coutp, int BN, int nprob) { return tiles_per_img * NI * (coutp / BN) * nprob; }
long step_workgroups(const Plan& p, const Step& s);   // of a full batch

int plan_contexts(int frames_in_flight, int B);   // batches in flight (+1 being filled)
int plan_busy_contexts(int frames_in_flight, int B);   // ... of which a caller that collects in order ever opens this many
const char* plan_stream_arrangement(int frames_in_flight, int B, int hw_queues);   // "one_per_context" / "per_frame_chains"
// per_frame_chains with the busy contexts' streams placed on hardware queues of their own: busy <= queues < contexts
bool plan_queue_placement(int frames_in_flight, int B, int hw_queues, int pad_streams);
// which candidate streams become the busy contexts' streams, from the measured "these two share a queue" map (pure; plan.cpp)
bool plan_pick_queue_groups(const std::vector<int>& share, int n, int busy, int per, std::vector<int>* pick);

// the text of rtp_plan_summary
std::string describe_plan(const Plan& p, int N, int B, int frames_in_flight, int hw_queues);

}  // namespace rtp

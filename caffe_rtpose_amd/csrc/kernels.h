// kernels.h — device-side contracts shared by the HIP kernels and the engine (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "jpeg_bound.h"
#include "jpeg_dec.h"

// Experiment knobs (tile overrides, ablation variants of the ring kernel — some of which compute WRONG results on purpose, stream
// plans, diagnostic probes) exist only in the second build target librtpose_mi355x_exp.so (-DRTP_EXPERIMENTS, used by tools/):
// in the production library the macro is a null pointer and the knob's name is not even a string in the binary
// (tests/test_host_cpu.py greps for them).  The production library reads ONE environment variable: RTP_EXEC=eager|graph.
#ifdef RTP_EXPERIMENTS
#define RTP_EXP_ENV(name) getenv(name)
#else
#define RTP_EXP_ENV(name) ((const char*)nullptr)
#endif

namespace rtp {

// Kernel residency stamps (rtp_stamp_probe, bench.py `idle_frac_kernel_stamps`): when a launch carries a slot pointer, thread 0 of every
// workgroup folds the 100 MHz wall clock (s_memrealtime: one clock for all XCDs, tools/clock_sync_probe.hip) into the slot when the
// workgroup starts and when it ends: slot[0] = max(~start) = ~(first workgroup's start), slot[1] = max(end) = the last workgroup's end.
// Null pointer (every launch outside a probe run): one scalar compare per workgroup.
#if defined(__HIPCC__)
struct KStamp {
  unsigned long long* s;
  __device__ __forceinline__ explicit KStamp(unsigned long long* p) : s(p) {
    if (s && threadIdx.x == 0 && threadIdx.y == 0) atomicMax(s, ~wall_clock64());
  }
  __device__ __forceinline__ ~KStamp() {
    if (s && threadIdx.x == 0 && threadIdx.y == 0) atomicMax(s + 1, wall_clock64());
  }
};
#endif

// ---------------------------------------------------------------------------------------
// Activation layout in HBM: NHWC with a zero spatial halo, one geometry per resolution level.
//   element (n, y, x, c) lives at  base + ((n*Hp + y+halo)*Wp + x+halo)*Cp + c
// Hp = H+2*halo, Wp = W+2*halo.  Halo pixels and pad channels are zeroed once at allocation
// and never written, so a k x k convolution with pad <= halo needs no bounds test: tap (r,s)
// of output pixel p (flat padded index) reads flat pixel p + (r-pad)*Wp + (s-pad).
// ---------------------------------------------------------------------------------------
struct Geom {
  int N, H, W, halo, Hp, Wp;
  long img_pix;  // Hp*Wp
};

#define RTP_MAX_DST 6
struct ConvDst {
  void* base;   // element pointer of (n=0, padded pixel 0, channel 0)
  int cstride;  // channels per pixel of the destination tensor (2*Cp when it carries a lo block)
  int coff;     // first channel this conv writes
  int lo_off;   // 0, or the channel offset of the tensor's lo block: channel c also gets lo = T(v - float(T(v))) at lo_off + c
  int q_off;    // 0, or the ELEMENT offset of the tensor's q block (fp8 error-compensation operands): per 64-channel group g,
                // bytes [128g, 128g+64) = fp8(lo * 2^12), bytes [128g+64, 128g+128) = fp8(T(v) * 2^2)   (e4m3, clamped to +-448)
};

struct ConvProblem {
  const void* in;     // element pointer of (n=0, padded pixel 0, channel 0)
  const void* w;      // packed weights [tap][chunk][CoutP][ROWB bytes]
  const float* bias;  // [CoutP] fp32
  ConvDst dst[RTP_MAX_DST];
  int ndst;
  float* out_nchw;  // optional fp32 planar output [N][out_C][H][W]
  int out_C, out_coff;
  int Cout;
};

struct ConvParams {
  ConvProblem prob[2];  // blockIdx.z selects (the L1 / L2 branch pair shares every shape)
  int H, W, Wp, halo;
  long img_pix;
  int in_cstride;  // channels per pixel of the input tensor (2*Cp when it carries a lo block)
  int nchunk;      // K chunks per filter row.  Plain layer: Cin_p*sizeof(T)/ROWB.  Split-precision layer: the passes
                   // [a_hi x W_hi][a_lo x W_hi][a_hi x W_lo] are further chunks of the same K loop (weights are
                   // packed in that order); the ACTIVATION chunk of virtual chunk v is v, or v - wrap_at from wrap_at on
  int wrap_at;     // 0 = no wrap (the chunks are contiguous in the input tensor)
  int last_phys;   // physical chunk index of the last virtual chunk (nchunk-1 without a wrap)
  // fp8-compensated split layers (ring kernels): virtual chunks [q_from, nchunk) are q chunks — the same channel groups once
  // more, as fp8 pairs (a_lo8 x W8, a8 x W_lo8) multiplied by v_mfma_scale_f32_32x32x64_f8f6f4 at twice the fp16 rate
  int q_from;      // 0 = none
  int wq_exp;      // the weights' q chunks hold fp8(W * 2^wq_exp) and fp8(W_lo * 2^(wq_exp + 11)); one exponent for both branches
                   // of a paired launch (a per-problem field read through prob[blockIdx-dependent] made hipcc keep the DMA base
                   // pointer in VGPRs)
  int jump_delta;  // bytes from the last hi chunk to the first q chunk of the input tensor (instead of + CHB)
  int row_back;    // byte offset of a filter row's last virtual chunk relative to its first (ring kernels)
  int CoutP;       // Cout rounded up to a multiple of BN
  int tiles_per_img;
  int nimg;    // images (scales) in the batch
  int relu;
  int rotate;  // ring kernel: rotate the filter-row order per tile (speed only)
  int xcdmap;  // 1: contiguous logical range per XCD, pixel tiles fastest (decode_block), 2: the same with N tiles fastest, 0: dispatch order
  int ring_sb; // ring depth request (4 or 6) where both are instantiated
  int spec;    // ring kernel: 1 = wave-specialised variant (4 DMA waves + 4 MFMA waves)
  int variant; // ring kernel experiments (env RTP_RING_VAR; see conv_ring.hip), 0 = production
  int ilv;     // ring kernel (wave-specialised, fp16): interleaved A-fragment rows, taps 1.. of a strip shift registers instead of re-reading LDS
  // fused 2x2 max pooling (ring kernels, conv_ring.hip POOL): the M tile is 2 image rows x BM/2 pixels, the epilogue writes only the
  // pooled tensor.  pool_wq = W + pad rounded up to even (pitch of the tile walk, so that every tile starts on an even x); pool_* =
  // geometry of the pooled (next) level
  int pool, pool_wq, pool_Wp, pool_halo;
  long pool_img_pix;
  int diag;    // experiments build (env RTP_EPI_DIAG; timing only, wrong results): 1 = the epilogue computes but does not store, 2 = no epilogue at all
  unsigned long long* stamp;     // kernel residency slot (KStamp) or null
  unsigned long long* clkprobe;  // diagnostics: {shader clock cycles, wall clock ticks} of workgroup 0 (spec ring kernels)
};

// which tile configuration a conv launch uses
enum ConvCfg { CFG_128x128 = 0, CFG_64x128 = 1, CFG_64x64 = 2, CFG_128x64 = 3, CFG_128x32 = 4, CFG_256x64 = 5, CFG_COUNT = 6 };

struct ConvCfgInfo { int BM, BN; };
inline ConvCfgInfo conv_cfg_info(int cfg) {
  switch (cfg) {
    case CFG_128x128: return {128, 128};
    case CFG_64x128: return {64, 128};
    case CFG_64x64: return {64, 64};
    case CFG_128x32: return {128, 32};
    case CFG_256x64: return {256, 64};   // 7x7 layers at batches of >= 4 images: twice the pixels per workgroup (one fill + epilogue per 98 K steps)
    default: return {128, 64};
  }
}

// prec: 0 = fp16 (MFMA f16, fp32 accumulate), 1 = fp32 (exact-f32 MFMA).  rowb: 64 or 128.
// Returns hipSuccess or the launch error.
hipError_t launch_conv(int prec, int cfg, int ks, int rowb, const ConvParams& P, int nprob, int N,
                       hipStream_t stream);

// LDS-DMA ring variant for k in {3,7}: chb = channel bytes per step (128, or 256 with the 64x64
// tile); weights packed with the matching 16-byte-chunk swizzle (see conv_ring.hip).
hipError_t launch_conv_ring(int prec, int cfg, int ks, int chb, const ConvParams& P, int nprob, int N,
                            hipStream_t stream);
// Two chained 1x1 convolutions in one launch (conv_pw2.hip): Y = W2 * act(W1 * X + b1) + b2, fp16 MFMA, Cin = 128 channels,
// middle layer a multiple of 128 channels, Cout <= 64.  P2 describes the SECOND convolution (destinations, bias, geometry;
// prob[].w = W2 packed [chunk][part][64][128]); the fields below the first one.
struct Pw2Params {
  ConvParams P2;
  const void* x_in[2];     // input tensor of the first convolution (element pointer of padded pixel 0)
  int x_cstride, x_lo_off; // channels per pixel; 0 or the offset of the input's lo block (split precision)
  const void* w1[2];       // W1 packed [chunk][part (hi, lo)][128][128]
  const float* b1[2];
  ConvDst mid[2];          // the middle layer's own blob tensor (base may be null)
  int c1_chunks;           // middle channels / 128
  int relu1;
  int split_w1, split_w2, h_lo;  // split precision: lo weights of either layer; lo part of the middle activations
};
hipError_t launch_conv_pw2(const Pw2Params& Q, int nprob, int nimg, hipStream_t stream);

inline int conv_ring_swz(int chb, int row) { return chb == 256 ? (row & 15) : ((row >> 1) & 7); }

// NCHW fp32 [N][3][H][W] -> level-0 tensor with 32 channels = 3x3 im2col of the image
// (channel (r*3+s)*3+c = in[c][y+r-1][x+s-1], zero outside; channels 27..31 zero).
hipError_t launch_pack_input(int prec, const float* in_nchw, void* out, Geom g, int Cp, hipStream_t stream);
// conv1_1 straight from the fp32 NCHW input (conv_first.hip): fp16 storage, 64 output channels, no split parts
struct FirstParams {
  const float* in;      // [N][3][H][W]
  Geom g;               // level-0 geometry (N = images in this launch)
  const uint4* wfrag;   // [tile 2][K-step 2][lane 64] A-operand fragments
  const float* bias;    // 64 floats in the kernel's channel order == reference order
  _Float16* out;        // halo'd NHWC destination, padded pixel 0
  int Cp;               // its channels per pixel (elements)
  int relu;
  unsigned long long* stamp;  // kernel residency slot (KStamp) or null
};
hipError_t launch_conv_first(const FirstParams& Q, hipStream_t stream);
int conv_first_channel_of_row(int i);
// 2x2 stride-2 MAX pooling between two halo'd NHWC tensors (pooling_layer.cpp:140-180).
// lo_i / lo_o: 0, or the channel offset of the lo block of a split-precision tensor — the pooled element keeps ITS lo
// part (the maximum of hi + lo, not two independent maxima).
// q_i / q_o: 0, or the element offset of the q block (fp8 compensation operands, ConvDst::q_off) — copied from the selected element.
hipError_t launch_maxpool(int prec, const void* in, Geom gi, int Cpi, void* out, Geom go, int Cpo, int C, int lo_i, int lo_o, int q_i, int q_o,
                          hipStream_t stream);
// halo'd NHWC (T) -> planar fp32 [N][C][H][W] (debug tap; channel map: out c reads in chmap[c]).
// lo_off != 0: the tensor carries a lo block, the exported value is hi + lo.
// q_off != 0 (and no lo block): the exported value is hi + fp8 lo part / 2^12.
hipError_t launch_export(int prec, const void* in, Geom g, int Cp, const int* chmap_dev, int C, int lo_off, int q_off, float* out,
                         hipStream_t stream);
// one wave waits `ticks` of the 100 MHz wall clock (at most 10 ms) and writes {start, end} to out2 (queue probe, measurement only)
hipError_t launch_queue_wait(long ticks, unsigned long long* out2, hipStream_t stream);

// ---------------------------------------------------------------------------------------
// Pre-processing on the device (row a1): see preproc.hip
// ---------------------------------------------------------------------------------------
// warp: BicubicTab_i of OpenCV's initInterTab2D, [fy][fx][k1*4+k2] 15-bit fixed-point weights (device pointer, 32 KiB)
struct AreaScale {                    // cv::resize(INTER_AREA) tables of one pyramid level (device pointers)
  int tw, th, identity;
  int fast_x, fast_y;                 // > 0: integer scale on both axes (resizeAreaFast_): block sums instead of the tables
  const int* xstart; const int* xsi; const float* xalpha;   // entries of dst column x: [xstart[x], xstart[x+1])
  const int* ystart; const int* ysi; const float* yalpha;
  // linear != 0: an axis of this level is ENLARGED — cv::resize(INTER_AREA) then runs its bilinear kernel with area-mode coefficients
  // (preprocess.cpp linear_area_tab): lx [tw][4] / ly [th][4] = {source index, its clipped neighbour, 11-bit weight, 11-bit weight}
  int linear;
  const int* lx; const int* ly;
};
hipError_t launch_warp(unsigned long long* stamp, const unsigned char* src, int sw, int sh, double inv, const short* tab2d, unsigned char* dst, int dw, int dh,
                       hipStream_t stream);
hipError_t launch_area_pad(unsigned long long* stamp, const unsigned char* disp, int dw, int dh, const AreaScale* scales, int nscales, float* out, int net_w, int net_h,
                           hipStream_t stream);

// A caller's u8 frame in device memory (rtp_frame_view, checked on the host before any launch): channel c (0 B, 1 G, 2 R) of pixel
// (x, y) is the byte at data + y * row + x * pix + off[c].
struct FrameView {
  unsigned char* data;
  int w, h;
  long row, pix;
  long off[3];
};
// How the import / export kernels address a view.  The specialised layouts move 4 pixels per thread with dword loads and stores
// (frame_layout picks them only where data, row and every plane start are 4-byte aligned and w % 4 == 0); GENERIC gathers bytes.
enum FrameLayout { LAYOUT_GENERIC = 0, LAYOUT_HWC3_BGR, LAYOUT_HWC3_RGB, LAYOUT_HWC4_BGR, LAYOUT_HWC4_RGB, LAYOUT_PLANAR };
// avail = bytes from data to the end of its allocation: a 4-channel layout also reads (and rewrites unchanged) each pixel's 4th byte
int frame_layout(const FrameView& v, size_t avail);
// view (v.w x v.h) -> packed u8 BGR HWC of the same size
hipError_t launch_frame_import(unsigned long long* stamp, const FrameView& v, int layout, unsigned char* dst, hipStream_t stream);
// packed u8 BGR HWC (v.w x v.h) -> the three named channels of the view
hipError_t launch_frame_export(unsigned long long* stamp, const unsigned char* src, const FrameView& v, int layout, hipStream_t stream);
// launch_warp reading the caller's view in place of a packed frame (same per-pixel arithmetic)
hipError_t launch_warp_view(unsigned long long* stamp, const FrameView& v, double inv, const short* tab2d, unsigned char* dst, int dw, int dh,
                            hipStream_t stream);

// A caller's (or the staged) 8-bit YUV frame in device memory (rtp_yuv_view, checked on the host before any launch): luma of pixel
// (x, y) is y[y * ys + x], its chroma samples u / v[(y >> sy) * uvs + (x >> sx) * uvp].  u == v == nullptr: luma only.
struct YuvView {
  const unsigned char* y;
  const unsigned char* u;
  const unsigned char* v;
  int w, h, sx, sy;
  long ys, uvs, uvp;
};
// How the conversion kernels (yuv_import.hip) address a frame.  The 4:2:0 layouts give each thread a 4 x 2 luma block: two dword Y
// loads, the block's two U and two V samples as one 16-bit load per plane (PLANAR) or one dword (NV12: u, v, u, v; NV21: v, u, v, u),
// two rows of three dword stores.  yuv_layout picks them only for 4:2:0 with w % 4 == 0, h % 2 == 0, a packed-BGR destination
// (pix 3, offsets 0 1 2) and every dword / 16-bit access aligned: y, ys, dst.data and dst.row to 4 bytes, the chroma pointers and uvs
// to 2 bytes (PLANAR) or to 4 (interleaved, v == u + 1 or u == v + 1).  GENERIC: one thread per pixel, byte loads and stores.
enum YuvLayout { YUV_GENERIC = 0, YUV_420_PLANAR, YUV_420_NV12, YUV_420_NV21 };
int yuv_layout(const YuvView& s, const FrameView& d);
inline FrameView packed_bgr_view(unsigned char* p, int w, int h) { return FrameView{p, w, h, 3L * w, 3, {0, 1, 2}}; }
// YUV (BT.601 limited range, the integer arithmetic of codecs.cpp rtp_convert_yuv) -> the three named channels of the view (s.w x s.h)
hipError_t launch_yuv_import(unsigned long long* stamp, const YuvView& s, const FrameView& d, int layout, hipStream_t stream);
// The other direction (yuv_export.hip): the three named channels of the view -> the planes of d (written; d.w x d.h = s.w x s.h), the
// integer arithmetic of codecs.cpp rtp_convert_bgr_to_yuv.  yuv_export_layout returns a YuvLayout value: the 4:2:0 layouts (one thread
// per 4 x 2 luma block: two rows of three dword loads, two dword luma stores, 16-bit or dword chroma stores) only for a packed-BGR
// source (pix 3, offsets 0 1 2, data and row 4-byte aligned), w % 4 == 0, h % 2 == 0 and planes aligned as yuv_layout asks of them;
// GENERIC: one thread per chroma cell, byte loads and stores.
int yuv_export_layout(const FrameView& s, const YuvView& d);
hipError_t launch_yuv_export(unsigned long long* stamp, const FrameView& s, const YuvView& d, int layout, hipStream_t stream);

// ---------------------------------------------------------------------------------------
// JPEG encoder (rtp_encode_jpeg_device, rtp_set_render_jpeg): jpeg_enc.hip, the bytes of codecs.cpp's rtp_encode_jpeg
// ---------------------------------------------------------------------------------------
struct JpegHuffTab { unsigned short code[256]; unsigned char size[256]; };
// per quality: the natural-order quantiser of luma (0) and chroma (1) as jcdctmgr.c divides by it: 8 Q / 2 and ceil(2^32 / 8 Q)
struct JpegQuant { unsigned recip[2][64]; unsigned short half[2][64]; };
// Device scratch of one w x h encoder, carved from ONE allocation of jpeg_bufs_bytes(w, h) bytes at base
struct JpegBufs {
  void* base = nullptr;
  int w = 0, h = 0;
  JpegHuffTab* huff = nullptr;   // [4]: DC luma, AC luma, DC chroma, AC chroma (filled once by the host)
  short* coef = nullptr;         // [blocks][64] quantised, zig-zag order
  unsigned* bits = nullptr;      // [blocks] AC code length incl. ZRL / EOB; after jpeg_bits_kernel the block's whole code length
  unsigned* mcubits = nullptr;   // [MCUs] bits of each MCU
  unsigned* off = nullptr;       // [blocks] bit offset in the entropy-coded segment
  int* dcdiff = nullptr;         // [blocks] DC difference to the component's predictor
  unsigned* words = nullptr;     // the bit stream, MSB first, whole 4 KiB chunks
  unsigned* counts = nullptr;    // [chunks] 0xFF bytes per chunk
  unsigned* meta = nullptr;      // [0] bits, [1] bytes before stuffing, [2] bytes after the header (stuffed data + EOI)
  unsigned char* data = nullptr; // stuffed data + EOI, padded to 16 bytes
};
// bytes of the scratch for w x h; with layout != null, its pointers are set from layout->base
size_t jpeg_bufs_bytes(int w, int h, JpegBufs* layout);
// the entropy-coded segment + EOI of the view -> dst (device-accessible, 16-byte aligned, room for the bytes rounded up to 16),
// its length -> *dst_len.  Seven launches on `stream`, all stamped into `stamp`.
hipError_t launch_jpeg_encode(unsigned long long* stamp, const FrameView& v, const JpegQuant& q, const JpegBufs& jb, unsigned char* dst,
                              unsigned* dst_len, hipStream_t stream);

// ---------------------------------------------------------------------------------------
// JPEG decoder (rtp_decode_jpeg_device, rtp_submit_frame_jpeg): jpeg_dec.hip, the pixels of codecs.cpp's decode_jpeg
// ---------------------------------------------------------------------------------------
struct JdTables { JdScan scan; JdHuff dc[3], ac[3]; };
// Byte offsets of one decode's buffers inside ONE device allocation of `total` bytes; [0, staged) is what the host stages (the same
// offsets inside its pinned buffer) and one copy brings over
struct JdLayout {
  size_t words = 0, tab = 0, segs = 0, subs = 0, staged = 0;
  size_t entry = 0, exit_ = 0, count = 0, excl = 0, gexit = 0, flags = 0, status = 0, coef = 0, dcsum = 0, planes = 0, total = 0;
  int ngroups = 0;
};
JdLayout jd_layout(long blocks, long plane_bytes, size_t nwords, size_t nsegs, size_t nsubs, int group);
// The entropy kernels' view of those buffers
struct JdDev {
  const JdTables* tab;
  const JdSeg* segs;
  const JdSub* subs;
  const uint32_t* words;
  int nsub, nwords, ngroups;
  JdState* entry;
  JdState* exit_;
  int* count;
  int* excl;
  JdState* gexit;     // [2][ngroups]: the exit state of every workgroup's last subsequence, by launch parity
  int* flags;         // [ngroups]: launch r changed something
  unsigned* status;   // 0xffffffff, or (scan-order block << 2 | JD_ERR_*) of the first failure
  unsigned* status_out;   // where the last kernel copies *status (pinned host memory as the device addresses it), or null
  short* coef;
  int* dcsum;
};
// Geometry, quantisers and colour model of a file for the reconstruction kernels
struct JdRecon {
  int W, H, ncomp, rgb, hmax, vmax, blocks;
  int h[3], v[3], bw[3], bh[3], dw[3], dh[3], coef_off[3];
  long plane_off[3];
  unsigned short qn[3][64];
};
hipError_t launch_jpeg_entropy(unsigned long long* stamp, const JdDev& d, int group, int mcus, int ncomp, long blocks, hipStream_t stream);
// coefficient blocks (component after component, natural order) -> planes (scratch) -> the three named channels of dv (W x H)
hipError_t launch_jpeg_reconstruct(unsigned long long* stamp, const JdRecon& g, const short* coef, unsigned char* planes, const FrameView& dv, hipStream_t stream);

// ---------------------------------------------------------------------------------------
// Renderer (row 8f-3): render.hip
// ---------------------------------------------------------------------------------------
struct RenderParams {
  const unsigned char* src;  // display image, u8 BGR HWC (device)
  unsigned char* dst;        // rendered image, same layout
  int w, h;
  const float* poses;        // joints [max_people][num_parts][3], display coordinates (device)
  const int* num_people;     // device
  float* tab;                // scratch, render_tab_floats(max_people)
  int model, googly, max_people;
};
hipError_t launch_render(const RenderParams& p, hipStream_t stream);
size_t render_tab_floats(int max_people);
// the --part_to_show views of render() (rtpose.cpp:270-299): one heat-map channel, all part maps, or PAF channels over the frame
struct RenderViewParams {
  const unsigned char* src;  // display image, u8 BGR HWC (device)
  unsigned char* dst;
  int w, h;
  const float* maps;         // net-resolution maps [C][net_h][net_w] (what the Nms layer reads), device
  int net_w, net_h;
  int model, part_to_show;   // part_to_show > 0 as FLAGS_part_to_show
};
hipError_t launch_render_view(const RenderViewParams& p, hipStream_t stream);

// ---------------------------------------------------------------------------------------
// Post-processing (bit-exact restatements of the reference's CUDA kernels / host loop).
// ---------------------------------------------------------------------------------------
struct ResizeParams {
  const float* src;  // [num][C][h][w]
  float* dst;        // [C][th][tw]
  int num, C, h, w, tw, th;
  float start_scale, scale_gap;
};
hipError_t launch_resize(const ResizeParams& p, hipStream_t stream);

// Maps mode (maps_export.hip, rtp_set_maps_output): selected channels of a frame's maps, converted and written through a pitched view.
//   grid 0 (RTP_MAPS_GRID_NET):    plane k = channel chan[k] of the resized map (r.th x r.tw), the arithmetic of resize_kernel bit for bit
//   grid 1 (RTP_MAPS_GRID_LOWRES): plane n * nch + k = channel chan[k] of scale n of r.src (r.h x r.w), as it stands
// Element (x, y) of plane z is at dst + z * channel_stride + y * row_stride + x * (1 u8 | 2 f16 | 4 f32) bytes; pitch padding is never
// written.  format 2 (RTP_MAPS_U8) quantises channels <= num_parts as rintf(clamp(v * 255, 0, 255)) and the PAF channels behind
// them as rintf(clamp((v + 1) * 127.5, 0, 255)), NaN -> 0 (rtp_maps_quantize_u8); format 1 rounds to binary16, nearest even.
// wide = 1: groups of 4 consecutive outputs of a row leave as one 4 / 8 / 16-byte store (NET), typed element stores (LOWRES);
// maps_export_wide says where that is allowed.  wide = 0: every element leaves byte by byte (any address, any pitch).
#define RTP_MAPS_MAX_CHANNELS 70   // RTP_MAX_NUM_PARTS
struct MapsParams {
  ResizeParams r;            // r.src = the frame's low-res maps, r.dst unused
  unsigned char* dst;
  long channel_stride, row_stride;
  int grid, format, nch, num_parts, wide;
  unsigned short chan[RTP_MAPS_MAX_CHANNELS];
  unsigned long long* stamp;  // kernel residency slot (KStamp) or null
};
inline int maps_elem_bytes(int format) { return format == 2 ? 1 : format == 1 ? 2 : 4; }
// NET: data, both strides and the row's bytes are multiples of one 4-output group (4 u8 / 8 f16 / 16 f32 bytes) and width % 4 == 0;
// LOWRES: data and both strides are multiples of the element size
int maps_export_wide(int grid, int format, int width, const void* data, long channel_stride, long row_stride);
hipError_t launch_maps_export(const MapsParams& p, hipStream_t stream);

// Crops mode (crops.hip, rtp_set_crops_output): one box per person from the joints connect_assemble_kernel left in device memory, and
// the display image resampled into fixed-size slots; boxes and pixels are rtp_crop_people's bit for bit (include/rtpose_mi355x.h
// spells out the arithmetic).  One launch per frame, grid (tiles of one crop, max_crops); *num_people is read on the device
// (negative = connect's error code = 0 people) and the workgroups of slots >= min(*num_people, max_crops) leave at once.
//   src == nullptr: boxes only (a frame without a display image), a grid of (1, max_crops)
//   boxes == nullptr: pixels only (rtp_peek_crops_device runs the kernel again into a caller's memory)
// Crop k starts at dst + k * crop_stride.  One pixel per thread.  wide = 1: a workgroup's 256 pixels are gathered in LDS and leave as
// 16-byte stores; crops_wide says where that is allowed.  wide = 0: three byte stores per thread (any address and stride).
#define RTP_CROPS_MAX_PARTS 70   // RTP_MAX_NUM_PARTS
struct CropsParams {
  const unsigned char* src;  // display image, u8 BGR HWC (device)
  int w, h;
  const float* joints;       // [max_people][num_parts][3]
  const int* num_people;
  float* boxes;              // [max_crops][6] records
  unsigned char* dst;
  long crop_stride;
  int num_parts, nlist, min_parts, crop_w, crop_h, max_crops, layout, wide;
  float min_score, margin;
  unsigned char list[RTP_CROPS_MAX_PARTS];
};
// data and crop_stride multiples of 16, crop_w a multiple of 16 (then crop_w * 3 and every plane are too)
int crops_wide(int crop_w, const void* data, long crop_stride);
hipError_t launch_crops(const CropsParams& p, hipStream_t stream);

// Tracking mode (track.hip, rtp_set_tracking): the frame's people, read in device memory behind the connect kernels, are associated
// with the engine's track table; the table is updated and one record {id, slot, hits, cost bits} per person is written.  Integers
// and float bits are rtp_track_update's (include/rtpose_mi355x.h spells out the arithmetic).  ONE workgroup per launch; launches on
// one table must be ordered by the caller (the engine chains them with events).  *num_people is read on the device (negative =
// connect's error code = 0 people).  TrackTable is rtp_track_state's layout (engine_track.cpp asserts it).
#define RTP_TRACK_SLOTS 128      // RTP_MAX_TRACKS
#define RTP_TRACK_MAX_PARTS 70   // RTP_MAX_NUM_PARTS
#define RTP_TRACK_MAX_PEOPLE 96  // RTP_MAX_PEOPLE
struct TrackTable {
  unsigned struct_size;
  int num_parts;
  unsigned next_id, frames;
  int id[RTP_TRACK_SLOTS], hits[RTP_TRACK_SLOTS], misses[RTP_TRACK_SLOTS];
  float joints[RTP_TRACK_SLOTS][RTP_TRACK_MAX_PARTS][3];
};
struct TrackParams {
  const float* joints;       // [max_people][num_parts][3]
  const int* num_people;
  TrackTable* table;
  int* recs;                 // [RTP_TRACK_MAX_PEOPLE][4] records (the first min(max(*num_people, 0), 96) are written)
  int num_parts, min_parts, min_common, max_misses;
  float min_score, max_cost;
  int variant;               // RTP_TRACK_* below: the form of the assignment and the workgroup's size (same records and table in all)
};
// The assignment, deterministic on (cost bits, slot, person) keys in both forms:
//   ARGMIN  a workgroup-wide argmin over the keys per round, the winner's row and column struck out: two barriers per matched person
//   SORT    the candidates' indices compacted and sorted once in LDS (bitonic, on the keys), then ONE thread walks the list
// each with a workgroup of 256 or 1024 threads.  profiles/r13_track.txt has all four measured; RTP_TRACK_DEFAULT is the fastest.
enum { RTP_TRACK_ARGMIN_256 = 0, RTP_TRACK_ARGMIN_1024 = 1, RTP_TRACK_SORT_256 = 2, RTP_TRACK_SORT_1024 = 3, RTP_TRACK_VARIANTS = 4 };
#define RTP_TRACK_DEFAULT RTP_TRACK_SORT_1024
hipError_t launch_track(const TrackParams& p, hipStream_t stream);

// Appearance-aided tracking (appearance.hip, track.hip; rtp_set_track_appearance).  Integers and float bits are
// rtp_appearance_describe's and rtp_track_update_appearance's (include/rtpose_mi355x.h spells out the arithmetic).
// appear_describe: one workgroup of 256 threads per person slot, grid RTP_TRACK_MAX_PEOPLE; *num_people is read on the device (negative
// = 0 people) and the workgroups of slots >= min(*num_people, 96) leave at once.  Wave 0 derives the slot's box (crops.hip's way), every
// thread takes 4 of the 1024 samples into 128 LDS counters, and the 128 uint16 leave as 16 stores of 16 bytes, with the valid byte.
// src == nullptr (a frame without a display image): valid = 0 and zeros for every person.  Stateless.
#define RTP_APPEAR_BINS 128      // RTP_APPEARANCE_BINS
#define RTP_APPEAR_GRID 32       // RTP_APPEARANCE_GRID
struct AppearDescribeParams {
  const unsigned char* src;  // display image, u8 BGR HWC (device), or nullptr
  int w, h;
  const float* joints;       // [max_people][num_parts][3]
  const int* num_people;
  unsigned short* bins;      // [RTP_TRACK_MAX_PEOPLE][RTP_APPEAR_BINS], 16-byte aligned
  unsigned char* valid;      // [RTP_TRACK_MAX_PEOPLE]
  int num_parts, nlist, min_parts;
  float min_score, margin;
  unsigned char list[RTP_TRACK_MAX_PARTS];
};
hipError_t launch_appear_describe(const AppearDescribeParams& p, hipStream_t stream);
// The appearance form of the track kernel: the same kernel with THE COST in phase B (the 128-bin L1 distance of a pair that passed the
// motion gate; table and descriptors are read through L2 with 16-byte loads) and THE TABLE UPDATE in phase F.  All four forms
// (p.variant); the instantiations launch_track launches are the code they were.  AppearTable is rtp_appearance_state's layout
// (engine_appearance.cpp asserts it).
struct AppearTable {
  unsigned struct_size;
  int reserved[3];
  int owner[RTP_TRACK_SLOTS];
  unsigned short desc[RTP_TRACK_SLOTS][RTP_APPEAR_BINS];
};
struct TrackAppearParams {
  const unsigned short* bins;   // the frame's descriptors (appear_describe's), 16-byte aligned
  const unsigned char* valid;
  AppearTable* table;           // 16-byte aligned
  float weight, max_dist, unknown;
  int rate;
};
hipError_t launch_track_appearance(const TrackParams& p, const TrackAppearParams& a, hipStream_t stream);

// Smoothing mode (smooth.hip, rtp_set_smoothing): the frame's people, read in device memory behind the track kernel with their
// records, go through a per-(track slot, part) One-Euro filter; the filter table is updated and joints_s, vel and flags are written.
// Float bits and bytes are rtp_smooth_update's (include/rtpose_mi355x.h spells out the arithmetic).  ONE workgroup per launch that
// loops over the n * P <= 6720 independent (person, part) items; the one shared value is the table's `frames`, which every thread
// reads before a barrier and one thread writes behind it.  Launches on one table must be ordered by the caller (the engine chains
// them with events).  SmoothTable is rtp_smooth_state's layout (engine_smooth.cpp asserts it).
struct SmoothCell {
  int owner;
  unsigned last;
  float pos[2], vel[2];
  float score;
};
struct SmoothTable {
  unsigned struct_size;
  int num_parts;
  unsigned frames;
  SmoothCell cell[RTP_TRACK_SLOTS][RTP_TRACK_MAX_PARTS];
};
struct SmoothParams {
  const float* joints;       // [max_people][num_parts][3]
  const int* num_people;
  const int* recs;           // [RTP_TRACK_MAX_PEOPLE][4] the frame's track records
  SmoothTable* table;
  float* joints_s;           // [RTP_TRACK_MAX_PEOPLE][num_parts][3]   (the first n people of each are written)
  float* vel;                // [RTP_TRACK_MAX_PEOPLE][num_parts][2]
  unsigned char* flags;      // [RTP_TRACK_MAX_PEOPLE][num_parts]
  int num_parts, max_hold;
  float min_score, min_cutoff, beta, d_cutoff;
  int variant;               // RTP_SMOOTH_* below: the workgroup's size (same outputs and table in both)
};
// Both sizes are built and measured (profiles/r14_smooth.txt, tools/bench_smooth.py): a launch's period for 1 / 8 / 96 tracked people
// is 2.1 / 2.3 / 7.2 us with 256 threads and 2.2 / 2.3 / 3.8 us with 1024.  1024 is the default: twice as fast on a full frame, within
// 0.1 us on a small one.
enum { RTP_SMOOTH_256 = 0, RTP_SMOOTH_1024 = 1, RTP_SMOOTH_VARIANTS = 2 };
#define RTP_SMOOTH_DEFAULT RTP_SMOOTH_1024
hipError_t launch_smooth(const SmoothParams& p, hipStream_t stream);

// Overlay mode (overlay.hip, rtp_set_track_overlay): two kernels.  Integers and bytes are rtp_overlay_update's and rtp_overlay_draw's
// (include/rtpose_mi355x.h spells out both).
// overlay_update: ONE workgroup per launch, behind the frame's track (and smooth) kernel.  The frame's people, read in device memory
// with their records, advance the trail table, one ring per track slot, and the frame's draw list is written: a prefix sum over the
// people's item counts gives every person its place, so the list is in person order.  Launches on one table must be ordered by the
// caller (the engine chains them with events).  TrailTable is rtp_trail_state's layout (engine_overlay.cpp asserts it).
#define RTP_OVL_TRAIL_MAX 32                                          // RTP_TRAIL_MAX
#define RTP_OVL_ITEM_INTS 9                                           // RTP_OVERLAY_ITEM_INTS
#define RTP_OVL_MAX_ITEMS (RTP_TRACK_MAX_PEOPLE * (RTP_OVL_TRAIL_MAX + 1))   // RTP_OVERLAY_MAX_ITEMS
struct TrailSlot {
  int owner, count, head;
  int pts[RTP_OVL_TRAIL_MAX][2];
};
struct TrailTable {
  unsigned struct_size;
  int num_parts;
  unsigned frames;
  TrailSlot slot[RTP_TRACK_SLOTS];
};
struct OverlayUpdateParams {
  const float* joints;       // [max_people][num_parts][3]
  const int* num_people;
  const int* recs;           // [RTP_TRACK_MAX_PEOPLE][4] the frame's track records
  TrailTable* table;
  int* items;                // [RTP_OVL_MAX_ITEMS][RTP_OVL_ITEM_INTS]   (the first *num_items are written)
  int* num_items;
  int num_parts;
  unsigned what;
  float min_score;
  int box_margin, line_width, label_scale, trail_len, trail_radius, alpha;
  int palette[16];           // RTP_OVERLAY_PALETTE
};
hipError_t launch_overlay_update(const OverlayUpdateParams& p, hipStream_t stream);
// overlay_draw: the draw list in place into a BGR image, one workgroup of 256 threads per tile of RTP_OVL_TILE_W x RTP_OVL_TILE_H
// pixels (two rows per thread).  The workgroup walks the list 256 items at a time: every thread tests one item's bounding box against
// the tile, a wave ballot and a prefix count over the four waves compact the hits IN ITEM ORDER into an LDS list, and whenever the
// next 256 candidates might not fit any more (and at the end) every thread blends its pixels through the list in order.  A tile that
// no item touches loads and stores no pixel.  Reads only *num_items, the items and the image: no table, so it needs no ordering
// against other frames.
#define RTP_OVL_TILE_W 32
#define RTP_OVL_TILE_H 16
struct OverlayDrawParams {
  const int* items;
  const int* num_items;      // clamped to 0 .. RTP_OVL_MAX_ITEMS
  unsigned char* image;      // BGR, in place
  int w, h;
  long stride;
  unsigned char font[10][7]; // RTP_OVERLAY_FONT
};
hipError_t launch_overlay_draw(const OverlayDrawParams& p, hipStream_t stream);

// Redaction mode (redact.hip, rtp_set_redaction): two kernels.  Integers and bytes are rtp_redact_regions' and rtp_redact_apply's
// (include/rtpose_mi355x.h spells out both).
// redact_regions: ONE workgroup per launch, one thread per person.  The frame's people, read in device memory, give one record
// {cx, cy, rx, ry, count, valid} each; behind the RTP_TRACK_MAX_PEOPLE records' room the launch writes n.  No table: no ordering
// against other frames.
#define RTP_RDC_REGION_INTS 6      // RTP_REDACT_REGION_INTS
#define RTP_RDC_MAX_RADIUS 4096    // RTP_REDACT_MAX_RADIUS
#define RTP_RDC_TILE 32            // both sides: a tile holds whole mosaic cells for every allowed cell
#define RTP_RDC_MAX_BLUR 16        // the largest blur radius: the halo of a tile
enum { RTP_RDC_MOSAIC = 0, RTP_RDC_BLUR = 1, RTP_RDC_FILL = 2 };   // RTP_REDACT_*
struct RedactRegionsParams {
  const float* joints;       // [max_people][num_parts][3]
  const int* num_people;
  int* regions;              // [RTP_TRACK_MAX_PEOPLE][RTP_RDC_REGION_INTS]   (the first n are written)
  int* num_regions;          // n = clamp(*num_people, 0, RTP_TRACK_MAX_PEOPLE)
  int num_parts, nlist, min_parts;
  float min_score;
  int scale_q8, aspect_q8, pad, min_radius;
  unsigned char list[RTP_TRACK_MAX_PARTS];
};
hipError_t launch_redact_regions(const RedactRegionsParams& p, hipStream_t stream);
// redact_apply: one workgroup of 256 threads per tile of RTP_RDC_TILE x RTP_RDC_TILE pixels, four pixels of one row per thread.  The
// workgroup culls the valid regions against its tile into LDS; a tile that no region touches reads nothing else and stores nothing.
// Every covered pixel's value is computed from `src` and stored to `dst` at the same position.  FILL and MOSAIC run with
// dst == src (a mosaic cell is read by exactly one workgroup, before a barrier in front of its first store).  BLUR reads a halo that
// neighbouring workgroups write, so it takes two launches: pass 0 with dst = a scratch image, pass 1 (copy = 1) copies the covered
// pixels from the scratch image back.  launch_redact_apply enqueues what the effect needs.
struct RedactApplyParams {
  const int* regions;
  const int* num_regions;    // clamped to 0 .. RTP_TRACK_MAX_PEOPLE
  unsigned char* image;      // BGR, redacted in place
  unsigned char* scratch;    // BLUR only: h rows of `stride` bytes, never the image
  int w, h;
  long stride;
  int effect, ellipse, cell, radius;
  unsigned colour;
};
hipError_t launch_redact_apply(const RedactApplyParams& p, hipStream_t stream);

struct NmsParams {
  const float* src;  // resized map [src_planes][H][W]
  float* peaks;      // [num_parts][max_peaks+1][3]  (in/out)
  int* strip_count;  // [num_parts][nstrips]
  int* strip_list;   // [num_parts][nstrips][max_peaks]  flat pixel index of the first max_peaks maxima of the strip
  int src_planes, H, W, num_parts, max_peaks, nstrips, strip_rows;
  float threshold;
  unsigned long long* probe;  // diagnostics (RTP_NMS_PROBE): wall-clock stamps of the phases of one strip workgroup, [0] = count
  unsigned long long* stamp;  // kernel residency slots (KStamp) or null: [0,1] strip kernel, [2,3] write kernel
  int* clear_flag;            // production chain: the connect kernels' people counter / error flag, reset here (the write kernel runs right in
                              // front of them on the same stream) instead of by a 4-byte fill launch of its own between the two
};
hipError_t launch_nms(const NmsParams& p, hipStream_t stream);
// Production path: the same peaks WITHOUT materialising the resized map — each strip workgroup
// evaluates ImResize for its rows (+1 halo row) in LDS, the centroid windows are evaluated on demand.
// `p.src` is ignored; `r.dst` is ignored.
hipError_t launch_nms_fused(const NmsParams& p, const ResizeParams& r, hipStream_t stream);

struct ConnectParams {
  unsigned long long* stamp;  // kernel residency slots (KStamp) or null: [0,1] pairs, [2,3] match, [4,5] assemble
  int counter_cleared;  // 1: *num_people was reset by the NMS write kernel in front of this chain (NmsParams::clear_flag)
  int* tickets;         // [num_limbs + 1] zeros (device): non-null = the production chain runs as ONE launch (connect_chain_kernel): per-limb tickets of
                        // the pair workgroups + one of the limbs; the kernel leaves them zero again
  const float* heat;   // resized map [C][net_h][net_w]
  const float* peaks;  // [num_parts][max_peaks+1][3]
  float* joints;       // [max_people][num_parts][3]
  int* num_people;     // [1]  (<0: error code)
  // scratch
  float* cand_score;   // [num_limbs][max_peaks*max_peaks]
  int* cand_ij;        // [num_limbs][max_peaks*max_peaks]  (i<<16|j), raster (i,j) order, compacted
  int* cand_count;     // [num_limbs]
  int* cand_blk;       // [num_limbs][ceil(max_peaks^2 / 256)] survivors per block of 256 pairs
  int* conn;           // [num_limbs][max_peaks][2]  (indexA, indexB) flat peak-score indices
  float* conn_score;   // [num_limbs][max_peaks]
  int* conn_count;     // [num_limbs]
  int* subset_idx;     // [max_rows][num_parts]
  double* subset_score;  // [max_rows]
  int* subset_cnt;     // [max_rows]
  int max_rows;
  int assemble_preload;  // set by launch_connect: the assembly kernel copies its inputs to LDS first
  int pairs_full;        // experiments (RTP_PAIRS_FULL=1): the pair kernel evaluates all 10 samples of every pair (round 5's behaviour; same results)
  int diag_stages;       // diagnostics (RTP_DIAG_SKIP_POST): 0 = all kernels, 1 = pairs only, 2 = pairs + match, 3 = all
  int model;           // 0 COCO_18, 1 MPI_15
  int num_parts, num_limbs, max_peaks;
  int net_w, net_h, disp_w, disp_h;
  float inter_threshold;
  int inter_min_above;
  int min_subset_cnt;
  float min_subset_score;
  int max_people;
};
hipError_t launch_connect(const ConnectParams& p, hipStream_t stream);
// Production path: PAF samples are evaluated from the low-res maps on demand (`p.heat` ignored).
hipError_t launch_connect_fused(const ConnectParams& p, const ResizeParams& r, hipStream_t stream);

}  // namespace rtp

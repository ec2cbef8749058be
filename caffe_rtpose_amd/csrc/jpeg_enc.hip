// jpeg_enc.hip — baseline JPEG encoding of a u8 frame view on the GPU, byte for byte the file codecs.cpp encode_jpeg_impl writes
// (libjpeg's islow path: jccolor integer YCbCr, 4:2:0 with h2v2 bias 1,2, jfdctint islow, round-half-away quantisation through the
// exact reciprocal, the standard Huffman tables, no restart markers, last byte padded with 1-bits).  All arithmetic is integer.
//
//   1. transform  one thread per 8x8 block (Y blocks first, then Cb/Cr): samples through the view, FDCT, quantise; the zig-zag
//                 coefficients -> coef, the AC code length (incl. ZRL/EOB) -> bits.  Dummy edge blocks: zeros.
//   2. bits       one thread per MCU: the dummy blocks' DC (the previous block's, always inside the MCU), every DC difference and
//                 block code length, the MCU's total.
//   3. scan       one workgroup: an exclusive scan of the MCU totals -> each block's bit offset; zeroes the words a block shares.
//   4. emit       one thread per block: its code words at its bit offset into 32-bit words (MSB first); words wholly inside the block
//                 are stored, the two it may share are atomicOr'ed (order-free, so deterministic).
//   5. count      per 4 KiB chunk of the bit stream: the number of 0xFF bytes.
//   6. scatter    per chunk: its output position (the sum of earlier chunks' counts), the bytes with a 0x00 after each 0xFF, and
//                 after the last byte the EOI marker; meta[2] = the bytes after the header.
//   7. copy       the data (16 B stores) to the destination, which may be pinned host memory, and its length.
// The header is written by the host (rtp_internal_jpeg_setup).  Vector memory operations only.
#include <algorithm>

#include "kernels.h"

namespace rtp {
namespace {

constexpr int kZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr int kChunkBytes = 4096;  // count / scatter: 256 threads x 16 bytes
constexpr int kScanThreads = 1024;

__device__ __forceinline__ int bit_category(int v) { const unsigned a = (unsigned)(v < 0 ? -v : v); return a ? 32 - __clz(a) : 0; }

// jfdctint.c jpeg_fdct_islow on level-shifted samples (codecs.cpp fdct_islow), int32, fully unrolled: d stays in registers
__device__ __forceinline__ void fdct_islow(int (&d)[64]) {
  constexpr int CONST_BITS = 13, PASS1_BITS = 2;
  constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
                F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
                F_2_562915447 = 20995, F_3_072711026 = 25172;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int step = pass ? 8 : 1, next = pass ? 1 : 8;
    const int sh = pass ? CONST_BITS + PASS1_BITS : CONST_BITS - PASS1_BITS;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int b = i * next;
      const int tmp0 = d[b] + d[b + 7 * step], tmp7 = d[b] - d[b + 7 * step], tmp1 = d[b + step] + d[b + 6 * step], tmp6 = d[b + step] - d[b + 6 * step];
      const int tmp2 = d[b + 2 * step] + d[b + 5 * step], tmp5 = d[b + 2 * step] - d[b + 5 * step], tmp3 = d[b + 3 * step] + d[b + 4 * step],
                tmp4 = d[b + 3 * step] - d[b + 4 * step];
      const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
      const int z1e = (tmp12 + tmp13) * F_0_541196100;
      if (!pass) {
        d[b] = (tmp10 + tmp11) * (1 << PASS1_BITS);
        d[b + 4 * step] = (tmp10 - tmp11) * (1 << PASS1_BITS);
      } else {
        d[b] = (tmp10 + tmp11 + (1 << (PASS1_BITS - 1))) >> PASS1_BITS;
        d[b + 4 * step] = (tmp10 - tmp11 + (1 << (PASS1_BITS - 1))) >> PASS1_BITS;
      }
      d[b + 2 * step] = (z1e + tmp13 * F_0_765366865 + (1 << (sh - 1))) >> sh;
      d[b + 6 * step] = (z1e + tmp12 * (-F_1_847759065) + (1 << (sh - 1))) >> sh;
      int z1 = tmp4 + tmp7, z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
      const int z5 = (z3 + z4) * F_1_175875602;
      const int t4 = tmp4 * F_0_298631336, t5 = tmp5 * F_2_053119869, t6 = tmp6 * F_3_072711026, t7 = tmp7 * F_1_501321110;
      z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
      z3 += z5; z4 += z5;
      d[b + 7 * step] = (t4 + z1 + z3 + (1 << (sh - 1))) >> sh;
      d[b + 5 * step] = (t5 + z2 + z4 + (1 << (sh - 1))) >> sh;
      d[b + 3 * step] = (t6 + z2 + z3 + (1 << (sh - 1))) >> sh;
      d[b + step] = (t7 + z1 + z4 + (1 << (sh - 1))) >> sh;
    }
  }
}

struct Geo {  // codecs.cpp encode_jpeg_impl's plane geometry
  int W, H, mcux, nmcu, yw_blocks, yh_blocks;
};
__host__ __device__ inline Geo make_geo(int W, int H) {
  Geo g;
  g.W = W; g.H = H;
  g.mcux = (W + 15) / 16;
  g.nmcu = g.mcux * ((H + 15) / 16);
  g.yw_blocks = (W + 7) / 8; g.yh_blocks = (H + 7) / 8;
  return g;
}
// block b (0..3 luma in raster order, 4 Cb, 5 Cr) of MCU m is real (Cb, Cr and luma 0 always are: the chroma planes' width in blocks
// is the MCU count)
__device__ __forceinline__ bool block_real(const Geo& g, int m, int b) {
  if (b == 0 || b >= 4) return true;
  const int my = m / g.mcux, mx = m - my * g.mcux;
  return mx * 2 + (b & 1) < g.yw_blocks && my * 2 + (b >> 1) < g.yh_blocks;
}

__device__ __forceinline__ void load_px(const FrameView& v, int x, int y, int* r, int* gg, int* b) {
  const unsigned char* p = v.data + (long)y * v.row + (long)x * v.pix;
  *b = p[v.off[0]]; *gg = p[v.off[1]]; *r = p[v.off[2]];
}

__global__ __launch_bounds__(256) void jpeg_transform_kernel(unsigned long long* stamp, FrameView v, JpegQuant q, JpegBufs jb) {
  const KStamp kstamp_(stamp);
  const Geo g = make_geo(v.w, v.h);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 6 * g.nmcu) return;
  int m, b;
  if (t < 4 * g.nmcu) { m = t >> 2; b = t & 3; }                      // luma threads first: waves stay on one path
  else { const int u = t - 4 * g.nmcu; m = u >> 1; b = 4 + (u & 1); }
  const int blk = m * 6 + b;
  const int my = m / g.mcux, mx = m - my * g.mcux;
  const int tq = b >= 4;
  const JpegHuffTab* hac = jb.huff + (tq ? 3 : 1);
  int d[64];
  if (!block_real(g, m, b)) {  // dummy edge block: zero coefficients; its DC is resolved by the scan
    uint4* o = reinterpret_cast<uint4*>(jb.coef + (size_t)blk * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = make_uint4(0, 0, 0, 0);
    jb.bits[blk] = hac->size[0x00];
    return;
  }
  if (b < 4) {
    // luma of real pixels, the right edge and the rows below the image replicated (expand_right_edge / bottom rows)
    const int x0 = mx * 16 + (b & 1) * 8, y0 = my * 16 + (b >> 1) * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int y = min(y0 + r, g.H - 1);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        int R, G, B;
        load_px(v, min(x0 + c, g.W - 1), y, &R, &G, &B);
        d[r * 8 + c] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
      }
    }
  } else {
    // h2v2_downsample of Cb or Cr: 2x2 sums, bias 1,2 along the row; chroma rows past ceil(H/2) repeat the last one
    const int crow = (g.H + 1) / 2;
    const int kr = b == 4 ? -11059 : 32768, kg = b == 4 ? -21709 : -27439, kb = b == 4 ? 32768 : -5329;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int sy = min(my * 8 + r, crow - 1);
      const int ya = min(2 * sy, g.H - 1), yb = min(2 * sy + 1, g.H - 1);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int sx = mx * 8 + c;
        const int xa = min(2 * sx, g.W - 1), xb = min(2 * sx + 1, g.W - 1);
        int s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          int R, G, B;
          load_px(v, (k & 1) ? xb : xa, (k >> 1) ? yb : ya, &R, &G, &B);
          s += (kr * R + kg * G + kb * B + (128 << 16) + 32767) >> 16;
        }
        d[r * 8 + c] = ((s + ((c & 1) ? 2 : 1)) >> 2) - 128;
      }
    }
  }
  fdct_islow(d);
  // jcdctmgr.c quantisation: round half away from zero, the division through the exact reciprocal (|t| < 2^17, 8*Q < 2^11)
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int x = d[i];
    const unsigned a = (unsigned)(x < 0 ? -x : x) + q.half[tq][i];
    const int mq = (int)__umulhi(a, q.recip[tq][i]);
    d[i] = x < 0 ? -mq : mq;
  }
  // zig-zag int16 coefficients, 8 x 16 B stores; AC code length exactly as the emitter will write it
  unsigned pk[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) pk[k] = (unsigned)(d[kZZ[2 * k]] & 0xFFFF) | ((unsigned)d[kZZ[2 * k + 1]] << 16);
  uint4* o = reinterpret_cast<uint4*>(jb.coef + (size_t)blk * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = make_uint4(pk[4 * i], pk[4 * i + 1], pk[4 * i + 2], pk[4 * i + 3]);
  unsigned bits = 0;
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int c = d[kZZ[k]];
    if (c == 0) { ++run; continue; }
    while (run > 15) { bits += hac->size[0xF0]; run -= 16; }
    const int s = bit_category(c);
    bits += hac->size[(run << 4) | s] + s;
    run = 0;
  }
  if (run) bits += hac->size[0x00];
  jb.bits[blk] = bits;
}

__device__ __forceinline__ int blk_dc(const JpegBufs& jb, int blk) { return jb.coef[(size_t)blk * 64]; }

// the 6 DC values of MCU m after dummy resolution (a dummy luma block takes the DC of the block coded before it)
__device__ __forceinline__ void mcu_dc(const Geo& g, const JpegBufs& jb, int m, int (&dc)[6]) {
#pragma unroll
  for (int b = 0; b < 6; ++b) dc[b] = (b == 0 || b >= 4 || block_real(g, m, b)) ? blk_dc(jb, m * 6 + b) : dc[b - 1];
}

// per MCU, all MCUs in parallel: every block's DC difference (-> dcdiff) and whole code length (-> bits, in place of the AC length),
// the MCU's total (-> mcubits).  The predictors are the previous MCU's DC values, resolved the same way.
__global__ __launch_bounds__(256) void jpeg_bits_kernel(unsigned long long* stamp, int W, int H, JpegBufs jb) {
  const KStamp kstamp_(stamp);
  const Geo g = make_geo(W, H);
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= g.nmcu) return;
  int dc[6], pv[6] = {0, 0, 0, 0, 0, 0};
  mcu_dc(g, jb, m, dc);
  if (m > 0) mcu_dc(g, jb, m - 1, pv);
  const int pred[6] = {pv[3], dc[0], dc[1], dc[2], pv[4], pv[5]};
  unsigned tot = 0;
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const int diff = dc[b] - pred[b];
    const int s = bit_category(diff);
    const unsigned bits = jb.huff[b >= 4 ? 2 : 0].size[s] + s + jb.bits[m * 6 + b];
    jb.dcdiff[m * 6 + b] = diff;
    jb.bits[m * 6 + b] = bits;
    tot += bits;
  }
  jb.mcubits[m] = tot;
}

// one workgroup: exclusive scan of the MCU totals -> every block's bit offset; the first and last word of each block start at zero
__global__ __launch_bounds__(kScanThreads) void jpeg_scan_kernel(unsigned long long* stamp, int W, int H, JpegBufs jb) {
  const KStamp kstamp_(stamp);
  const Geo g = make_geo(W, H);
  __shared__ unsigned wsum[kScanThreads / 64];
  __shared__ unsigned carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < g.nmcu; base += kScanThreads) {
    const int m = base + tid;
    unsigned bits[6] = {0, 0, 0, 0, 0, 0};
    unsigned tot = 0;
    if (m < g.nmcu) {
      tot = jb.mcubits[m];
#pragma unroll
      for (int b = 0; b < 6; ++b) bits[b] = jb.bits[m * 6 + b];
    }
    // inclusive scan of tot over the workgroup: within each wave, then over the wave totals
    unsigned inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned y = __shfl_up(inc, o, 64);
      if (lane >= o) inc += y;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned before = carry_s;
    for (int w = 0; w < wv; ++w) before += wsum[w];
    unsigned off = before + inc - tot;
    if (m < g.nmcu) {
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        jb.off[m * 6 + b] = off;
        jb.words[off >> 5] = 0u;                         // the words this block may share with a neighbour start at zero
        jb.words[(off + bits[b] - 1) >> 5] = 0u;
        off += bits[b];
      }
    }
    __syncthreads();
    if (tid == kScanThreads - 1) carry_s = before + inc;
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned T = carry_s;
    jb.meta[0] = T;
    jb.meta[1] = (T + 7) >> 3;
  }
}

struct BitSink {
  unsigned* words;
  unsigned start, end;     // this block's bit range
  unsigned w;              // word the pending bits belong to
  unsigned long long acc;  // pending bits in the low n bits
  int n;
  __device__ __forceinline__ void word_out(unsigned x) {
    if (w * 32u >= start && w * 32u + 32u <= end) words[w] = x;
    else if (x) atomicOr(words + w, x);
    ++w;
  }
  __device__ __forceinline__ void put(unsigned code, int size) {  // size <= 27
    acc = (acc << size) | code;
    n += size;
    if (n >= 32) { n -= 32; word_out((unsigned)(acc >> n)); }
  }
  __device__ __forceinline__ void flush() {
    if (n > 0) word_out((unsigned)(acc << (32 - n)));
  }
};

__global__ __launch_bounds__(256) void jpeg_emit_kernel(unsigned long long* stamp, int W, int H, JpegBufs jb) {
  const KStamp kstamp_(stamp);
  const Geo g = make_geo(W, H);
  const int blk = blockIdx.x * blockDim.x + threadIdx.x;
  const int nblk = 6 * g.nmcu;
  if (blk >= nblk) return;
  const int hidx = (blk % 6) >= 4 ? 2 : 0;
  const JpegHuffTab* hdc = jb.huff + hidx;
  const JpegHuffTab* hac = jb.huff + hidx + 1;
  BitSink bs;
  bs.words = jb.words;
  bs.start = jb.off[blk];
  bs.end = blk + 1 < nblk ? jb.off[blk + 1] : jb.meta[0];
  bs.w = bs.start >> 5;
  bs.acc = 0;
  bs.n = (int)(bs.start & 31);  // zero bits of the preceding block(s) in the first word
  const int diff = jb.dcdiff[blk];
  int s = bit_category(diff);
  bs.put(((unsigned)hdc->code[s] << s) | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1)), hdc->size[s] + s);
  const uint4* cp = reinterpret_cast<const uint4*>(jb.coef + (size_t)blk * 64);
  unsigned pk[32];
#pragma unroll
  for (int i = 0; i < 8; ++i) { const uint4 x = cp[i]; pk[4 * i] = x.x; pk[4 * i + 1] = x.y; pk[4 * i + 2] = x.z; pk[4 * i + 3] = x.w; }
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int c = (int)(short)((k & 1) ? (pk[k >> 1] >> 16) : (pk[k >> 1] & 0xFFFF));
    if (c == 0) { ++run; continue; }
    while (run > 15) { bs.put(hac->code[0xF0], hac->size[0xF0]); run -= 16; }
    s = bit_category(c);
    const int sym = (run << 4) | s;
    bs.put(((unsigned)hac->code[sym] << s) | ((unsigned)(c < 0 ? c - 1 : c) & ((1u << s) - 1)), hac->size[sym] + s);
    run = 0;
  }
  if (run) bs.put(hac->code[0x00], hac->size[0x00]);
  bs.flush();
}

// 16 bytes of the bit stream from byte p (a multiple of 16), MSB-first; bytes at or past nb read as 0, the last byte padded with 1-bits
__device__ __forceinline__ void stream_bytes(const JpegBufs& jb, unsigned p, unsigned T, unsigned nb, unsigned char (&o)[16]) {
  const uint4 x = *reinterpret_cast<const uint4*>(jb.words + (p >> 2));
  const unsigned w4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const unsigned idx = p + i;
    unsigned char c = (unsigned char)(w4[i >> 2] >> (24 - 8 * (i & 3)));
    if (idx == nb - 1 && (T & 7)) c |= (unsigned char)(0xFFu >> (T & 7));
    o[i] = idx < nb ? c : 0;
  }
}

__global__ __launch_bounds__(256) void jpeg_count_kernel(unsigned long long* stamp, JpegBufs jb) {
  const KStamp kstamp_(stamp);
  const unsigned T = jb.meta[0], nb = jb.meta[1];
  const unsigned nchunks = (nb + kChunkBytes - 1) / kChunkBytes;
  __shared__ unsigned red[4];
  for (unsigned c = blockIdx.x; c < nchunks; c += gridDim.x) {
    unsigned char o[16];
    stream_bytes(jb, c * kChunkBytes + threadIdx.x * 16, T, nb, o);
    unsigned n = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) n += o[i] == 0xFF;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) jb.counts[c] = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void jpeg_scatter_kernel(unsigned long long* stamp, JpegBufs jb) {
  const KStamp kstamp_(stamp);
  const unsigned T = jb.meta[0], nb = jb.meta[1];
  const unsigned nchunks = (nb + kChunkBytes - 1) / kChunkBytes;
  __shared__ unsigned red[4], wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (unsigned c = blockIdx.x; c < nchunks; c += gridDim.x) {
    // the 0x00 bytes inserted before this chunk: the sum of the earlier chunks' counts
    unsigned pre = 0;
    for (unsigned i = tid; i < c; i += 256) pre += jb.counts[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) pre += __shfl_xor(pre, d, 64);
    if (lane == 0) red[wv] = pre;
    const unsigned p = c * kChunkBytes + tid * 16;
    unsigned char o[16];
    stream_bytes(jb, p, T, nb, o);
    unsigned n = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) n += o[i] == 0xFF;
    unsigned inc = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned y = __shfl_up(inc, d, 64);
      if (lane >= d) inc += y;
    }
    if (lane == 63) wtot[wv] = inc;
    __syncthreads();
    unsigned pos = red[0] + red[1] + red[2] + red[3] + p + inc - n;
    for (int w = 0; w < wv; ++w) pos += wtot[w];
    if (p < nb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (p + i < nb) {
          jb.data[pos++] = o[i];
          if (o[i] == 0xFF) jb.data[pos++] = 0;
        }
      }
      if (p + 16 >= nb) {  // this thread wrote the last byte: EOI behind it
        jb.data[pos] = 0xFF;
        jb.data[pos + 1] = 0xD9;
        jb.meta[2] = pos + 2;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void jpeg_copy_kernel(unsigned long long* stamp, JpegBufs jb, unsigned char* dst, unsigned* dst_len) {
  const KStamp kstamp_(stamp);
  const unsigned n = jb.meta[2];
  const unsigned n16 = (n + 15) >> 4;
  const uint4* s = reinterpret_cast<const uint4*>(jb.data);
  uint4* d = reinterpret_cast<uint4*>(dst);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += gridDim.x * blockDim.x) d[i] = s[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) *dst_len = n;
}

}  // namespace

size_t jpeg_bufs_bytes(int W, int H, JpegBufs* layout) {
  const Geo g = make_geo(W, H);
  const size_t nblk = (size_t)g.nmcu * 6;
  const size_t max_bits = nblk * kJpegMaxBlockBits;
  const size_t words = ((max_bits + 31) / 32 + kChunkBytes / 4 - 1) / (kChunkBytes / 4) * (kChunkBytes / 4);  // whole chunks
  const size_t chunks = words * 4 / kChunkBytes;
  const size_t data = ((max_bits + 7) / 8 * 2 + 2 + 15) / 16 * 16;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
  const size_t o_huff = take(sizeof(JpegHuffTab) * 4), o_coef = take(nblk * 64 * 2), o_ac = take(nblk * 4), o_mcu = take((size_t)g.nmcu * 4), o_off = take(nblk * 4),
               o_dc = take(nblk * 4), o_words = take(words * 4), o_counts = take(chunks * 4), o_meta = take(16), o_data = take(data);
  if (layout) {
    unsigned char* b = reinterpret_cast<unsigned char*>(layout->base);
    layout->huff = reinterpret_cast<JpegHuffTab*>(b + o_huff);
    layout->coef = reinterpret_cast<short*>(b + o_coef);
    layout->bits = reinterpret_cast<unsigned*>(b + o_ac);
    layout->mcubits = reinterpret_cast<unsigned*>(b + o_mcu);
    layout->off = reinterpret_cast<unsigned*>(b + o_off);
    layout->dcdiff = reinterpret_cast<int*>(b + o_dc);
    layout->words = reinterpret_cast<unsigned*>(b + o_words);
    layout->counts = reinterpret_cast<unsigned*>(b + o_counts);
    layout->meta = reinterpret_cast<unsigned*>(b + o_meta);
    layout->data = b + o_data;
    layout->w = W; layout->h = H;
  }
  return o;
}

hipError_t launch_jpeg_encode(unsigned long long* stamp, const FrameView& v, const JpegQuant& q, const JpegBufs& jb, unsigned char* dst,
                              unsigned* dst_len, hipStream_t stream) {
  if (v.w != jb.w || v.h != jb.h) return hipErrorInvalidValue;
  const Geo g = make_geo(v.w, v.h);
  const unsigned nblk = 6u * (unsigned)g.nmcu;
  const unsigned grid_blk = (nblk + 255) / 256;
  const size_t maxchunks = ((size_t)nblk * kJpegMaxBlockBits / 8 + kChunkBytes) / kChunkBytes;
  const unsigned grid_chunks = (unsigned)std::min<size_t>(maxchunks, 1024);
  hipLaunchKernelGGL(jpeg_transform_kernel, dim3(grid_blk), dim3(256), 0, stream, stamp, v, q, jb);
  hipLaunchKernelGGL(jpeg_bits_kernel, dim3((g.nmcu + 255) / 256), dim3(256), 0, stream, stamp, v.w, v.h, jb);
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, stamp, v.w, v.h, jb);
  hipLaunchKernelGGL(jpeg_emit_kernel, dim3(grid_blk), dim3(256), 0, stream, stamp, v.w, v.h, jb);
  hipLaunchKernelGGL(jpeg_count_kernel, dim3(grid_chunks), dim3(256), 0, stream, stamp, jb);
  hipLaunchKernelGGL(jpeg_scatter_kernel, dim3(grid_chunks), dim3(256), 0, stream, stamp, jb);
  hipLaunchKernelGGL(jpeg_copy_kernel, dim3(256), dim3(256), 0, stream, stamp, jb, dst, dst_len);
  return hipGetLastError();
}

}  // namespace rtp

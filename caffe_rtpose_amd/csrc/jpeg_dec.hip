// jpeg_dec.hip — JPEG files decoded on the GPU (rtp_decode_jpeg_device, rtp_submit_frame_jpeg): byte for byte the pixels codecs.cpp's
// decode_jpeg (libjpeg's default path) makes of the file.
//
// Entropy decoding (sequential Huffman files with one scan; jpeg_dec.h holds the per-symbol step, shared with the host):
//   jd_sync_kernel   self-synchronising parallel Huffman decode.  One thread per subsequence of S bits.  Round 0 decodes every
//                    subsequence from a guessed state and keeps its exit state; then exit_i = f_i(exit_{i-1}) is iterated inside the
//                    workgroup until nothing changes (at most T rounds).  Between workgroups states travel only from one LAUNCH to
//                    the next (gexit, double buffered by launch parity): launch r makes workgroup r exact, so `groups` launches
//                    reach the fixed point for any input; a launch behind one that changed nothing returns at once on flags[r-1].
//   jd_scan_kernel   blocks completed per subsequence -> blocks in front of every subsequence
//   jd_write_kernel  the final pass from the true entry states: coefficients, raw DC differences, the first failure in scan order
//   jd_dc_kernel     DC differences -> DC values: a prefix sum per component, restarted at every restart segment
// No workgroup waits for another one, every loop has a bound fixed before it starts, no read leaves the staged scan.
// Reconstruction (every file the host decoder accepts; coefficients from the kernels above or from the host's entropy decoder):
//   jd_idct_kernel   dequantise + jidctint.c jpeg_idct_islow in 64-bit integers as codecs.cpp computes it (coefficients of a corrupt or
//                    synthetic file are not bounded by the sample range, so no 32-bit variant is provably equal), & 1023 range limit
//   jd_color_kernel  jdsample.c fancy up-sampling (h2v1, h2v2, h1v2; replication for narrow planes and other ratios) evaluated at
//                    the output pixel, jdcolor.c YCbCr -> RGB, through the destination view
#include "kernels.h"

namespace rtp {

namespace {

__device__ __forceinline__ void jd_load_tables(JdTables* dst, const JdTables* src) {
  const unsigned* s = reinterpret_cast<const unsigned*>(src);
  unsigned* d = reinterpret_cast<unsigned*>(dst);
  for (unsigned i = threadIdx.x; i < sizeof(JdTables) / 4; i += blockDim.x) d[i] = s[i];
  __syncthreads();
}

__global__ __launch_bounds__(1024) void jd_sync_kernel(unsigned long long* stamp, JdDev d, int round, int T) {
  const KStamp kstamp_(stamp);
  if (round > 0 && d.flags[round - 1] == 0) return;   // the launch before changed nothing: the fixed point is reached
  __shared__ JdTables tab;
  __shared__ JdState s_exit[1024];
  __shared__ int s_changed;
  jd_load_tables(&tab, d.tab);
  const int t = threadIdx.x, i = blockIdx.x * T + t;
  const bool valid = t < T && i < d.nsub;
  const JdBits br = {d.words, d.nwords};
  JdSub sub = {0, 0, 0, 0};
  JdState entry = {0, 0, 0}, ex = {0, 0, 0}, guess = {0, 0, 0}, prev_group = {0, 0, 0};
  int cnt = 0, limit = 0;
  bool dirty = false, any = false;
  if (valid) {
    sub = d.subs[i];
    limit = d.segs[sub.seg].limit;
    guess.pos = sub.start;
    if (round == 0) {
      entry = guess;
      ex = jd_run_sub(br, sub, limit, tab.dc, tab.ac, tab.scan, entry, &cnt);
      dirty = true;
    } else {
      entry = d.entry[i]; ex = d.exit_[i]; cnt = d.count[i];
    }
    prev_group = entry;
    if (t == 0 && round > 0 && blockIdx.x > 0) prev_group = d.gexit[((round - 1) & 1) * d.ngroups + blockIdx.x - 1];
  }
  for (int it = 0; it < T; ++it) {
    if (valid) s_exit[t] = ex;
    if (t == 0) s_changed = 0;
    __syncthreads();
    bool ch = false;
    if (valid) {
      const JdState want = (sub.flags & JD_SUB_ANCHORED) ? guess : (t > 0 ? s_exit[t - 1] : prev_group);
      if (!jd_same(want, entry)) {
        entry = want;
        ex = jd_run_sub(br, sub, limit, tab.dc, tab.ac, tab.scan, entry, &cnt);
        ch = true;
      }
    }
    if (ch) { s_changed = 1; dirty = true; any = true; }
    __syncthreads();
    const int go = s_changed;
    __syncthreads();
    if (!go) break;
  }
  if (valid) {
    if (dirty) { d.entry[i] = entry; d.exit_[i] = ex; d.count[i] = cnt; }
    if (t == T - 1 || i == d.nsub - 1) d.gexit[(round & 1) * d.ngroups + blockIdx.x] = ex;
    if (any || (round == 0 && t == 0)) d.flags[round] = 1;   // round 0 has seen no other workgroup's state yet: round 1 always runs
  }
}

// excl[i] = blocks completed by subsequences 0 .. i-1 (one workgroup; ceil(nsub / 1024) iterations)
__global__ __launch_bounds__(1024) void jd_scan_kernel(unsigned long long* stamp, JdDev d) {
  const KStamp kstamp_(stamp);
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) carry_s = 0;
  __syncthreads();
  const int iters = (d.nsub + 1023) / 1024;
  for (int it = 0; it < iters; ++it) {
    const int i = it * 1024 + t;
    const int v = i < d.nsub ? d.count[i] : 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int before = carry_s;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (i < d.nsub) d.excl[i] = before + x - v;
    __syncthreads();
    if (t == 1023) carry_s = before + x;
    __syncthreads();
  }
  if (t == 0) d.excl[d.nsub] = carry_s;
}

__global__ __launch_bounds__(256) void jd_write_kernel(unsigned long long* stamp, JdDev d) {
  const KStamp kstamp_(stamp);
  __shared__ JdTables tab;
  jd_load_tables(&tab, d.tab);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.nsub) return;
  const JdSub sub = d.subs[i];
  const JdSeg seg = d.segs[sub.seg];
  const JdBits br = {d.words, d.nwords};
  const int base = d.excl[i] - d.excl[seg.first_sub];
  unsigned* status = d.status;
  jd_write_sub(br, sub, seg, tab.dc, tab.ac, tab.scan, d.entry[i], base, d.coef, [status](unsigned v) { atomicMin(status, v); });
}

// One workgroup per component: inclusive prefix sums of the DC differences in scan order (int32) into dcsum, then every block's
// DC value = its sum minus the sum in front of its restart segment, stored as int16.  Workgroup 0 also hands the status word to
// the host.
__global__ __launch_bounds__(1024) void jd_dc_kernel(unsigned long long* stamp, JdDev d, int mcus) {
  const KStamp kstamp_(stamp);
  __shared__ int wsum[16];
  __shared__ int carry_s;
  __shared__ JdScan sc;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, c = blockIdx.x;
  for (unsigned i = t; i < sizeof(JdScan) / 4; i += blockDim.x) reinterpret_cast<unsigned*>(&sc)[i] = reinterpret_cast<const unsigned*>(&d.tab->scan)[i];
  if (t == 0) carry_s = 0;
  __syncthreads();
  const int per_mcu = sc.h[c] * sc.v[c];
  const int total = mcus * per_mcu;
  const int per_seg = sc.restart_blocks ? (sc.restart_blocks / sc.nblk) * per_mcu : 0;
  int* P = d.dcsum + sc.coef_off[c];
  const auto block_of = [&](int j) {
    const int mcu = j / per_mcu, b = j - mcu * per_mcu;
    const int my = mcu / sc.mcux, mx = mcu - my * sc.mcux;
    const int by = b / sc.h[c], bx = b - by * sc.h[c];
    return (long)(sc.coef_off[c] + (my * sc.v[c] + by) * sc.bw[c] + mx * sc.h[c] + bx) * 64;
  };
  const int iters = (total + 1023) / 1024;
  for (int it = 0; it < iters; ++it) {
    const int j = it * 1024 + t;
    int x = j < total ? (int)d.coef[block_of(j)] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int before = carry_s;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (j < total) P[j] = before + x;
    __syncthreads();
    if (t == 1023) carry_s = before + x;
    __syncthreads();
  }
  __syncthreads();   // P was written by this workgroup alone
  for (int it = 0; it < iters; ++it) {
    const int j = it * 1024 + t;
    if (j >= total) break;
    const int s0 = per_seg ? (j / per_seg) * per_seg : 0;
    d.coef[block_of(j)] = (short)(P[j] - (s0 ? P[s0 - 1] : 0));
  }
  if (c == 0 && t == 0 && d.status_out) *d.status_out = *d.status;
}

__device__ __forceinline__ unsigned char jd_limit(int x) {   // idct_limit of codecs.cpp
  const int i = x & 1023;
  if (i < 128) return (unsigned char)(128 + i);
  if (i < 512) return 255;
  if (i < 896) return 0;
  return (unsigned char)(i - 896);
}

// One thread per 8 x 8 block: idct_islow of codecs.cpp, statement for statement
__global__ __launch_bounds__(64) void jd_idct_kernel(unsigned long long* stamp, JdRecon g, const short* __restrict__ coef, unsigned char* __restrict__ planes) {
  const KStamp kstamp_(stamp);
  typedef long long L;
  const int gb = blockIdx.x * blockDim.x + threadIdx.x;
  if (gb >= g.blocks) return;
  int c = 0;
  if (g.ncomp == 3) c = gb >= g.coef_off[2] ? 2 : (gb >= g.coef_off[1] ? 1 : 0);
  const int lb = gb - g.coef_off[c];
  const int by = lb / g.bw[c], bx = lb - by * g.bw[c];
  const short* blk = coef + (long)gb * 64;
  const unsigned short* q = g.qn[c];
  const int CONST_BITS = 13, PASS1_BITS = 2;
  const L F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
          F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
          F_2_562915447 = 20995, F_3_072711026 = 25172;
  L ws[64];
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    L in[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = (L)((int)blk[r * 8 + col] * (int)q[r * 8 + col]);
    L z2 = in[2], z3 = in[6];
    L z1 = (z2 + z3) * F_0_541196100;
    L tmp2 = z1 + z3 * (-F_1_847759065);
    L tmp3 = z1 + z2 * F_0_765366865;
    z2 = in[0]; z3 = in[4];
    L tmp0 = (z2 + z3) * ((L)1 << CONST_BITS);
    L tmp1 = (z2 - z3) * ((L)1 << CONST_BITS);
    const L tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    L z4 = tmp1 + tmp3;
    const L z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336; tmp1 *= F_2_053119869; tmp2 *= F_3_072711026; tmp3 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const int n = CONST_BITS - PASS1_BITS;
    const L rnd = (L)1 << (n - 1);
    ws[col] = (tmp10 + tmp3 + rnd) >> n;      ws[56 + col] = (tmp10 - tmp3 + rnd) >> n;
    ws[8 + col] = (tmp11 + tmp2 + rnd) >> n;  ws[48 + col] = (tmp11 - tmp2 + rnd) >> n;
    ws[16 + col] = (tmp12 + tmp1 + rnd) >> n; ws[40 + col] = (tmp12 - tmp1 + rnd) >> n;
    ws[24 + col] = (tmp13 + tmp0 + rnd) >> n; ws[32 + col] = (tmp13 - tmp0 + rnd) >> n;
  }
  const int stride = g.bw[c] * 8;
  unsigned char* out = planes + g.plane_off[c] + (long)(by * 8) * stride + bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const L* w = ws + r * 8;
    L z2 = w[2], z3 = w[6];
    L z1 = (z2 + z3) * F_0_541196100;
    L tmp2 = z1 + z3 * (-F_1_847759065);
    L tmp3 = z1 + z2 * F_0_765366865;
    L tmp0 = (w[0] + w[4]) * ((L)1 << CONST_BITS);
    L tmp1 = (w[0] - w[4]) * ((L)1 << CONST_BITS);
    const L tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = w[7]; tmp1 = w[5]; tmp2 = w[3]; tmp3 = w[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    L z4 = tmp1 + tmp3;
    const L z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336; tmp1 *= F_2_053119869; tmp2 *= F_3_072711026; tmp3 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const int S = CONST_BITS + PASS1_BITS + 3;
    const L rnd = (L)1 << (S - 1);
    const unsigned o0 = jd_limit((int)((tmp10 + tmp3 + rnd) >> S)), o7 = jd_limit((int)((tmp10 - tmp3 + rnd) >> S));
    const unsigned o1 = jd_limit((int)((tmp11 + tmp2 + rnd) >> S)), o6 = jd_limit((int)((tmp11 - tmp2 + rnd) >> S));
    const unsigned o2 = jd_limit((int)((tmp12 + tmp1 + rnd) >> S)), o5 = jd_limit((int)((tmp12 - tmp1 + rnd) >> S));
    const unsigned o3 = jd_limit((int)((tmp13 + tmp0 + rnd) >> S)), o4 = jd_limit((int)((tmp13 - tmp0 + rnd) >> S));
    uint2 v;
    v.x = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
    v.y = o4 | (o5 << 8) | (o6 << 16) | (o7 << 24);
    *reinterpret_cast<uint2*>(out + (long)r * stride) = v;   // planes are 256-byte aligned and their pitch is a multiple of 8
  }
}

// The full-resolution sample of component c at (x, y): upsample() of codecs.cpp evaluated at one pixel
__device__ __forceinline__ int jd_sample(const JdRecon& g, const unsigned char* __restrict__ planes, int c, int x, int y) {
  const unsigned char* p = planes + g.plane_off[c];
  const int stride = g.bw[c] * 8, dw = g.dw[c], dh = g.dh[c];
  const int hs = g.hmax / g.h[c], vs = g.vmax / g.v[c];
  const auto row = [&](int yy) { return p + (long)min(max(yy, 0), dh - 1) * stride; };
  const bool fancy = dw > 2;
  if (hs == 1 && vs == 1) return row(y)[x];
  if (hs == 2 && vs == 1) {
    const unsigned char* in = row(y);
    const int i = x >> 1;
    if (!fancy) return in[i];
    if (x & 1) return i == dw - 1 ? in[i] : (in[i] * 3 + in[i + 1] + 2) >> 2;
    return i == 0 ? in[0] : (in[i] * 3 + in[i - 1] + 1) >> 2;
  }
  if (hs == 2 && vs == 2) {
    const int iy = y >> 1, i = x >> 1;
    const unsigned char* in0 = row(iy);
    if (!fancy) return in0[i];
    const unsigned char* in1 = row((y & 1) ? iy + 1 : iy - 1);
    const int cur = in0[i] * 3 + in1[i];
    if (x & 1) {
      if (i == dw - 1) return (cur * 4 + 7) >> 4;
      return (cur * 3 + in0[i + 1] * 3 + in1[i + 1] + 7) >> 4;
    }
    if (i == 0) return (cur * 4 + 8) >> 4;
    return (cur * 3 + in0[i - 1] * 3 + in1[i - 1] + 8) >> 4;
  }
  if (hs == 1 && vs == 2) {
    const int iy = y >> 1;
    const unsigned char* in0 = row(iy);
    const unsigned char* in1 = row((y & 1) ? iy + 1 : iy - 1);
    return (in0[x] * 3 + in1[x] + ((y & 1) ? 2 : 1)) >> 2;
  }
  return row(y / vs)[x / hs];
}

__device__ __forceinline__ unsigned jd_clamp255(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// packed B | G << 8 | R << 16 of pixel (x, y)
__device__ __forceinline__ unsigned jd_pixel(const JdRecon& g, const unsigned char* __restrict__ planes, int x, int y) {
  if (g.ncomp == 1) {
    const unsigned v = planes[g.plane_off[0] + (long)y * (g.bw[0] * 8) + x];
    return v | (v << 8) | (v << 16);
  }
  const int a = jd_sample(g, planes, 0, x, y), b = jd_sample(g, planes, 1, x, y), c = jd_sample(g, planes, 2, x, y);
  if (g.rgb) return (unsigned)c | ((unsigned)b << 8) | ((unsigned)a << 16);
  // jdcolor.c build_ycc_rgb_table / ycc_rgb_convert, the tables' entries computed in place (64-bit as on the host)
  const long long cb = b - 128, cr = c - 128;
  const int cr_r = (int)((91881LL * cr + 32768LL) >> 16);
  const int cb_b = (int)((116130LL * cb + 32768LL) >> 16);
  const int gg = (int)((-22554LL * cb + 32768LL + -46802LL * cr) >> 16);
  return jd_clamp255(a + cb_b) | (jd_clamp255(a + gg) << 8) | (jd_clamp255(a + cr_r) << 16);
}

// any destination: one thread per pixel, byte stores through the view
__global__ __launch_bounds__(256) void jd_color_kernel(unsigned long long* stamp, JdRecon g, const unsigned char* __restrict__ planes, FrameView dv) {
  const KStamp kstamp_(stamp);
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (unsigned)g.W * (unsigned)g.H) return;
  const int y = (int)(i / (unsigned)g.W), x = (int)(i - (unsigned)y * g.W);
  const unsigned p = jd_pixel(g, planes, x, y);
  unsigned char* o = dv.data + y * dv.row + x * dv.pix;
  o[dv.off[0]] = (unsigned char)(p & 0xffu);
  o[dv.off[1]] = (unsigned char)((p >> 8) & 0xffu);
  o[dv.off[2]] = (unsigned char)(p >> 16);
}

// packed BGR with data and pitch aligned to 16 bytes: one thread per 16 pixels of a row = three 16-byte stores (a row's tail of
// fewer than 16 pixels goes out as bytes)
__global__ __launch_bounds__(256) void jd_color_bgr16_kernel(unsigned long long* stamp, JdRecon g, const unsigned char* __restrict__ planes, unsigned char* __restrict__ dst,
                                                           long drow) {
  const KStamp kstamp_(stamp);
  const int per_row = (g.W + 15) >> 4;
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (unsigned)per_row * (unsigned)g.H) return;
  const int y = (int)(i / (unsigned)per_row), x0 = (int)(i - (unsigned)y * per_row) * 16;
  unsigned char* o = dst + (long)y * drow + 3L * x0;
  if (x0 + 16 <= g.W) {
    unsigned w[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned p0 = jd_pixel(g, planes, x0 + 4 * q, y), p1 = jd_pixel(g, planes, x0 + 4 * q + 1, y);
      const unsigned p2 = jd_pixel(g, planes, x0 + 4 * q + 2, y), p3 = jd_pixel(g, planes, x0 + 4 * q + 3, y);
      w[3 * q] = p0 | (p1 << 24);
      w[3 * q + 1] = (p1 >> 8) | (p2 << 16);
      w[3 * q + 2] = (p2 >> 16) | (p3 << 8);
    }
    uint4* o4 = reinterpret_cast<uint4*>(o);
    o4[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o4[1] = make_uint4(w[4], w[5], w[6], w[7]);
    o4[2] = make_uint4(w[8], w[9], w[10], w[11]);
  } else {
    for (int x = x0; x < g.W; ++x) {
      const unsigned p = jd_pixel(g, planes, x, y);
      o[3 * (x - x0)] = (unsigned char)(p & 0xffu);
      o[3 * (x - x0) + 1] = (unsigned char)((p >> 8) & 0xffu);
      o[3 * (x - x0) + 2] = (unsigned char)(p >> 16);
    }
  }
}

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

JdLayout jd_layout(long blocks, long plane_bytes, size_t nwords, size_t nsegs, size_t nsubs, int group) {
  JdLayout L;
  size_t o = 0;
  const auto take = [&](size_t bytes) { const size_t at = o; o = up256(o + bytes); return at; };
  // the part the host stages and one copy brings over: the scan, the tables, the segment and subsequence lists
  L.words = take(nwords * 4);
  L.tab = take(sizeof(JdTables));
  L.segs = take(nsegs * sizeof(JdSeg));
  L.subs = take(nsubs * sizeof(JdSub));
  L.staged = o;
  const size_t groups = nsubs ? (nsubs + group - 1) / group : 0;
  L.ngroups = (int)groups;
  L.entry = take(nsubs * sizeof(JdState));
  L.exit_ = take(nsubs * sizeof(JdState));
  L.count = take(nsubs * sizeof(int));
  L.excl = take((nsubs + 1) * sizeof(int));
  L.gexit = take(2 * groups * sizeof(JdState));
  L.flags = take((groups + 1) * sizeof(int));   // zeroed per frame together with the status word behind it
  L.status = L.flags + groups * sizeof(int);
  L.coef = take((size_t)blocks * 64 * sizeof(short));
  L.dcsum = take((size_t)blocks * sizeof(int));
  L.planes = take((size_t)plane_bytes);
  L.total = o;
  return L;
}

// Everything between the staged bytes and the coefficients: zero the coefficients, the round flags and set the status word, then the
// rounds, the scan, the final pass and the DC sums.  group = T (subsequences per workgroup, <= 1024).
hipError_t launch_jpeg_entropy(unsigned long long* stamp, const JdDev& d, int group, int mcus, int ncomp, long blocks, hipStream_t stream) {
  hipError_t st;
  if ((st = hipMemsetAsync(d.coef, 0, (size_t)blocks * 64 * sizeof(short), stream)) != hipSuccess) return st;
  if ((st = hipMemsetAsync(d.flags, 0, (size_t)d.ngroups * sizeof(int), stream)) != hipSuccess) return st;
  if ((st = hipMemsetAsync(d.status, 0xff, sizeof(unsigned), stream)) != hipSuccess) return st;
  const int threads = (group + 63) / 64 * 64;
  for (int r = 0; r < d.ngroups; ++r)
    hipLaunchKernelGGL(jd_sync_kernel, dim3(d.ngroups), dim3(threads), 0, stream, stamp, d, r, group);
  hipLaunchKernelGGL(jd_scan_kernel, dim3(1), dim3(1024), 0, stream, stamp, d);
  hipLaunchKernelGGL(jd_write_kernel, dim3((d.nsub + 255) / 256), dim3(256), 0, stream, stamp, d);
  hipLaunchKernelGGL(jd_dc_kernel, dim3(ncomp), dim3(1024), 0, stream, stamp, d, mcus);
  return hipGetLastError();
}

hipError_t launch_jpeg_reconstruct(unsigned long long* stamp, const JdRecon& g, const short* coef, unsigned char* planes, const FrameView& dv, hipStream_t stream) {
  hipLaunchKernelGGL(jd_idct_kernel, dim3((g.blocks + 63) / 64), dim3(64), 0, stream, stamp, g, coef, planes);
  const bool bgr16 = dv.pix == 3 && dv.off[0] == 0 && dv.off[1] == 1 && dv.off[2] == 2 && ((uintptr_t)dv.data & 15) == 0 && dv.row % 16 == 0;
  if (bgr16) {
    const long n = (long)((g.W + 15) / 16) * g.H;
    hipLaunchKernelGGL(jd_color_bgr16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, stamp, g, planes, dv.data, dv.row);
  } else {
    const long n = (long)g.W * g.H;
    hipLaunchKernelGGL(jd_color_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, stamp, g, planes, dv);
  }
  return hipGetLastError();
}

}  // namespace rtp

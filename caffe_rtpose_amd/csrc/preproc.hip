// preproc.hip — row a1 on the GPU: from the decoded u8 BGR frame to the net input,
// bit-identical to the host restatement in preprocess.cpp (which restates OpenCV's warpAffine
// INTER_CUBIC / resize INTER_AREA as used by rtpose.cpp:322-368):
//   warp_cubic_kernel : display-fit scale, 1/32-pixel fixed-point coordinates, OpenCV's 2-D table of 15-bit cubic weights,
//                       one rounding per pixel, BORDER_CONSTANT 0 — pure integer arithmetic.
//   area_pad_kernel   : per scale, fractional-area resize (float accumulation in the host's order:
//                       x-sum per source row, then beta-weighted row sum), round-to-nearest-even — or, where the level ENLARGES
//                       an axis, OpenCV's fixed-point bilinear kernel with area-mode coefficients —,
//                       u8/256 - 0.5, centre zero-pad into the net frame (process_and_pad_image).
//   frame_import / frame_export : a caller's u8 view in device memory (any pitch, HWC BGR/RGB/BGRA/RGBA, planar) <-> the packed BGR
//                       image the kernels above and the renderer work on; the warp reads such a view in place (warp_cubic_view_kernel).
// Compiled with -ffp-contract=off.  HBM-bound streaming kernels: 2.8 MB in, 11.6 MB out per 720p frame.
#include <cstring>

#include "kernels.h"

// built with the BITEXACT flags of csrc/Makefile (no packed-f32 VALU; see postproc.hip)

namespace rtp {

// Source addressing of the cubic warp: the engine's packed BGR frame, or a caller's view read in place (rtp_submit_frame_device)
struct PackedSrc {
  const unsigned char* __restrict__ p;
  int w;
  __device__ __forceinline__ const unsigned char* px(int x, int y) const { return p + ((size_t)y * w + x) * 3; }
  __device__ __forceinline__ int at(const unsigned char* q, int c) const { return q[c]; }
};
struct ViewSrc {
  const unsigned char* __restrict__ p;
  long row, pix, o0, o1, o2;
  __device__ __forceinline__ const unsigned char* px(int x, int y) const { return p + y * row + x * pix; }
  __device__ __forceinline__ int at(const unsigned char* q, int c) const { return q[c == 0 ? o0 : (c == 1 ? o1 : o2)]; }
};

template <class Src>
__device__ __forceinline__ void warp_cubic_px(const Src& src, int sw, int sh, double inv, const short* __restrict__ tab2d, unsigned char* __restrict__ dst,
                                              int dw, int dh) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= dw) return;
  const int INTER_BITS = 5, INTER_TAB = 1 << INTER_BITS, AB_BITS = 10, AB_SCALE = 1 << AB_BITS, COEF_BITS = 15;
  const int round_delta = AB_SCALE / INTER_TAB / 2;
  const int Y0 = (int)__double2ll_rn((inv * y) * AB_SCALE) + round_delta;
  const int Y = Y0 >> (AB_BITS - INTER_BITS);
  const int sy = (Y >> INTER_BITS) - 1, fy = Y & (INTER_TAB - 1);
  const int X = (round_delta + (int)__double2ll_rn(inv * x * AB_SCALE)) >> (AB_BITS - INTER_BITS);
  const int sx = (X >> INTER_BITS) - 1, fx = X & (INTER_TAB - 1);
  const short* w = tab2d + ((size_t)fy * 32 + fx) * 16;   // remapBicubic: 16 fixed-point weights, one rounding per pixel
  int acc[3] = {0, 0, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int yy = sy + r;
    if (yy < 0 || yy >= sh) continue;   // BORDER_CONSTANT, value 0
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int xx = sx + q;
      if (xx < 0 || xx >= sw) continue;
      const unsigned char* p = src.px(xx, yy);
      const int wv = w[r * 4 + q];
      acc[0] += src.at(p, 0) * wv; acc[1] += src.at(p, 1) * wv; acc[2] += src.at(p, 2) * wv;
    }
  }
  unsigned char* o = dst + ((size_t)y * dw + x) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = (acc[c] + (1 << (COEF_BITS - 1))) >> COEF_BITS;
    o[c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

__global__ __launch_bounds__(256) void warp_cubic_kernel(unsigned long long* stamp, const unsigned char* __restrict__ src, int sw, int sh, double inv,
                                                         const short* __restrict__ tab2d, unsigned char* __restrict__ dst, int dw, int dh) {
  const KStamp kstamp_(stamp);
  warp_cubic_px(PackedSrc{src, sw}, sw, sh, inv, tab2d, dst, dw, dh);
}

__global__ __launch_bounds__(256) void warp_cubic_view_kernel(unsigned long long* stamp, FrameView v, double inv, const short* __restrict__ tab2d,
                                                              unsigned char* __restrict__ dst, int dw, int dh) {
  const KStamp kstamp_(stamp);
  warp_cubic_px(ViewSrc{v.data, v.row, v.pix, v.off[0], v.off[1], v.off[2]}, v.w, v.h, inv, tab2d, dst, dw, dh);
}

// One thread per pixel of the (net_w x net_h) frame of scale `blockIdx.z`.
__global__ __launch_bounds__(256) void area_pad_kernel(unsigned long long* stamp, const unsigned char* __restrict__ disp, int dw, int dh, AreaScale sc0, AreaScale sc1,
                                                       AreaScale sc2, AreaScale sc3, int nscales_in_launch, float* __restrict__ out, int net_w,
                                                       int net_h, int scale_base) {
  const KStamp kstamp_(stamp);
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  const int si = blockIdx.z;
  if (x >= net_w || si >= nscales_in_launch) return;
  const AreaScale sc = si == 0 ? sc0 : (si == 1 ? sc1 : (si == 2 ? sc2 : sc3));
  const int padw = (net_w - sc.tw) / 2, padh = (net_h - sc.th) / 2;
  float* o = out + (size_t)(scale_base + si) * 3 * net_h * net_w + (size_t)y * net_w + x;
  const size_t plane = (size_t)net_h * net_w;
  const int ox = x - padw, oy = y - padh;
  if (ox < 0 || ox >= sc.tw || oy < 0 || oy >= sc.th) { o[0] = 0.f; o[plane] = 0.f; o[2 * plane] = 0.f; return; }
  float r3[3];
  if (sc.identity) {
    const unsigned char* p = disp + ((size_t)oy * dw + ox) * 3;
    r3[0] = p[0]; r3[1] = p[1]; r3[2] = p[2];
  } else if (sc.linear) {  // an enlarged axis: HResizeLinear into int rows, VResizeLinear's u8 specialisation (integer arithmetic throughout)
    const int* tx = sc.lx + ox * 4;
    const int* ty = sc.ly + oy * 4;
    const unsigned char* r0 = disp + (size_t)ty[0] * dw * 3;
    const unsigned char* r1 = disp + (size_t)ty[1] * dw * 3;
    const int x0 = tx[0] * 3, x1 = tx[1] * 3, a0 = tx[2], a1 = tx[3], b0 = ty[2], b1 = ty[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int d0 = r0[x0 + c] * a0 + r0[x1 + c] * a1;
      const int d1 = r1[x0 + c] * a0 + r1[x1 + c] * a1;
      r3[c] = (float)(unsigned char)((((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2);
    }
  } else if (sc.fast_x > 0) {  // resizeAreaFast_: integer scale; 2x2 rounds half up, other areas go through float * (1.f/area)
    int sum[3] = {0, 0, 0};
    for (int yy = 0; yy < sc.fast_y; ++yy)
      for (int xx = 0; xx < sc.fast_x; ++xx) {
        const unsigned char* p = disp + ((size_t)(oy * sc.fast_y + yy) * dw + ox * sc.fast_x + xx) * 3;
        sum[0] += p[0]; sum[1] += p[1]; sum[2] += p[2];
      }
    const float inv_area = 1.f / (float)(sc.fast_x * sc.fast_y);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int v = (sc.fast_x == 2 && sc.fast_y == 2) ? ((sum[c] + 2) >> 2) : (int)rintf((float)sum[c] * inv_area);
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      r3[c] = (float)v;
    }
  } else {
    const int xs = sc.xstart[ox], xe = sc.xstart[ox + 1];
    const int ys = sc.ystart[oy], ye = sc.ystart[oy + 1];
    float sum[3] = {0.f, 0.f, 0.f};
    for (int yi = ys; yi < ye; ++yi) {
      const unsigned char* srow = disp + (size_t)sc.ysi[yi] * dw * 3;
      const float beta = sc.yalpha[yi];
      float b[3] = {0.f, 0.f, 0.f};
      for (int xi = xs; xi < xe; ++xi) {
        const unsigned char* p = srow + sc.xsi[xi] * 3;
        const float a = sc.xalpha[xi];
        b[0] += p[0] * a; b[1] += p[1] * a; b[2] += p[2] * a;
      }
      sum[0] += beta * b[0]; sum[1] += beta * b[1]; sum[2] += beta * b[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int v = (int)rintf(sum[c]);  // cvRound: round half to even
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      r3[c] = (float)v;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * plane] = r3[c] / 256.0f - 0.5f;
}

// ---- caller frames in device memory (rtp_submit_frame_device, rtp_collect_rendered_device) ---------------------------------------
// Streaming copies between a caller's view and the engine's packed BGR image.  The specialised layouts give each thread 4 pixels of a row:
// 12 bytes of packed BGR as three dwords against three dwords of HWC3, four of HWC4 or one per plane, the bytes moved with constant
// shifts.  One flat grid over the w/4 x h groups (no half-empty block at the end of every row).  Export writes only the three named
// channels: a 4-channel view's pixel is read and its 4th byte written back as it was.
__device__ __forceinline__ unsigned byte_at(const unsigned* w, int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }
__device__ __forceinline__ void set_byte(unsigned* w, int i, unsigned b) {
  const int s = (i & 3) * 8;
  w[i >> 2] = (w[i >> 2] & ~(0xffu << s)) | (b << s);
}

// PS = bytes per pixel of an HWC view (channel c of pixel k at byte k * PS + (SWAP ? 2 - c : c)); PS == 1: planar (plane c at off[c])
template <int PS, bool SWAP>
__global__ __launch_bounds__(256) void frame_import_vec_kernel(unsigned long long* stamp, FrameView v, unsigned char* __restrict__ dst) {
  const KStamp kstamp_(stamp);
  const int gw = v.w >> 2;
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;   // (the host refuses views of 2^31 pixels or more)
  if (g >= (unsigned)gw * (unsigned)v.h) return;
  const int y = (int)(g / (unsigned)gw), x = 4 * (int)(g - (unsigned)y * gw);
  const unsigned char* row = v.data + y * v.row;
  unsigned out[3] = {0u, 0u, 0u};
  if (PS == 1) {
    unsigned in[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) in[c] = *(const unsigned*)(row + v.off[c] + x);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) set_byte(out, k * 3 + c, byte_at(&in[c], k));
  } else {
    const unsigned* p = (const unsigned*)(row + (size_t)x * PS);
    unsigned in[PS];
#pragma unroll
    for (int i = 0; i < PS; ++i) in[i] = p[i];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) set_byte(out, k * 3 + c, byte_at(in, k * PS + (SWAP ? 2 - c : c)));
  }
  unsigned* o = (unsigned*)(dst + ((size_t)y * v.w + x) * 3);
  o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}

template <int PS, bool SWAP>
__global__ __launch_bounds__(256) void frame_export_vec_kernel(unsigned long long* stamp, const unsigned char* __restrict__ src, FrameView v) {
  const KStamp kstamp_(stamp);
  const int gw = v.w >> 2;
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;   // (the host refuses views of 2^31 pixels or more)
  if (g >= (unsigned)gw * (unsigned)v.h) return;
  const int y = (int)(g / (unsigned)gw), x = 4 * (int)(g - (unsigned)y * gw);
  const unsigned* s = (const unsigned*)(src + ((size_t)y * v.w + x) * 3);
  const unsigned in[3] = {s[0], s[1], s[2]};
  unsigned char* row = v.data + y * v.row;
  if (PS == 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      unsigned o = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) set_byte(&o, k, byte_at(in, k * 3 + c));
      *(unsigned*)(row + v.off[c] + x) = o;
    }
  } else {
    unsigned* p = (unsigned*)(row + (size_t)x * PS);
    unsigned o[PS];
#pragma unroll
    for (int i = 0; i < PS; ++i) o[i] = PS == 4 ? p[i] : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) set_byte(o, k * PS + (SWAP ? 2 - c : c), byte_at(in, k * 3 + c));
#pragma unroll
    for (int i = 0; i < PS; ++i) p[i] = o[i];
  }
}

// any other view: one thread per pixel, byte gather / scatter
__global__ __launch_bounds__(256) void frame_import_generic_kernel(unsigned long long* stamp, FrameView v, unsigned char* __restrict__ dst) {
  const KStamp kstamp_(stamp);
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (unsigned)v.w * (unsigned)v.h) return;
  const int y = (int)(g / (unsigned)v.w), x = (int)(g - (unsigned)y * v.w);
  const unsigned char* p = v.data + y * v.row + x * v.pix;
  unsigned char* o = dst + (size_t)g * 3;
  o[0] = p[v.off[0]]; o[1] = p[v.off[1]]; o[2] = p[v.off[2]];
}

__global__ __launch_bounds__(256) void frame_export_generic_kernel(unsigned long long* stamp, const unsigned char* __restrict__ src, FrameView v) {
  const KStamp kstamp_(stamp);
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (unsigned)v.w * (unsigned)v.h) return;
  const int y = (int)(g / (unsigned)v.w), x = (int)(g - (unsigned)y * v.w);
  unsigned char* p = v.data + y * v.row + x * v.pix;
  const unsigned char* s = src + (size_t)g * 3;
  p[v.off[0]] = s[0]; p[v.off[1]] = s[1]; p[v.off[2]] = s[2];
}

int frame_layout(const FrameView& v, size_t avail) {
  const auto al4 = [&](long o) { return (((uintptr_t)v.data + (uintptr_t)o) & 3) == 0; };
  if (v.w % 4 || v.row % 4 || !al4(0)) return LAYOUT_GENERIC;
  const bool bgr = v.off[0] == 0 && v.off[1] == 1 && v.off[2] == 2, rgb = v.off[0] == 2 && v.off[1] == 1 && v.off[2] == 0;
  if (v.pix == 3 && (bgr || rgb)) return bgr ? LAYOUT_HWC3_BGR : LAYOUT_HWC3_RGB;
  if (v.pix == 4 && (bgr || rgb) && (size_t)(v.h - 1) * (size_t)v.row + (size_t)v.w * 4 <= avail) return bgr ? LAYOUT_HWC4_BGR : LAYOUT_HWC4_RGB;
  if (v.pix == 1 && al4(v.off[0]) && al4(v.off[1]) && al4(v.off[2])) return LAYOUT_PLANAR;
  return LAYOUT_GENERIC;
}

hipError_t launch_frame_import(unsigned long long* stamp, const FrameView& v, int layout, unsigned char* dst, hipStream_t stream) {
  const long n = layout == LAYOUT_GENERIC ? (long)v.w * v.h : (long)(v.w / 4) * v.h;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  switch (layout) {
    case LAYOUT_HWC3_BGR: hipLaunchKernelGGL((frame_import_vec_kernel<3, false>), grid, block, 0, stream, stamp, v, dst); break;
    case LAYOUT_HWC3_RGB: hipLaunchKernelGGL((frame_import_vec_kernel<3, true>), grid, block, 0, stream, stamp, v, dst); break;
    case LAYOUT_HWC4_BGR: hipLaunchKernelGGL((frame_import_vec_kernel<4, false>), grid, block, 0, stream, stamp, v, dst); break;
    case LAYOUT_HWC4_RGB: hipLaunchKernelGGL((frame_import_vec_kernel<4, true>), grid, block, 0, stream, stamp, v, dst); break;
    case LAYOUT_PLANAR: hipLaunchKernelGGL((frame_import_vec_kernel<1, false>), grid, block, 0, stream, stamp, v, dst); break;
    default: hipLaunchKernelGGL(frame_import_generic_kernel, grid, block, 0, stream, stamp, v, dst); break;
  }
  return hipGetLastError();
}

hipError_t launch_frame_export(unsigned long long* stamp, const unsigned char* src, const FrameView& v, int layout, hipStream_t stream) {
  const long n = layout == LAYOUT_GENERIC ? (long)v.w * v.h : (long)(v.w / 4) * v.h;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  switch (layout) {
    case LAYOUT_HWC3_BGR: hipLaunchKernelGGL((frame_export_vec_kernel<3, false>), grid, block, 0, stream, stamp, src, v); break;
    case LAYOUT_HWC3_RGB: hipLaunchKernelGGL((frame_export_vec_kernel<3, true>), grid, block, 0, stream, stamp, src, v); break;
    case LAYOUT_HWC4_BGR: hipLaunchKernelGGL((frame_export_vec_kernel<4, false>), grid, block, 0, stream, stamp, src, v); break;
    case LAYOUT_HWC4_RGB: hipLaunchKernelGGL((frame_export_vec_kernel<4, true>), grid, block, 0, stream, stamp, src, v); break;
    case LAYOUT_PLANAR: hipLaunchKernelGGL((frame_export_vec_kernel<1, false>), grid, block, 0, stream, stamp, src, v); break;
    default: hipLaunchKernelGGL(frame_export_generic_kernel, grid, block, 0, stream, stamp, src, v); break;
  }
  return hipGetLastError();
}

hipError_t launch_warp_view(unsigned long long* stamp, const FrameView& v, double inv, const short* tab2d, unsigned char* dst, int dw, int dh, hipStream_t stream) {
  dim3 grid((dw + 255) / 256, dh);
  hipLaunchKernelGGL(warp_cubic_view_kernel, grid, dim3(256), 0, stream, stamp, v, inv, tab2d, dst, dw, dh);
  return hipGetLastError();
}

hipError_t launch_warp(unsigned long long* stamp, const unsigned char* src, int sw, int sh, double inv, const short* tab2d, unsigned char* dst, int dw, int dh,
                       hipStream_t stream) {
  dim3 grid((dw + 255) / 256, dh);
  hipLaunchKernelGGL(warp_cubic_kernel, grid, dim3(256), 0, stream, stamp, src, sw, sh, inv, tab2d, dst, dw, dh);
  return hipGetLastError();
}

hipError_t launch_area_pad(unsigned long long* stamp, const unsigned char* disp, int dw, int dh, const AreaScale* scales, int nscales, float* out, int net_w, int net_h,
                           hipStream_t stream) {
  for (int base = 0; base < nscales; base += 4) {
    const int n = nscales - base < 4 ? nscales - base : 4;
    AreaScale z;
    memset(&z, 0, sizeof z);
    const AreaScale& a = scales[base];
    const AreaScale& b = n > 1 ? scales[base + 1] : z;
    const AreaScale& c = n > 2 ? scales[base + 2] : z;
    const AreaScale& d = n > 3 ? scales[base + 3] : z;
    dim3 grid((net_w + 255) / 256, net_h, n);
    hipLaunchKernelGGL(area_pad_kernel, grid, dim3(256), 0, stream, stamp, disp, dw, dh, a, b, c, d, n, out, net_w, net_h, base);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace rtp

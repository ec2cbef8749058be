// resize_math.h — the arithmetic of ImResize (imresize_layer.cu:9-18,99-155) that more than one kernel file evaluates: the cubic
// interpolation and the 8 x 8 output block of resize_kernel.  Device code of postproc.hip and maps_export.hip only; both files are
// built with -ffp-contract=off (csrc/Makefile BITEXACT), so every operation below rounds where the reference's source rounds and
// every kernel that calls these functions returns the same bits for the same low-res maps.
#pragma once
#include "kernels.h"

namespace rtp {

// imresize_layer.cu:14-17 with C++'s usual arithmetic conversions spelled out, in two halves: the three sub-expressions that do
// not depend on the fraction (8 consecutive outputs along an axis share them), and the evaluation at a fraction.  Same
// operations in the same order as the one-piece expression (no contraction in these files): cubic_interp IS this pair.
struct CubicCoef { float a; double b; float c; float v1; };
__device__ __forceinline__ CubicCoef cubic_coef(float v0, float v1, float v2, float v3) {
  CubicCoef k;
  k.a = (-0.5f * v0 + 1.5f * v1 - 1.5f * v2 + 0.5f * v3);
  k.b = ((double)(v0 - 2.5f * v1) + 2.0 * (double)v2 - 0.5 * (double)v3);
  k.c = (-0.5f * v0 + 0.5f * v2);
  k.v1 = v1;
  return k;
}
__device__ __forceinline__ float cubic_eval(const CubicCoef& k, float dx) {
  const float t1 = k.a * dx * dx * dx;
  const double t2 = k.b * (double)dx * (double)dx;
  const float t3 = k.c * dx;
  return (float)((((double)t1 + t2) + (double)t3) + (double)k.v1);
}
__device__ __forceinline__ float cubic_interp(float v0, float v1, float v2, float v3, float dx) {
  return cubic_eval(cubic_coef(v0, v1, v2, v3), dx);
}

// The 8 x 8 block of outputs (x0 .. x0 + 7, y0 .. y0 + 7; x0 = 8k - 4, y0 = 8m - 4) of one channel, summed over the scales in order;
// the caller divides by p.num last.  src_c = the channel's map at scale 0.  For the full-size scale such a block shares ONE 4x4
// low-res neighbourhood, so the 4 row interpolations t[i] of an output column are computed once and reused by the 8 output rows
// (1.5 cubic evaluations per output instead of 5) and the 16 neighbours are loaded once per block.  Per-output arithmetic and
// rounding are exactly the reference kernel's; whenever the neighbourhood of an output differs from the previous one (other
// scales, borders) it is simply recomputed.  Outputs outside the map keep 0.
__device__ __forceinline__ void resize_block8(const ResizeParams& p, const float* src_c, int x0, int y0, float (&sum)[8][8]) {
  const long src_offset = (long)p.C * p.h * p.w;
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[r][j] = 0.f;
  for (int n = 0; n < p.num; ++n) {
    const int padw = (int)floorf((float)(p.w / 2) * (1 - p.start_scale + n * p.scale_gap));
    const int padh = (int)floorf((float)(p.h / 2) * (1 - p.start_scale + n * p.scale_gap));
    const int ow = p.w - 2 * padw, oh = p.h - 2 * padh;
    const float* sp = src_c + n * src_offset;
    const float offset_x = (float)((double)(p.tw / (float)ow / 2) - 0.5);
    const float offset_y = (float)((double)(p.th / (float)oh / 2) - 0.5);
    const int rw = ow + 2 * padw;
    float t[4][8];   // row interpolations of the current y-neighbourhood, per output column
    int prev_y = -1;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int y = y0 + r;
      if (y < 0 || y >= p.th) continue;
      const float y_on = (y - offset_y) * ((float)oh / p.th);
      int yn1 = (int)((double)y_on + 1e-5);
      yn1 = (yn1 < 0) ? 0 : yn1;
      const float dy = y_on - yn1;
      if (yn1 != prev_y) {
        prev_y = yn1;
        int yn[4];
        yn[0] = ((yn1 - 1 < 0) ? yn1 : (yn1 - 1)) + padh;
        yn[2] = (yn1 + 1 >= oh) ? (oh - 1) : (yn1 + 1);
        yn[3] = ((yn[2] + 1 >= oh) ? (oh - 1) : (yn[2] + 1)) + padh;
        yn[1] = yn1 + padh;
        yn[2] += padh;
        float v[4][4];
        int prev_x = -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int x = x0 + j;
          if (x < 0 || x >= p.tw) continue;
          const float x_on = (x - offset_x) * ((float)ow / p.tw);
          int xn1 = (int)((double)x_on + 1e-5);
          xn1 = (xn1 < 0) ? 0 : xn1;
          const float dx = x_on - xn1;
          if (xn1 != prev_x) {
            prev_x = xn1;
            const int xn0 = ((xn1 - 1 < 0) ? xn1 : (xn1 - 1)) + padw;
            const int xn2 = (xn1 + 1 >= ow) ? (ow - 1) : (xn1 + 1);
            const int xn3 = ((xn2 + 1 >= ow) ? (ow - 1) : (xn2 + 1)) + padw;
            const int xa = xn1 + padw, xb = xn2 + padw;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float* rr = sp + yn[i] * rw;
              v[i][0] = rr[xn0]; v[i][1] = rr[xa]; v[i][2] = rr[xb]; v[i][3] = rr[xn3];
            }
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) t[i][j] = cubic_interp(v[i][0], v[i][1], v[i][2], v[i][3], dx);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int x = x0 + j;
        if (x < 0 || x >= p.tw) continue;
        const float d = cubic_interp(t[0][j], t[1][j], t[2][j], t[3][j], dy);
        sum[r][j] = sum[r][j] + d;
      }
    }
  }
}

}  // namespace rtp

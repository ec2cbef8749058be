// yuv_export.hip — a u8 BGR image in device memory (the rendered frame, or any rtp_frame_view) -> 8-bit YUV planes (I420 / YV12 / NV12 /
// NV21 / 4:2:2 / 4:4:4 / luma only): rtp_convert_to_yuv_device, rtp_set_render_yuv, rtp_collect_rendered_yuv_device.  The other direction
// of yuv_import.hip.  BT.601 limited range in the integer arithmetic of codecs.cpp's rtp_convert_bgr_to_yuv, bit for bit:
//   Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16                       per pixel
//   U = ((-38 R - 74 G + 112 B + 128) >> 8) + 128                     per chroma sample, on the rounded mean of the cell's pixels
//   V = ((112 R - 94 G - 18 B + 128) >> 8) + 128                      (coordinates clamped to the last column / row)
// (arithmetic shift).  Over the whole 2^24 cube Y stays in 16..235 and U, V in 16..240, so there is no clamp: every value is a byte as it
// stands (nothing here has the shift-then-clamp shape of yuv_import.hip's shr8_u8 remark; the whole-cube tests of both kernels guard it).
// Streaming kernels: 2.76 MB in, 1.38 MB out per 720p 4:2:0 frame.  No kernel addresses a byte outside the source view or outside the
// planes as the view describes them: the 4 x 2 kernel runs only where every block is whole (yuv_export_layout), the generic one moves
// single bytes.
#include "kernels.h"

namespace rtp {

__device__ __forceinline__ unsigned luma_px(unsigned b, unsigned g, unsigned r) { return ((66u * r + 129u * g + 25u * b + 128u) >> 8) + 16u; }
__device__ __forceinline__ unsigned cb_px(int b, int g, int r) { return (unsigned)(((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128); }
__device__ __forceinline__ unsigned cr_px(int b, int g, int r) { return (unsigned)(((112 * r - 94 * g - 18 * b + 128) >> 8) + 128); }

// 4:2:0 from packed BGR, one thread per 4 x 2 luma block: two rows of three dword loads, two dword luma stores, the block's two U and
// two V samples as one 16-bit store per plane (PLANAR) or one dword (NV12: u, v, u, v; NV21: v, u, v, u).  Neighbouring lanes hold
// neighbouring blocks of a row.  MODE: YUV_420_PLANAR, YUV_420_NV12 or YUV_420_NV21.
template <int MODE>
__global__ __launch_bounds__(256) void yuv420_export_kernel(unsigned long long* stamp, const unsigned char* __restrict__ src, long srow, YuvView d) {
  const KStamp kstamp_(stamp);
  const int gw = d.w >> 2;
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;   // (the host refuses views of 2^31 pixels or more)
  if (g >= (unsigned)gw * (unsigned)(d.h >> 1)) return;
  const int by = (int)(g / (unsigned)gw), bx = (int)(g - (unsigned)by * gw);
  const unsigned char* srow0 = src + (size_t)(2 * by) * srow + 12 * bx;
  unsigned yy[2];
  int sb[2] = {0, 0}, sg[2] = {0, 0}, sr[2] = {0, 0};   // channel sums of the block's two 2 x 2 cells
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned* in = (const unsigned*)(srow0 + (size_t)r * srow);
    const unsigned a0 = in[0], a1 = in[1], a2 = in[2];
    const unsigned p[4] = {a0 & 0xffffffu, (a0 >> 24) | ((a1 & 0xffffu) << 8), (a1 >> 16) | ((a2 & 0xffu) << 16), a2 >> 8};
    unsigned packed = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned b = p[i] & 0xffu, gg = (p[i] >> 8) & 0xffu, rr = p[i] >> 16;
      packed |= luma_px(b, gg, rr) << (8 * i);
      sb[i >> 1] += (int)b; sg[i >> 1] += (int)gg; sr[i >> 1] += (int)rr;
    }
    yy[r] = packed;
  }
  unsigned char* yrow = const_cast<unsigned char*>(d.y) + (size_t)(2 * by) * d.ys + 4 * bx;
  *(unsigned*)yrow = yy[0];
  *(unsigned*)(yrow + d.ys) = yy[1];
  unsigned u[2], v[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int b = (sb[c] + 2) >> 2, gg = (sg[c] + 2) >> 2, rr = (sr[c] + 2) >> 2;
    u[c] = cb_px(b, gg, rr);
    v[c] = cr_px(b, gg, rr);
  }
  if (MODE == YUV_420_PLANAR) {
    *(unsigned short*)(const_cast<unsigned char*>(d.u) + (size_t)by * d.uvs + 2 * bx) = (unsigned short)(u[0] | (u[1] << 8));
    *(unsigned short*)(const_cast<unsigned char*>(d.v) + (size_t)by * d.uvs + 2 * bx) = (unsigned short)(v[0] | (v[1] << 8));
  } else {
    unsigned char* base = const_cast<unsigned char*>(MODE == YUV_420_NV12 ? d.u : d.v);   // the first byte of the pair
    const unsigned a0 = MODE == YUV_420_NV12 ? u[0] : v[0], b0 = MODE == YUV_420_NV12 ? v[0] : u[0];
    const unsigned a1 = MODE == YUV_420_NV12 ? u[1] : v[1], b1 = MODE == YUV_420_NV12 ? v[1] : u[1];
    *(unsigned*)(base + (size_t)by * d.uvs + 4 * bx) = a0 | (b0 << 8) | (a1 << 16) | (b1 << 24);
  }
}

// any other pair of views: one thread per chroma cell (1 x 1, 2 x 1 or 2 x 2 luma pixels; luma only: per pixel), byte loads of the three
// named channels of the source view, byte stores
__global__ __launch_bounds__(256) void yuv_export_generic_kernel(unsigned long long* stamp, FrameView s, YuvView d) {
  const KStamp kstamp_(stamp);
  const int sx = d.u ? d.sx : 0, sy = d.u ? d.sy : 0;
  const int cw = (d.w + sx) >> sx, ch = (d.h + sy) >> sy;
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (unsigned)cw * (unsigned)ch) return;
  const int cy = (int)(g / (unsigned)cw), cx = (int)(g - (unsigned)cy * cw);
  int sb = 0, sg = 0, sr = 0;
  for (int dy = 0; dy <= sy; ++dy) {
    const int y = (cy << sy) + dy, yc = y < d.h ? y : d.h - 1;   // an odd edge cell repeats its last pixel
    for (int dx = 0; dx <= sx; ++dx) {
      const int x = (cx << sx) + dx, xc = x < d.w ? x : d.w - 1;
      const unsigned char* p = s.data + (size_t)yc * s.row + (size_t)xc * s.pix;
      const unsigned b = p[s.off[0]], gg = p[s.off[1]], rr = p[s.off[2]];
      sb += (int)b; sg += (int)gg; sr += (int)rr;
      if (x < d.w && y < d.h) const_cast<unsigned char*>(d.y)[(size_t)y * d.ys + x] = (unsigned char)luma_px(b, gg, rr);
    }
  }
  if (!d.u) return;
  const int sh = sx + sy, half = (1 << sh) >> 1;   // (sum + 2) >> 2, (sum + 1) >> 1, or the pixel itself
  const int b = (sb + half) >> sh, gg = (sg + half) >> sh, rr = (sr + half) >> sh;
  const size_t c = (size_t)cy * d.uvs + (size_t)cx * d.uvp;
  const_cast<unsigned char*>(d.u)[c] = (unsigned char)cb_px(b, gg, rr);
  const_cast<unsigned char*>(d.v)[c] = (unsigned char)cr_px(b, gg, rr);
}

int yuv_export_layout(const FrameView& s, const YuvView& d) {
  const auto al = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
  if (!d.u || !d.v || d.sx != 1 || d.sy != 1 || d.w % 4 || d.h % 2) return YUV_GENERIC;
  if (s.pix != 3 || s.off[0] != 0 || s.off[1] != 1 || s.off[2] != 2 || !al(s.data, 4) || s.row % 4) return YUV_GENERIC;
  if (!al(d.y, 4) || d.ys % 4) return YUV_GENERIC;
  if (d.uvp == 1) return al(d.u, 2) && al(d.v, 2) && d.uvs % 2 == 0 ? YUV_420_PLANAR : YUV_GENERIC;
  if (d.uvp == 2 && d.uvs % 4 == 0) {
    if (d.v == d.u + 1 && al(d.u, 4)) return YUV_420_NV12;
    if (d.u == d.v + 1 && al(d.v, 4)) return YUV_420_NV21;
  }
  return YUV_GENERIC;
}

hipError_t launch_yuv_export(unsigned long long* stamp, const FrameView& s, const YuvView& d, int layout, hipStream_t stream) {
  const int sx = d.u ? d.sx : 0, sy = d.u ? d.sy : 0;
  const long n = layout == YUV_GENERIC ? (long)((d.w + sx) >> sx) * ((d.h + sy) >> sy) : (long)(d.w / 4) * (d.h / 2);
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  switch (layout) {
    case YUV_420_PLANAR: hipLaunchKernelGGL((yuv420_export_kernel<YUV_420_PLANAR>), grid, block, 0, stream, stamp, s.data, s.row, d); break;
    case YUV_420_NV12: hipLaunchKernelGGL((yuv420_export_kernel<YUV_420_NV12>), grid, block, 0, stream, stamp, s.data, s.row, d); break;
    case YUV_420_NV21: hipLaunchKernelGGL((yuv420_export_kernel<YUV_420_NV21>), grid, block, 0, stream, stamp, s.data, s.row, d); break;
    default: hipLaunchKernelGGL(yuv_export_generic_kernel, grid, block, 0, stream, stamp, s, d); break;
  }
  return hipGetLastError();
}

}  // namespace rtp

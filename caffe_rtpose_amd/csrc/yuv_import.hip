// yuv_import.hip — 8-bit YUV frames (I420 / YV12 / NV12 / NV21 / 4:2:2 / 4:4:4 / luma only) -> the u8 BGR image the pre-processing
// kernels of preproc.hip work on (rtp_submit_frame_yuv, rtp_submit_frame_yuv_device, rtp_convert_yuv_device).  BT.601 limited range in
// the integer arithmetic of codecs.cpp's rtp_convert_yuv (what rtp_video_read makes of a Y4M frame), bit for bit:
//   c = 298 (Y - 16), d = U - 128, e = V - 128
//   R = clamp((c + 409 e + 128) >> 8), G = clamp((c - 100 d - 208 e + 128) >> 8), B = clamp((c + 516 d + 128) >> 8)
// Streaming kernels: 1.38 MB in, 2.76 MB out per 720p 4:2:0 frame.  No kernel addresses a byte outside the planes as the view
// describes them: the 4 x 2 kernel runs only where every block is whole (yuv_layout), the generic one loads single bytes.
#include "kernels.h"

namespace rtp {

// clamp255(x >> 8), written as max(0, min(x, 65535)) >> 8: the same number for every int x, and provably below 256 to the compiler,
// so the bytes can be ORed into a dword.  (In the shift-then-clamp form hipcc pairs channels into v_ashr_pk_u8_i32, whose result
// did not have the zero upper half the packing needs; the whole-cube tests of both kernels guard this.)
__device__ __forceinline__ unsigned shr8_u8(int x) { return (unsigned)(x < 0 ? 0 : (x > 65535 ? 65535 : x)) >> 8; }

// packed B | G << 8 | R << 16 of one pixel
__device__ __forceinline__ unsigned yuv_px(int Y, int d, int e) {
  const int c = 298 * (Y - 16) + 128;
  const unsigned r = shr8_u8(c + 409 * e);
  const unsigned g = shr8_u8(c - 100 * d - 208 * e);
  const unsigned b = shr8_u8(c + 516 * d);
  return b | (g << 8) | (r << 16);
}

// 4:2:0, one thread per 4 x 2 luma block.  MODE: YUV_420_PLANAR, YUV_420_NV12 or YUV_420_NV21.
template <int MODE>
__global__ __launch_bounds__(256) void yuv420_block_kernel(unsigned long long* stamp, YuvView s, unsigned char* __restrict__ dst, long drow) {
  const KStamp kstamp_(stamp);
  const int gw = s.w >> 2;
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;   // (the host refuses views of 2^31 pixels or more)
  if (g >= (unsigned)gw * (unsigned)(s.h >> 1)) return;
  const int by = (int)(g / (unsigned)gw), bx = (int)(g - (unsigned)by * gw);
  const unsigned char* yrow = s.y + (size_t)(2 * by) * s.ys + 4 * bx;
  const unsigned y0 = *(const unsigned*)yrow;
  const unsigned y1 = *(const unsigned*)(yrow + s.ys);
  int d[2], e[2];
  if (MODE == YUV_420_PLANAR) {
    const unsigned uu = *(const unsigned short*)(s.u + (size_t)by * s.uvs + 2 * bx);
    const unsigned vv = *(const unsigned short*)(s.v + (size_t)by * s.uvs + 2 * bx);
    d[0] = (int)(uu & 0xffu) - 128; d[1] = (int)(uu >> 8) - 128;
    e[0] = (int)(vv & 0xffu) - 128; e[1] = (int)(vv >> 8) - 128;
  } else {
    const unsigned char* base = MODE == YUV_420_NV12 ? s.u : s.v;   // the first byte of the pair
    const unsigned q = *(const unsigned*)(base + (size_t)by * s.uvs + 4 * bx);
    const int a0 = (int)(q & 0xffu) - 128, b0 = (int)((q >> 8) & 0xffu) - 128, a1 = (int)((q >> 16) & 0xffu) - 128, b1 = (int)(q >> 24) - 128;
    d[0] = MODE == YUV_420_NV12 ? a0 : b0; e[0] = MODE == YUV_420_NV12 ? b0 : a0;
    d[1] = MODE == YUV_420_NV12 ? a1 : b1; e[1] = MODE == YUV_420_NV12 ? b1 : a1;
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned yy = r ? y1 : y0;
    const unsigned p0 = yuv_px((int)(yy & 0xffu), d[0], e[0]), p1 = yuv_px((int)((yy >> 8) & 0xffu), d[0], e[0]);
    const unsigned p2 = yuv_px((int)((yy >> 16) & 0xffu), d[1], e[1]), p3 = yuv_px((int)(yy >> 24), d[1], e[1]);
    unsigned* o = (unsigned*)(dst + (size_t)(2 * by + r) * drow + 12 * bx);
    o[0] = p0 | (p1 << 24);
    o[1] = (p1 >> 8) | (p2 << 16);
    o[2] = (p2 >> 16) | (p3 << 8);
  }
}

// any other frame: one thread per pixel, byte loads, the three named channels of the destination view as byte stores
__global__ __launch_bounds__(256) void yuv_generic_kernel(unsigned long long* stamp, YuvView s, FrameView dv) {
  const KStamp kstamp_(stamp);
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (unsigned)s.w * (unsigned)s.h) return;
  const int y = (int)(g / (unsigned)s.w), x = (int)(g - (unsigned)y * s.w);
  const int Y = s.y[(size_t)y * s.ys + x];
  int d = 0, e = 0;
  if (s.u) {
    const size_t c = (size_t)(y >> s.sy) * s.uvs + (size_t)(x >> s.sx) * s.uvp;
    d = (int)s.u[c] - 128;
    e = (int)s.v[c] - 128;
  }
  const unsigned p = yuv_px(Y, d, e);
  unsigned char* o = dv.data + y * dv.row + x * dv.pix;
  o[dv.off[0]] = (unsigned char)(p & 0xffu);
  o[dv.off[1]] = (unsigned char)((p >> 8) & 0xffu);
  o[dv.off[2]] = (unsigned char)(p >> 16);
}

int yuv_layout(const YuvView& s, const FrameView& d) {
  const auto al = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
  if (!s.u || !s.v || s.sx != 1 || s.sy != 1 || s.w % 4 || s.h % 2) return YUV_GENERIC;
  if (!al(s.y, 4) || s.ys % 4) return YUV_GENERIC;
  if (d.pix != 3 || d.off[0] != 0 || d.off[1] != 1 || d.off[2] != 2 || !al(d.data, 4) || d.row % 4) return YUV_GENERIC;
  if (s.uvp == 1) return al(s.u, 2) && al(s.v, 2) && s.uvs % 2 == 0 ? YUV_420_PLANAR : YUV_GENERIC;
  if (s.uvp == 2 && s.uvs % 4 == 0) {
    if (s.v == s.u + 1 && al(s.u, 4)) return YUV_420_NV12;
    if (s.u == s.v + 1 && al(s.v, 4)) return YUV_420_NV21;
  }
  return YUV_GENERIC;
}

hipError_t launch_yuv_import(unsigned long long* stamp, const YuvView& s, const FrameView& d, int layout, hipStream_t stream) {
  const long n = layout == YUV_GENERIC ? (long)s.w * s.h : (long)(s.w / 4) * (s.h / 2);
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  switch (layout) {
    case YUV_420_PLANAR: hipLaunchKernelGGL((yuv420_block_kernel<YUV_420_PLANAR>), grid, block, 0, stream, stamp, s, d.data, d.row); break;
    case YUV_420_NV12: hipLaunchKernelGGL((yuv420_block_kernel<YUV_420_NV12>), grid, block, 0, stream, stamp, s, d.data, d.row); break;
    case YUV_420_NV21: hipLaunchKernelGGL((yuv420_block_kernel<YUV_420_NV21>), grid, block, 0, stream, stamp, s, d.data, d.row); break;
    default: hipLaunchKernelGGL(yuv_generic_kernel, grid, block, 0, stream, stamp, s, d); break;
  }
  return hipGetLastError();
}

}  // namespace rtp

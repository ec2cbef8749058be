// maps_export.hip — maps mode (rtp_set_maps_output): selected channels of one frame's part-confidence maps and PAFs, straight from
// the low-res maps into a pitched view in the requested element format.  The 55 MB fp32 resized map is never written.
//
// NET grid: per output value the arithmetic of resize_kernel (resize_block8, resize_math.h; this file is built with the same
// -ffp-contract=off, so the values are rtp_resize's bit for bit), in resize_kernel's layout: one thread owns an 8 x 8 output block
// offset by -4, whose full-size scale shares one 4 x 4 neighbourhood.  Because of that offset an 8-output row of a block starts
// 4 elements off an 8-element boundary, so it leaves as its two 4-output halves, each naturally aligned: 2 x 4 bytes (u8),
// 2 x 8 bytes (f16), 2 x 16 bytes (f32).  The first strip's left half and, with width % 8 == 4, the last strip's right half lie
// outside the map.  Where the destination does not allow that (a caller's view at an odd address or pitch, width % 4 != 0) every
// element leaves byte by byte; maps_export_wide chooses on the host.
// LOWRES grid: a gather of the chosen channels of every scale with the same conversion, one thread per element.
#include "kernels.h"
#include "resize_math.h"

namespace rtp {

namespace {

enum { FMT_F32 = 0, FMT_F16 = 1, FMT_U8 = 2 };

// rtp_maps_quantize_u8: no expression here can contract (a multiply feeds a max, an add feeds a multiply), rintf rounds half to even,
// fmaxf(NaN, 0) = 0
__device__ __forceinline__ unsigned quant_u8(float v, bool paf) {
  const float s = paf ? (v + 1.f) * 127.5f : v * 255.f;
  return (unsigned)rintf(fminf(fmaxf(s, 0.f), 255.f));
}
__device__ __forceinline__ unsigned f16_bits(float v) {
  const _Float16 h = (_Float16)v;   // v_cvt_f16_f32: round to nearest even, denormals kept
  return (unsigned)__builtin_bit_cast(unsigned short, h);
}

// 4 consecutive outputs of one row -> dst (the address of the first one)
template <int FMT, bool WIDE>
__device__ __forceinline__ void store4(unsigned char* dst, const float v[4], bool paf) {
  if (FMT == FMT_U8) {
    unsigned q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = quant_u8(v[i], paf);
    if (WIDE) {
      *reinterpret_cast<unsigned*>(dst) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) dst[i] = (unsigned char)q[i];
    }
  } else if (FMT == FMT_F16) {
    unsigned h[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = f16_bits(v[i]);
    if (WIDE) {
      *reinterpret_cast<uint2*>(dst) = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) { dst[2 * i] = (unsigned char)h[i]; dst[2 * i + 1] = (unsigned char)(h[i] >> 8); }
    }
  } else {
    if (WIDE) {
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned b = __float_as_uint(v[i]);
        dst[4 * i] = (unsigned char)b; dst[4 * i + 1] = (unsigned char)(b >> 8); dst[4 * i + 2] = (unsigned char)(b >> 16); dst[4 * i + 3] = (unsigned char)(b >> 24);
      }
    }
  }
}
// one output
template <int FMT, bool WIDE>
__device__ __forceinline__ void store1(unsigned char* dst, float v, bool paf) {
  if (FMT == FMT_U8) {
    dst[0] = (unsigned char)quant_u8(v, paf);
  } else if (FMT == FMT_F16) {
    const unsigned h = f16_bits(v);
    if (WIDE) *reinterpret_cast<unsigned short*>(dst) = (unsigned short)h;
    else { dst[0] = (unsigned char)h; dst[1] = (unsigned char)(h >> 8); }
  } else {
    const unsigned b = __float_as_uint(v);
    if (WIDE) *reinterpret_cast<unsigned*>(dst) = b;
    else { dst[0] = (unsigned char)b; dst[1] = (unsigned char)(b >> 8); dst[2] = (unsigned char)(b >> 16); dst[3] = (unsigned char)(b >> 24); }
  }
}

// resize_kernel's grid with blockIdx.z = the output plane
template <int FMT, bool WIDE>
__global__ __launch_bounds__(128) void maps_net_kernel(MapsParams p) {
  KStamp stamp_(p.stamp);
  const int k = blockIdx.x * blockDim.x + threadIdx.x;  // 8-wide column strip
  const int x0 = 8 * k - 4;
  const int y0 = 8 * (int)blockIdx.y - 4;
  const int tw = p.r.tw, th = p.r.th;
  if (x0 >= tw) return;
  const int c = p.chan[blockIdx.z];
  const bool paf = c > p.num_parts;
  constexpr int ELEM = FMT == FMT_U8 ? 1 : FMT == FMT_F16 ? 2 : 4;
  float sum[8][8];
  resize_block8(p.r, p.r.src + (long)c * p.r.h * p.r.w, x0, y0, sum);
  unsigned char* o = p.dst + (long)blockIdx.z * p.channel_stride;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int y = y0 + r;
    if (y < 0 || y >= th) continue;
    unsigned char* row = o + (long)y * p.row_stride;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int x = x0 + 4 * half;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = sum[r][4 * half + i] / p.r.num;
      if (WIDE) {   // tw % 4 == 0: a half lies inside the map or outside it as a whole
        if (x >= 0 && x < tw) store4<FMT, true>(row + (long)x * ELEM, v, paf);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (x + i >= 0 && x + i < tw) store1<FMT, false>(row + (long)(x + i) * ELEM, v[i], paf);
      }
    }
  }
}

// blockIdx.z = n * nch + k: channel chan[k] of scale n
template <int FMT, bool WIDE>
__global__ __launch_bounds__(256) void maps_lowres_kernel(MapsParams p) {
  KStamp stamp_(p.stamp);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int plane = p.r.h * p.r.w;
  if (i >= plane) return;
  const int n = (int)blockIdx.z / p.nch, c = p.chan[(int)blockIdx.z % p.nch];
  const int y = i / p.r.w, x = i - y * p.r.w;
  constexpr int ELEM = FMT == FMT_U8 ? 1 : FMT == FMT_F16 ? 2 : 4;
  const float v = p.r.src[((long)n * p.r.C + c) * plane + i];
  store1<FMT, WIDE>(p.dst + (long)blockIdx.z * p.channel_stride + (long)y * p.row_stride + (long)x * ELEM, v, c > p.num_parts);
}

template <int FMT, bool WIDE>
void launch_one(const MapsParams& p, hipStream_t stream) {
  if (p.grid == 0) {
    const int strips = (p.r.tw + 4 + 7) / 8;  // x0 = 8k-4 covers x in [-4, tw)
    const int bands = (p.r.th + 4 + 7) / 8;   // y0 = 8m-4
    hipLaunchKernelGGL((maps_net_kernel<FMT, WIDE>), dim3((strips + 127) / 128, bands, p.nch), dim3(128), 0, stream, p);
  } else {
    hipLaunchKernelGGL((maps_lowres_kernel<FMT, WIDE>), dim3((p.r.h * p.r.w + 255) / 256, 1, p.r.num * p.nch), dim3(256), 0, stream, p);
  }
}

}  // namespace

int maps_export_wide(int grid, int format, int width, const void* data, long channel_stride, long row_stride) {
  const long unit = (long)maps_elem_bytes(format) * (grid == 0 ? 4 : 1);
  if (grid == 0 && width % 4 != 0) return 0;
  return ((unsigned long long)(uintptr_t)data % unit == 0 && channel_stride % unit == 0 && row_stride % unit == 0) ? 1 : 0;
}

hipError_t launch_maps_export(const MapsParams& p, hipStream_t stream) {
  if (p.nch < 1 || p.nch > RTP_MAPS_MAX_CHANNELS || p.r.num < 1 || p.grid < 0 || p.grid > 1 || (long)p.r.num * p.nch > 65535) return hipErrorInvalidValue;
  switch (p.format * 2 + (p.wide ? 1 : 0)) {
    case 0: launch_one<FMT_F32, false>(p, stream); break;
    case 1: launch_one<FMT_F32, true>(p, stream); break;
    case 2: launch_one<FMT_F16, false>(p, stream); break;
    case 3: launch_one<FMT_F16, true>(p, stream); break;
    case 4: launch_one<FMT_U8, false>(p, stream); break;
    case 5: launch_one<FMT_U8, true>(p, stream); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace rtp

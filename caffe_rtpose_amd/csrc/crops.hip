// crops.hip — crops mode (rtp_set_crops_output): one box per person from the joints the connect kernels left in device memory, and the
// frame's display image resampled into fixed-size crops.  One launch per frame serves every person: grid (tiles of one crop,
// max_crops).  Every workgroup reads *num_people on the device (no host synchronisation; a negative value is connect's error code
// and counts as 0) and leaves at once when its slot is not a person's.  Otherwise its first wave derives the slot's box (a person
// has at most 70 parts: one or two list entries per lane, then a cross-lane min / max), hands it to the other waves through LDS,
// and tile 0 also writes the slot's box record.
//
// The arithmetic is rtp_crop_people's (host_util.cpp; include/rtpose_mi355x.h spells it out) bit for bit: the box in float32 with
// every operation rounded on its own (this file is built with -ffp-contract=off, like postproc.hip), everything past the four
// Q16 conversions in integers.  min and max of finite numbers do not depend on the order they are taken in (-0 was made +0), so the
// cross-lane tree gives the host loop's bits.
//
// The box values are made wave-uniform (readfirstlane) so that the sample loops run on scalar trip counts without divergence; taps
// outside the image are clamped to an address inside it and get weight 0 instead of a branch.  The source is read with direct
// byte loads (3-byte pixels at arbitrary positions); neighbouring outputs share taps through the caches.
// One pixel per thread, a workgroup tile = 256 consecutive pixels of the crop in row-major order.  Stores: wide = the tile's 768 bytes
// are laid out in LDS as they lie in memory and leave as 48 stores of 16 bytes per lane; otherwise three byte stores per thread.
// crops_wide chooses on the host.  (A first version gave a thread 16 consecutive pixels and three 16-byte stores of its own: the
// sample loops of 16 pixels in a row are one long chain of load latencies, 59 us against 5 us for one 128x128 crop;
// profiles/r12_crops.txt.)
#include "kernels.h"

namespace rtp {

namespace {

enum { LAYOUT_HWC_BGR = 0, LAYOUT_CHW_RGB = 1 };

struct CropBox {   // wave-uniform
  long long ox, oy, dx, dy;
  int lsx, lsy;    // log2 of the samples per axis (1, 2 or 4)
  int valid;
};

__device__ __forceinline__ long long uniform64(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ int log2_samples(long long step) { return step <= 98304 ? 0 : step <= 196608 ? 1 : 2; }

// One output pixel (i, j) of a slot with a box: the three channels in the display image's order (B, G, R)
__device__ __forceinline__ void crop_pixel(const unsigned char* __restrict__ src, int w, int h, const CropBox& b, int i, int j, unsigned v[3]) {
  const long long bx = b.ox + (long long)i * b.dx - 32768, by = b.oy + (long long)j * b.dy - 32768;
  const int Sx = 1 << b.lsx, Sy = 1 << b.lsy;
  unsigned long long T0 = 0, T1 = 0, T2 = 0;
  for (int sb = 0; sb < Sy; ++sb) {
    const long long py = by + (((long long)(2 * sb + 1) * b.dy) >> (b.lsy + 1));
    const int Y = (int)(py >> 16);
    const unsigned fy = (((unsigned)py & 65535u) + 16u) >> 5;
    const unsigned wy0 = (unsigned)Y < (unsigned)h ? 2048u - fy : 0u;
    const unsigned wy1 = (unsigned)(Y + 1) < (unsigned)h ? fy : 0u;
    const unsigned char* r0 = src + (long)min(max(Y, 0), h - 1) * w * 3;
    const unsigned char* r1 = src + (long)min(max(Y + 1, 0), h - 1) * w * 3;
    for (int sa = 0; sa < Sx; ++sa) {
      const long long px = bx + (((long long)(2 * sa + 1) * b.dx) >> (b.lsx + 1));
      const int X = (int)(px >> 16);
      const unsigned fx = (((unsigned)px & 65535u) + 16u) >> 5;
      const unsigned wx0 = (unsigned)X < (unsigned)w ? 2048u - fx : 0u;
      const unsigned wx1 = (unsigned)(X + 1) < (unsigned)w ? fx : 0u;
      const int c0 = 3 * min(max(X, 0), w - 1), c1 = 3 * min(max(X + 1, 0), w - 1);
      // (at most 2048 * 2048 * 255 per sample: 32 bits suffice; the sum over up to 16 samples needs 34)
      T0 += wy0 * (wx0 * r0[c0] + wx1 * r0[c1]) + wy1 * (wx0 * r1[c0] + wx1 * r1[c1]);
      T1 += wy0 * (wx0 * r0[c0 + 1] + wx1 * r0[c1 + 1]) + wy1 * (wx0 * r1[c0 + 1] + wx1 * r1[c1 + 1]);
      T2 += wy0 * (wx0 * r0[c0 + 2] + wx1 * r0[c1 + 2]) + wy1 * (wx0 * r1[c0 + 2] + wx1 * r1[c1 + 2]);
    }
  }
  const int sh = 22 + b.lsx + b.lsy;
  const unsigned long long half = 1ull << (sh - 1);
  v[0] = (unsigned)((T0 + half) >> sh);
  v[1] = (unsigned)((T1 + half) >> sh);
  v[2] = (unsigned)((T2 + half) >> sh);
}

template <bool WIDE, int LAYOUT>
__global__ __launch_bounds__(256) void crops_kernel(CropsParams p) {
  const int k = blockIdx.y;
  const int people = *p.num_people;
  const int n = min(max(people, 0), p.max_crops);
  if (k >= n) return;   // (the whole workgroup: in front of the barrier)
  __shared__ long long s_q[4];
  __shared__ int s_valid;
  if (threadIdx.x < 64) {
    const float* jp = p.joints + (long)k * p.num_parts * 3;
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    int count = 0;
    for (int i = threadIdx.x; i < p.nlist; i += 64) {
      const int part = p.list[i];
      const float x = jp[3 * part], y = jp[3 * part + 1], s = jp[3 * part + 2];
      if (s > p.min_score && __builtin_isfinite(x) && __builtin_isfinite(y)) {
        const float xz = x + 0.0f, yz = y + 0.0f;
        x0 = fminf(x0, xz); x1 = fmaxf(x1, xz); y0 = fminf(y0, yz); y1 = fmaxf(y1, yz);
        ++count;
      }
    }
    x0 = wave_min(x0); x1 = wave_max(x1); y0 = wave_min(y0); y1 = wave_max(y1);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) count += __shfl_xor(count, m, 64);
    // every lane holds the same five values: the box, in the header's order of operations
    bool valid = count >= p.min_parts;
    const float fcw = (float)p.crop_w, fch = (float)p.crop_h;
    const float sx = x0 + x1, sy = y0 + y1;
    const float cx = sx * 0.5f, cy = sy * 0.5f;
    float bw = x1 - x0, bh = y1 - y0;
    valid = valid && __builtin_isfinite(bw) && __builtin_isfinite(bh);
    const float gm = p.margin * fmaxf(bw, bh);
    const float g = gm * 2.0f;
    const float wg = bw + g, hg = bh + g;
    bw = fmaxf(wg, 1.0f); bh = fmaxf(hg, 1.0f);
    const float wn = bh * fcw;
    const float wa = wn / fch;
    if (wa > bw) bw = wa;
    else { const float hn = bw * fch; bh = hn / fcw; }
    const float hw = bw * 0.5f, hh = bh * 0.5f;
    const float left = cx - hw, top = cy - hh;
    const float right = left + bw, bottom = top + bh;
    const float lim = 1048576.0f;
    valid = valid && fabsf(left) <= lim && fabsf(top) <= lim && fabsf(right) <= lim && fabsf(bottom) <= lim;   // (a NaN fails)
    if (threadIdx.x == 0) {
      const float lq = left * 65536.0f, tq = top * 65536.0f;
      const float stx = bw / fcw, sty = bh / fch;
      const float dxq = stx * 65536.0f, dyq = sty * 65536.0f;
      s_q[0] = valid ? (long long)rintf(lq) : 0;
      s_q[1] = valid ? (long long)rintf(tq) : 0;
      s_q[2] = valid ? (long long)rintf(dxq) : 65536;
      s_q[3] = valid ? (long long)rintf(dyq) : 65536;
      s_valid = valid ? 1 : 0;
      if (blockIdx.x == 0 && p.boxes) {
        float* rec = p.boxes + (long)k * 6;
        rec[0] = valid ? left : 0.f; rec[1] = valid ? top : 0.f; rec[2] = valid ? bw : 0.f; rec[3] = valid ? bh : 0.f;
        rec[4] = (float)count; rec[5] = valid ? 1.f : 0.f;
      }
    }
  }
  if (!p.src || !p.dst) return;   // boxes only (kernel argument: the whole grid)
  __syncthreads();
  CropBox b;
  b.ox = uniform64(s_q[0]); b.oy = uniform64(s_q[1]); b.dx = uniform64(s_q[2]); b.dy = uniform64(s_q[3]);
  b.valid = __builtin_amdgcn_readfirstlane(s_valid);
  b.lsx = log2_samples(b.dx); b.lsy = log2_samples(b.dy);
  unsigned char* out = p.dst + (long)k * p.crop_stride;
  const int cw = p.crop_w, ch = p.crop_h;
  const int pixels = cw * ch;
  const int u0 = blockIdx.x * 256;                 // the tile: 256 consecutive pixels of the crop in row-major order
  const int u = u0 + threadIdx.x;
  unsigned v[3] = {0u, 0u, 0u};
  if (u < pixels && b.valid) {                     // (b.valid is wave-uniform)
    const int j = u / cw;
    crop_pixel(p.src, p.w, p.h, b, u - j * cw, j, v);
  }
  const long plane = (long)pixels;
  if (WIDE) {
    // The tile's bytes are laid out in LDS as they lie in memory (HWC: 768 consecutive bytes; CHW: 256 consecutive bytes of each
    // plane) and leave as 48 stores of 16 bytes.  pixels % 16 == 0, so a partial last tile holds whole 16-byte groups too.
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[768];
    const int t = threadIdx.x;
    if (LAYOUT == LAYOUT_HWC_BGR) {
      s_tile[3 * t] = (unsigned char)v[0]; s_tile[3 * t + 1] = (unsigned char)v[1]; s_tile[3 * t + 2] = (unsigned char)v[2];
    } else {
      s_tile[t] = (unsigned char)v[2]; s_tile[256 + t] = (unsigned char)v[1]; s_tile[512 + t] = (unsigned char)v[0];
    }
    __syncthreads();
    const int valid_px = min(256, pixels - u0);    // a multiple of 16
    if (t < 48) {
      if (LAYOUT == LAYOUT_HWC_BGR) {
        if (16 * t < 3 * valid_px) *reinterpret_cast<uint4*>(out + 3L * u0 + 16 * t) = *reinterpret_cast<const uint4*>(s_tile + 16 * t);
      } else {
        const int c = t >> 4, g = t & 15;          // plane, 16-byte group of the tile's 256 bytes in it
        if (16 * g < valid_px) *reinterpret_cast<uint4*>(out + c * plane + u0 + 16 * g) = *reinterpret_cast<const uint4*>(s_tile + 256 * c + 16 * g);
      }
    }
  } else {
    if (u >= pixels) return;
    if (LAYOUT == LAYOUT_HWC_BGR) {
      unsigned char* o = out + (long)u * 3;
      o[0] = (unsigned char)v[0]; o[1] = (unsigned char)v[1]; o[2] = (unsigned char)v[2];
    } else {
      out[u] = (unsigned char)v[2]; out[plane + u] = (unsigned char)v[1]; out[2 * plane + u] = (unsigned char)v[0];
    }
  }
}

template <bool WIDE, int LAYOUT>
void launch_one(const CropsParams& p, hipStream_t stream) {
  const long units = (long)p.crop_h * p.crop_w;
  const int tiles = (p.src && p.dst) ? (int)((units + 255) / 256) : 1;
  hipLaunchKernelGGL((crops_kernel<WIDE, LAYOUT>), dim3(tiles, p.max_crops), dim3(256), 0, stream, p);
}

}  // namespace

int crops_wide(int crop_w, const void* data, long crop_stride) {
  return (crop_w % 16 == 0 && (unsigned long long)(uintptr_t)data % 16 == 0 && crop_stride % 16 == 0) ? 1 : 0;
}

hipError_t launch_crops(const CropsParams& p, hipStream_t stream) {
  if (!p.joints || !p.num_people || p.nlist < 1 || p.nlist > RTP_CROPS_MAX_PARTS || p.num_parts < 1 || p.max_crops < 1 || p.max_crops > 65535 ||
      p.crop_w < 8 || p.crop_h < 8 || p.crop_w > 512 || p.crop_h > 512 || p.layout < 0 || p.layout > 1)
    return hipErrorInvalidValue;
  if (p.src && p.dst && (p.w < 1 || p.h < 1 || p.crop_stride < (long)p.crop_w * p.crop_h * 3)) return hipErrorInvalidValue;
  if (p.wide && !crops_wide(p.crop_w, p.dst, p.crop_stride)) return hipErrorInvalidValue;
  for (int i = 0; i < p.nlist; ++i)
    if (p.list[i] >= p.num_parts) return hipErrorInvalidValue;
  switch (p.layout * 2 + (p.wide ? 1 : 0)) {
    case 0: launch_one<false, LAYOUT_HWC_BGR>(p, stream); break;
    case 1: launch_one<true, LAYOUT_HWC_BGR>(p, stream); break;
    case 2: launch_one<false, LAYOUT_CHW_RGB>(p, stream); break;
    default: launch_one<true, LAYOUT_CHW_RGB>(p, stream); break;
  }
  return hipGetLastError();
}

}  // namespace rtp

// appearance.hip — appearance-aided tracking (rtp_set_track_appearance): one colour descriptor per person from the joints the connect
// kernels left in device memory and the frame's un-rendered display image.  One launch per frame serves every person: one workgroup of
// 256 threads per person slot.  Every workgroup reads *num_people on the device (no host synchronisation; a negative value is
// connect's error code and counts as 0) and leaves at once when its slot is not a person's.  Otherwise its first wave derives the
// person's box as crops.hip does (a person has at most 70 parts: one or two list entries per lane, then a cross-lane min / max) and
// hands the four Q16 values to the other waves through LDS; every thread then takes 4 of the 32 x 32 samples (thread t reads grid
// column t & 31 of the grid rows t >> 5, + 8, + 16 and + 24) into 128 LDS counters, and threads 0 .. 15 store the 128 uint16 as 16
// bytes each.  The kernel keeps no state.
//
// The arithmetic is rtp_appearance_describe's (host_util.cpp; include/rtpose_mi355x.h spells it out) bit for bit: the box in float32
// with every operation rounded on its own (this file is built with -ffp-contract=off, like crops.hip), everything past the four Q16
// conversions in integers.  min and max of finite numbers do not depend on the order they are taken in (-0 was made +0), and a
// histogram does not depend on the order of its increments.  Sample positions are clamped into the image (the border is replicated),
// so every load lies inside it.
#include "kernels.h"

namespace rtp {

namespace {

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

__global__ __launch_bounds__(256) void appear_describe_kernel(AppearDescribeParams p) {
  const int k = blockIdx.x;
  const int people = *p.num_people;
  const int n = min(max(people, 0), RTP_TRACK_MAX_PEOPLE);
  if (k >= n) return;   // (the whole workgroup: in front of the barrier)
  __shared__ long long s_q[4];
  __shared__ int s_valid;
  __shared__ __attribute__((aligned(16))) unsigned s_bins[RTP_APPEAR_BINS];
  __shared__ __attribute__((aligned(16))) unsigned short s_out[RTP_APPEAR_BINS];
  const int tid = threadIdx.x;
  if (tid < RTP_APPEAR_BINS) s_bins[tid] = 0u;
  if (tid < 64) {
    const float* jp = p.joints + (long)k * p.num_parts * 3;
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    int count = 0;
    for (int i = tid; i < p.nlist; i += 64) {
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
    bool valid = p.src != nullptr && count >= p.min_parts;
    const float sx = x0 + x1, sy = y0 + y1;
    const float cx = sx * 0.5f, cy = sy * 0.5f;
    float bw = x1 - x0, bh = y1 - y0;
    valid = valid && __builtin_isfinite(bw) && __builtin_isfinite(bh);
    const float gm = p.margin * fmaxf(bw, bh);
    const float g = gm * 2.0f;
    const float wg = bw + g, hg = bh + g;
    bw = fmaxf(wg, 1.0f); bh = fmaxf(hg, 1.0f);
    const float hw = bw * 0.5f, hh = bh * 0.5f;
    const float left = cx - hw, top = cy - hh;
    const float right = left + bw, bottom = top + bh;
    const float lim = 1048576.0f;
    valid = valid && fabsf(left) <= lim && fabsf(top) <= lim && fabsf(right) <= lim && fabsf(bottom) <= lim;   // (a NaN fails)
    if (tid == 0) {
      const float lq = left * 65536.0f, tq = top * 65536.0f;
      const float stx = bw / 32.0f, sty = bh / 32.0f;
      const float dxq = stx * 65536.0f, dyq = sty * 65536.0f;
      s_q[0] = valid ? (long long)rintf(lq) : 0;
      s_q[1] = valid ? (long long)rintf(tq) : 0;
      s_q[2] = valid ? (long long)rintf(dxq) : 0;
      s_q[3] = valid ? (long long)rintf(dyq) : 0;
      s_valid = valid ? 1 : 0;
    }
  }
  __syncthreads();
  const int valid = s_valid;
  if (valid) {   // (the same value in every thread)
    const long long ox = s_q[0], oy = s_q[1], dx = s_q[2], dy = s_q[3];
    const int i = tid & 31;
    const long long colq = (ox + (long long)i * dx + (dx >> 1)) >> 16;   // dx >= 0: / 2 is the shift
    const int col = (int)min(max(colq, 0ll), (long long)(p.w - 1));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = (tid >> 5) + 8 * r;
      const long long rowq = (oy + (long long)j * dy + (dy >> 1)) >> 16;
      const int row = (int)min(max(rowq, 0ll), (long long)(p.h - 1));
      const unsigned char* px = p.src + ((long)row * p.w + col) * 3;
      const unsigned b = px[0], g = px[1], rr = px[2];
      atomicAdd(&s_bins[(j >= 16 ? 64u : 0u) + (rr >> 6) * 16u + (g >> 6) * 4u + (b >> 6)], 1u);
    }
  }
  __syncthreads();
  if (tid < RTP_APPEAR_BINS) s_out[tid] = (unsigned short)s_bins[tid];   // (zeros where the person has no descriptor)
  __syncthreads();
  if (tid < 16) reinterpret_cast<uint4*>(p.bins + (long)k * RTP_APPEAR_BINS)[tid] = reinterpret_cast<const uint4*>(s_out)[tid];
  if (tid == 0) p.valid[k] = (unsigned char)valid;
}

}  // namespace

hipError_t launch_appear_describe(const AppearDescribeParams& p, hipStream_t stream) {
  if (!p.joints || !p.num_people || !p.bins || !p.valid || p.nlist < 1 || p.nlist > RTP_TRACK_MAX_PARTS || p.num_parts < 1 || p.num_parts > RTP_TRACK_MAX_PARTS ||
      p.min_parts < 1 || (unsigned long long)(uintptr_t)p.bins % 16 != 0)
    return hipErrorInvalidValue;
  if (p.src && (p.w < 1 || p.h < 1 || p.w > 32768 || p.h > 32768)) return hipErrorInvalidValue;
  for (int i = 0; i < p.nlist; ++i)
    if (p.list[i] >= p.num_parts) return hipErrorInvalidValue;
  hipLaunchKernelGGL(appear_describe_kernel, dim3(RTP_TRACK_MAX_PEOPLE), dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace rtp

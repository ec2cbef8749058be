// redact.hip — redaction mode (rtp_set_redaction): people's heads mosaicked, blurred or filled in the rendered frame.  Two kernels.
//
// redact_regions_kernel: ONE workgroup behind the kernels that produce the joints the frame is rendered with.  It reads *num_people
// (no host synchronisation; a negative value is connect's error code and counts as 0) and the joints; one thread per person writes
// the person's record {cx, cy, rx, ry, count, valid}, thread 0 writes n behind the records' room.
//
// redact_apply_kernel: one workgroup of 256 threads per tile of 32 x 32 pixels, FOUR PIXELS OF ONE ROW per thread: 12 consecutive
// bytes, which leave as three 4-byte stores where all four are covered and the row address is a multiple of 4, byte by byte
// otherwise (any stride and any address work).  Every thread tests ONE region's bounding box against the tile and the hits go
// into an LDS list by an LDS atomic counter: at most 96, so the list always fits, and the result does not depend on their order.  A
// tile that no region touches returns there: it has read the region list and nothing else.  Otherwise every thread computes which of
// its pixels are covered (the ellipse test in int64) and the effect's value for them:
//   FILL    the colour.
//   MOSAIC  32 is a multiple of every allowed cell, so a tile holds whole cells and a cell's pixels are read by exactly ONE
//           workgroup: each thread loads its four pixels and adds them to its cell's sums in LDS (integer atomics: exact in any
//           order), a barrier, one thread per (cell, channel) divides, a barrier, and only then the first store.  In place.
//   BLUR    reads a halo of `radius` pixels that NEIGHBOURING workgroups write, so it is NOT computed in place.  Built: TWO LAUNCHES
//           and a scratch image of the display size per frame slot (allocated when the mode is switched on).  Pass 0 loads the tile
//           with its halo into LDS ((32 + 32)^2 x 3 B = 12 KiB at radius 16, zeros outside the image), builds horizontal window sums
//           with one running sum per (row, channel), sums them vertically per covered pixel and stores the value to the SCRATCH
//           image; pass 1 culls and tests again and copies the covered pixels back.  Chosen over a snapshot of the touched tiles
//           because it needs no list of tiles, no second cull result kept in memory between the launches and no device-side
//           allocation: the second launch is the first one's skeleton with a copy in the middle, and a launch boundary is the
//           only grid-wide barrier there is.
// LDS: 12.3 KiB pixels + 12.3 KiB row sums + 3 KiB cell sums + the list = 29 KiB per workgroup, five workgroups per CU by LDS; the
// kernel takes 34 VGPRs and no scratch memory, so registers allow more waves than that and LDS is what bounds the occupancy.  Rows of both LDS arrays are padded to an ODD number
// of dwords (49): the running sums walk 64 rows at once and the vertical sums 8, and with the natural pitch of 48 dwords those rows
// would share 4 banks.
//
// The divisions (sum + (cnt >> 1)) / cnt are plain unsigned 32-bit divisions, exact for every cnt, clipped cells and windows
// included: one per cell and channel for the mosaic, three per covered pixel for the blur, behind 33 LDS reads per channel.  No
// multiply-shift is used, so there is nothing to prove.
//
// Everything from the first rounding on is integer arithmetic, so the bytes are rtp_redact_apply's (host_util.cpp;
// include/rtpose_mi355x.h spells both definitions out).  Built with -ffp-contract=off like overlay.hip: the one float operation,
// v + 0.5f in front of floorf, is a single rounded addition.  Records and pixels are written with ordinary vector stores.
#include "kernels.h"

#include <cstdint>

namespace rtp {

namespace {

constexpr int kPeople = RTP_TRACK_MAX_PEOPLE, kInts = RTP_RDC_REGION_INTS, kMaxRadius = RTP_RDC_MAX_RADIUS;
constexpr int kRegionThreads = 128, kThreads = 256;
constexpr int kTile = RTP_RDC_TILE, kHalo = RTP_RDC_MAX_BLUR, kSpan = kTile + 2 * kHalo;
constexpr int kPxPitch = ((kSpan * 3 + 3) / 4 | 1) * 4;   // bytes per LDS row of pixels: 49 dwords
constexpr int kSumPitch = (kTile * 3 / 2 | 1) * 2;        // ushorts per LDS row of sums: 49 dwords
constexpr int kMaxCells = (kTile / 2) * (kTile / 2);      // cell 2
static_assert(kRegionThreads >= kPeople && kThreads >= kPeople, "one thread per person / per region");
static_assert(kThreads * 4 == kTile * kTile && kTile == 32, "four pixels of one row per thread, eight threads per row");
static_assert(kSpan * 3 <= kThreads, "one running sum per (row, channel)");
static_assert((2 * kHalo + 1) * 255 <= 65535, "a row sum fits 16 bits");

__device__ __forceinline__ int round_px(float v) {
  v = v < -32767.0f ? -32767.0f : v > 32767.0f ? 32767.0f : v;
  return (int)floorf(v + 0.5f);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__global__ __launch_bounds__(kRegionThreads) void redact_regions_kernel(RedactRegionsParams p) {
  const int tid = threadIdx.x;
  const int n = min(max(*p.num_people, 0), kPeople);
  if (tid == 0) *p.num_regions = n;
  if (tid >= n) return;
  const float* j = p.joints + (size_t)tid * p.num_parts * 3;
  float fx0 = 0.f, fx1 = 0.f, fy0 = 0.f, fy1 = 0.f;
  int c = 0;
  for (int i = 0; i < p.nlist; ++i) {
    const int q = p.list[i];
    const float x = j[3 * q], y = j[3 * q + 1], s = j[3 * q + 2];
    if (!(s > p.min_score) || !__builtin_isfinite(x) || !__builtin_isfinite(y)) continue;
    if (c++ == 0) { fx0 = fx1 = x; fy0 = fy1 = y; continue; }
    if (x < fx0) fx0 = x;
    if (x > fx1) fx1 = x;
    if (y < fy0) fy0 = y;
    if (y > fy1) fy1 = y;
  }
  int* rec = p.regions + tid * kInts;
  if (c < p.min_parts) {
    rec[0] = 0; rec[1] = 0; rec[2] = 0; rec[3] = 0; rec[4] = c; rec[5] = 0;
    return;
  }
  const int x0 = round_px(fx0), x1 = round_px(fx1), y0 = round_px(fy0), y1 = round_px(fy1);
  const int s = max(x1 - x0, y1 - y0) + 1;   // 1 .. 65535: s * scale_q8 < 2^28
  const int rx = clampi(((s * p.scale_q8) >> 9) + p.pad, p.min_radius, kMaxRadius);
  const int ry = min((rx * p.aspect_q8) >> 8, kMaxRadius);
  rec[0] = (x0 + x1) >> 1; rec[1] = (y0 + y1) >> 1; rec[2] = rx; rec[3] = ry; rec[4] = c; rec[5] = 1;
}

// copy == 0: the effect's values from p.image to dst; copy != 0: the covered pixels from p.scratch to p.image
__global__ __launch_bounds__(kThreads) void redact_apply_kernel(RedactApplyParams p, unsigned char* dst, int copy) {
  __shared__ int s_reg[kPeople][4];
  __shared__ int s_count;
  __shared__ unsigned s_cell[kMaxCells * 3];
  __shared__ unsigned char s_px[kSpan * kPxPitch];
  __shared__ unsigned short s_sum[kSpan * kSumPitch];
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
  const int tx1 = min(tx0 + kTile, p.w) - 1, ty1 = min(ty0 + kTile, p.h) - 1;   // the tile inside the image, inclusive
  if (tid == 0) s_count = 0;
  __syncthreads();
  const int n = min(max(*p.num_regions, 0), kPeople);
  if (tid < n) {
    const int* r = p.regions + tid * kInts;
    if (r[5] != 0) {
      const int cx = clampi(r[0], -65535, 65535), cy = clampi(r[1], -65535, 65535), rx = clampi(r[2], 0, kMaxRadius), ry = clampi(r[3], 0, kMaxRadius);
      if (cx - rx <= tx1 && cx + rx >= tx0 && cy - ry <= ty1 && cy + ry >= ty0) {
        int* d = s_reg[atomicAdd(&s_count, 1)];
        d[0] = cx; d[1] = cy; d[2] = rx; d[3] = ry;
      }
    }
  }
  __syncthreads();
  const int count = s_count;
  if (count == 0) return;   // (the whole workgroup: nothing but the region list was read)

  const int lx = (tid & 7) * 4, ly = tid >> 3;   // the thread's four pixels inside the tile: (lx .. lx + 3, ly)
  const int qx = tx0 + lx, py = ty0 + ly;
  unsigned mask = 0;   // bit k: pixel qx + k is inside the image and covered
  if (py < p.h) {
    for (int s = 0; s < count; ++s) {
      const int cx = s_reg[s][0], cy = s_reg[s][1], rx = s_reg[s][2], ry = s_reg[s][3];
      const int dy = py - cy;
      if (dy < -ry || dy > ry) continue;
      const long long ey = (long long)dy * rx, lim = (long long)rx * ry * ((long long)rx * ry);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int px = qx + k, dx = px - cx;
        if (px >= p.w || dx < -rx || dx > rx) continue;
        const long long ex = (long long)dx * ry;
        if (!p.ellipse || ex * ex + ey * ey <= lim) mask |= 1u << k;
      }
    }
  }

  unsigned char val[4][3] = {};
  const size_t off = (size_t)py * p.stride + (size_t)qx * 3;   // (only dereferenced for pixels inside the image)
  if (copy) {
    const unsigned char* src = p.scratch + off;
    if (mask == 15u && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
      const unsigned* s4 = reinterpret_cast<const unsigned*>(src);
      const unsigned a = s4[0], b = s4[1], c = s4[2];
      val[0][0] = a & 255; val[0][1] = (a >> 8) & 255; val[0][2] = (a >> 16) & 255; val[1][0] = a >> 24;
      val[1][1] = b & 255; val[1][2] = (b >> 8) & 255; val[2][0] = (b >> 16) & 255; val[2][1] = b >> 24;
      val[2][2] = c & 255; val[3][0] = (c >> 8) & 255; val[3][1] = (c >> 16) & 255; val[3][2] = c >> 24;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (mask & (1u << k)) { val[k][0] = src[3 * k]; val[k][1] = src[3 * k + 1]; val[k][2] = src[3 * k + 2]; }
    }
  } else if (p.effect == RTP_RDC_FILL) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { val[k][0] = p.colour & 255; val[k][1] = (p.colour >> 8) & 255; val[k][2] = (p.colour >> 16) & 255; }
  } else if (p.effect == RTP_RDC_MOSAIC) {
    const int cell = p.cell, per_side = kTile / cell, cells = per_side * per_side;
    for (int i = tid; i < cells * 3; i += kThreads) s_cell[i] = 0u;
    __syncthreads();
    // the thread's pixels into their cells' sums: one flush per cell (cell >= 4: all four pixels share one)
    if (py < p.h) {
      const unsigned char* src = p.image + off;
      const int crow = (ly / cell) * per_side;
      unsigned acc[3] = {0u, 0u, 0u};
      int cur = -1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (qx + k >= p.w) break;
        const int ci = crow + (lx + k) / cell;
        if (ci != cur && cur >= 0) {
          atomicAdd(&s_cell[cur * 3], acc[0]); atomicAdd(&s_cell[cur * 3 + 1], acc[1]); atomicAdd(&s_cell[cur * 3 + 2], acc[2]);
          acc[0] = acc[1] = acc[2] = 0u;
        }
        cur = ci;
        acc[0] += src[3 * k]; acc[1] += src[3 * k + 1]; acc[2] += src[3 * k + 2];
      }
      if (cur >= 0) { atomicAdd(&s_cell[cur * 3], acc[0]); atomicAdd(&s_cell[cur * 3 + 1], acc[1]); atomicAdd(&s_cell[cur * 3 + 2], acc[2]); }
    }
    __syncthreads();   // every pixel of the tile has been read: the sums are complete, and stores may follow
    for (int i = tid; i < cells * 3; i += kThreads) {
      const int ci = i / 3, x0 = tx0 + (ci % per_side) * cell, y0 = ty0 + (ci / per_side) * cell;
      const int cw = min(x0 + cell, p.w) - x0, ch = min(y0 + cell, p.h) - y0;
      if (cw > 0 && ch > 0) {
        const unsigned cnt = (unsigned)(cw * ch);
        s_cell[i] = (s_cell[i] + (cnt >> 1)) / cnt;
      }
    }
    __syncthreads();
    const int crow = (ly / cell) * per_side;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned* v = &s_cell[(crow + (lx + k) / cell) * 3];
      val[k][0] = (unsigned char)v[0]; val[k][1] = (unsigned char)v[1]; val[k][2] = (unsigned char)v[2];
    }
  } else {   // RTP_RDC_BLUR
    const int r = p.radius, span = kTile + 2 * r;
    for (int i = tid; i < span * span; i += kThreads) {
      const int yy = i / span, xx = i - yy * span, gx = tx0 - r + xx, gy = ty0 - r + yy;
      unsigned char b = 0, g = 0, c = 0;
      if (gx >= 0 && gx < p.w && gy >= 0 && gy < p.h) {
        const unsigned char* src = p.image + (size_t)gy * p.stride + (size_t)gx * 3;
        b = src[0]; g = src[1]; c = src[2];
      }
      unsigned char* d = &s_px[yy * kPxPitch + xx * 3];
      d[0] = b; d[1] = g; d[2] = c;
    }
    __syncthreads();
    if (tid < span * 3) {   // s_sum[yy][xo][c] = the sum over the window's 2 r + 1 columns around tile column xo
      const int yy = tid / 3, c = tid - yy * 3;
      const unsigned char* row = &s_px[yy * kPxPitch + c];
      unsigned short* out = &s_sum[yy * kSumPitch + c];
      unsigned run = 0;
      for (int xx = 0; xx <= 2 * r; ++xx) run += row[3 * xx];
      out[0] = (unsigned short)run;
      for (int xo = 1; xo < kTile; ++xo) {
        run += row[3 * (xo + 2 * r)];
        run -= row[3 * (xo - 1)];
        out[3 * xo] = (unsigned short)run;
      }
    }
    __syncthreads();
    if (mask) {
      const int ch = min(py + r, p.h - 1) - max(py - r, 0) + 1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(mask & (1u << k))) continue;
        const int px = qx + k;
        const unsigned cnt = (unsigned)((min(px + r, p.w - 1) - max(px - r, 0) + 1) * ch);
        unsigned sum[3] = {0u, 0u, 0u};
        const unsigned short* col = &s_sum[ly * kSumPitch + (lx + k) * 3];
        for (int yy = 0; yy <= 2 * r; ++yy, col += kSumPitch) { sum[0] += col[0]; sum[1] += col[1]; sum[2] += col[2]; }
        val[k][0] = (unsigned char)((sum[0] + (cnt >> 1)) / cnt);
        val[k][1] = (unsigned char)((sum[1] + (cnt >> 1)) / cnt);
        val[k][2] = (unsigned char)((sum[2] + (cnt >> 1)) / cnt);
      }
    }
  }

  if (!mask) return;
  unsigned char* out = dst + off;
  if (mask == 15u && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
    unsigned* o4 = reinterpret_cast<unsigned*>(out);
    o4[0] = val[0][0] | val[0][1] << 8 | val[0][2] << 16 | (unsigned)val[1][0] << 24;
    o4[1] = val[1][1] | val[1][2] << 8 | val[2][0] << 16 | (unsigned)val[2][1] << 24;
    o4[2] = val[2][2] | val[3][0] << 8 | val[3][1] << 16 | (unsigned)val[3][2] << 24;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (mask & (1u << k)) { out[3 * k] = val[k][0]; out[3 * k + 1] = val[k][1]; out[3 * k + 2] = val[k][2]; }
}

}  // namespace

hipError_t launch_redact_regions(const RedactRegionsParams& p, hipStream_t stream) {
  if (!p.joints || !p.num_people || !p.regions || !p.num_regions || p.num_parts < 1 || p.num_parts > RTP_TRACK_MAX_PARTS || p.nlist < 1 || p.nlist > RTP_TRACK_MAX_PARTS ||
      p.min_parts < 1 || !(p.min_score >= 0.f) || p.scale_q8 < 64 || p.scale_q8 > 4096 || p.aspect_q8 < 64 || p.aspect_q8 > 1024 || p.pad < 0 || p.pad > 256 ||
      p.min_radius < 0 || p.min_radius > 256)
    return hipErrorInvalidValue;
  for (int i = 0; i < p.nlist; ++i)
    if (p.list[i] >= p.num_parts) return hipErrorInvalidValue;
  hipLaunchKernelGGL(redact_regions_kernel, dim3(1), dim3(kRegionThreads), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_redact_apply(const RedactApplyParams& p, hipStream_t stream) {
  const bool blur = p.effect == RTP_RDC_BLUR;
  if (!p.regions || !p.num_regions || !p.image || p.w < 1 || p.h < 1 || p.w > 32768 || p.h > 32768 || p.stride < 3L * p.w ||
      (p.effect != RTP_RDC_MOSAIC && !blur && p.effect != RTP_RDC_FILL) || (p.cell != 2 && p.cell != 4 && p.cell != 8 && p.cell != 16 && p.cell != 32) || p.radius < 1 ||
      p.radius > RTP_RDC_MAX_BLUR || (blur && (!p.scratch || p.scratch == p.image)))
    return hipErrorInvalidValue;
  const dim3 grid((p.w + kTile - 1) / kTile, (p.h + kTile - 1) / kTile);
  hipLaunchKernelGGL(redact_apply_kernel, grid, dim3(kThreads), 0, stream, p, blur ? p.scratch : p.image, 0);
  if (blur) hipLaunchKernelGGL(redact_apply_kernel, grid, dim3(kThreads), 0, stream, p, p.image, 1);
  return hipGetLastError();
}

}  // namespace rtp

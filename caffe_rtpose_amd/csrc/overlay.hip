// overlay.hip — overlay mode (rtp_set_track_overlay): tracked people drawn into the rendered frame.  Two kernels per frame.
//
// overlay_update_kernel: ONE workgroup behind the frame's track (and smooth) kernel.  It reads *num_people (no host synchronisation; a
// negative value is connect's error code and counts as 0), the joints and the frame's records, advances the engine's trail table (one
// ring of anchor points per track slot; launches of consecutive frames are ordered by the engine, an event behind each) and writes the
// frame's draw list and its length.  One thread per person computes the box and pushes the anchor into the person's own ring (a
// record names each slot at most once); a prefix sum over the people's item counts gives every person its place in the list, which
// is therefore in person order, as rtp_overlay_update's; then the workgroup's threads write the items, one (person, item) each.
// Where the kernel and the host definition part: rtp_overlay_update REFUSES two records with id != 0 that name one slot, and a slot
// outside the table; the kernel cannot refuse.  A slot outside the table is handled as an untracked person (nothing outside the table
// is addressed).  Two records on one slot would make two threads race on one ring (inside the table, but with no defined result):
// the track kernel's records name each slot at most once, which is what this kernel relies on.
//
// overlay_draw_kernel: one workgroup of 256 threads per tile of 32 x 16 pixels of the image, two pixels (rows y and y + 8) per thread.
// The list is walked 256 items at a time.  Every thread tests ONE item's bounding box against the tile; a wave ballot plus a prefix
// count over the four waves' hit counts place the hits in an LDS list IN ITEM ORDER (atomics would scramble it, and the blends do not
// commute).  The LDS list holds 512 items: when the next 256 candidates might not fit behind what it holds, and after the last pass,
// every thread blends its two pixels through the list in order and the list starts again — so a tile crossed by all 3168 items of a
// full frame is drawn in several rounds, still in item order.  Pixels are loaded at the first round that has items and stored at the
// end where they changed: a tile that no item touches costs the bounding-box tests and no pixel traffic.
//
// Everything from the first rounding on is integer arithmetic (the capsule test in int64), so the bytes are rtp_overlay_draw's
// (host_util.cpp; include/rtpose_mi355x.h spells both definitions out).  Built with -ffp-contract=off like render.hip: the one float
// operation, v + 0.5f in front of floorf, is a single rounded addition.  Table, list and pixels are written with ordinary vector stores.
#include "kernels.h"

namespace rtp {

namespace {

constexpr int kSlots = RTP_TRACK_SLOTS, kPeople = RTP_TRACK_MAX_PEOPLE, kRing = RTP_OVL_TRAIL_MAX, kInts = RTP_OVL_ITEM_INTS;
constexpr int kPerPerson = kRing + 1;   // at most kRing - 1 capsules, the box and the label
constexpr int kKindCapsule = 1, kKindRect = 2, kKindLabel = 3;
constexpr unsigned kBox = 1u, kLabel = 2u, kTrail = 4u;
constexpr int kThreads = 256;

__device__ __forceinline__ int round_px(float v) {
  v = v < -32767.0f ? -32767.0f : v > 32767.0f ? 32767.0f : v;
  return (int)floorf(v + 0.5f);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ int digits_of(unsigned v) {
  int d = 1;
  while (v >= 10u) { v /= 10u; ++d; }
  return d;
}

__global__ __launch_bounds__(kThreads) void overlay_update_kernel(OverlayUpdateParams p) {
  __shared__ int s_cnt[kPeople], s_off[kPeople + 1], s_box[kPeople][4];
  TrailTable* tb = p.table;
  const int tid = threadIdx.x;
  const int P = p.num_parts;
  const int people = *p.num_people;
  const int n = min(max(people, 0), kPeople);
  unsigned now = tb->frames + 1u;
  if (now == 0u) now = 1u;
  __syncthreads();   // every thread has read the old `frames`
  if (tid == 0) tb->frames = now;
  if (tid < kPeople) {
    int cnt = 0;
    const int id = tid < n ? p.recs[4 * tid] : 0, t = tid < n ? p.recs[4 * tid + 1] : -1;
    if (id != 0 && t >= 0 && t < kSlots) {
      const float* j = p.joints + (size_t)tid * P * 3;
      float fx0 = 0.f, fx1 = 0.f, fy0 = 0.f, fy1 = 0.f;
      bool any = false;
      for (int q = 0; q < P; ++q) {
        const float x = j[3 * q], y = j[3 * q + 1], s = j[3 * q + 2];
        if (!(s > p.min_score) || !__builtin_isfinite(x) || !__builtin_isfinite(y)) continue;
        if (!any) { fx0 = fx1 = x; fy0 = fy1 = y; any = true; continue; }
        if (x < fx0) fx0 = x;
        if (x > fx1) fx1 = x;
        if (y < fy0) fy0 = y;
        if (y > fy1) fy1 = y;
      }
      if (any) {
        const int x0 = round_px(fx0) - p.box_margin, y0 = round_px(fy0) - p.box_margin;
        const int x1 = round_px(fx1) + p.box_margin, y1 = round_px(fy1) + p.box_margin;
        s_box[tid][0] = x0; s_box[tid][1] = y0; s_box[tid][2] = x1; s_box[tid][3] = y1;
        TrailSlot* S = &tb->slot[t];
        int count = clampi(S->count, 0, kRing), head = S->head & (kRing - 1);   // (a table from rtp_overlay_set_state is in range)
        if (S->owner != id) { S->owner = id; count = 0; head = 0; }
        S->pts[head][0] = (x0 + x1) >> 1;
        S->pts[head][1] = (y0 + y1) >> 1;
        S->head = (head + 1) & (kRing - 1);
        count = min(count + 1, p.trail_len);
        S->count = count;
        cnt = ((p.what & kTrail) ? max(count - 1, 0) : 0) + ((p.what & kBox) ? 1 : 0) + ((p.what & kLabel) ? 1 : 0);
      }
    }
    s_cnt[tid] = cnt;
  }
  __syncthreads();   // the counts, the boxes and the rings (global stores of this workgroup) are visible
  if (tid < kPeople) {
    int off = 0;
    for (int i = 0; i < tid; ++i) off += s_cnt[i];
    s_off[tid] = off;
    if (tid == kPeople - 1) s_off[kPeople] = off + s_cnt[tid];
  }
  __syncthreads();
  if (tid == 0) *p.num_items = s_off[kPeople];
  for (int idx = tid; idx < n * kPerPerson; idx += kThreads) {
    const int k = idx / kPerPerson, j = idx - k * kPerPerson;
    if (j >= s_cnt[k]) continue;
    const int id = p.recs[4 * k];
    const TrailSlot* S = &tb->slot[p.recs[4 * k + 1]];   // (s_cnt[k] > 0: the slot is inside the table)
    const int count = S->count, head = S->head;
    const int m = (p.what & kTrail) ? max(count - 1, 0) : 0;
    const int colour = p.palette[id & 15];
    int* it = p.items + (size_t)(s_off[k] + j) * kInts;
    if (j < m) {
      const int* a = S->pts[(head - count + j + kRing) & (kRing - 1)];
      const int* b = S->pts[(head - count + j + 1 + kRing) & (kRing - 1)];
      it[0] = kKindCapsule; it[1] = a[0]; it[2] = a[1]; it[3] = b[0]; it[4] = b[1]; it[5] = p.trail_radius; it[6] = colour;
      it[7] = p.alpha * (j + 1) / m; it[8] = 0;
    } else if (j == m && (p.what & kBox)) {
      it[0] = kKindRect; it[1] = s_box[k][0]; it[2] = s_box[k][1]; it[3] = s_box[k][2]; it[4] = s_box[k][3]; it[5] = p.line_width; it[6] = colour;
      it[7] = p.alpha; it[8] = 0;
    } else {
      const int lw = (6 * digits_of((unsigned)id) + 1) * p.label_scale, lh = 9 * p.label_scale;
      const int x0 = s_box[k][0], y0 = s_box[k][1];
      const int ly = y0 - lh < 0 ? y0 : y0 - lh;
      it[0] = kKindLabel; it[1] = x0; it[2] = ly; it[3] = x0 + lw - 1; it[4] = ly + lh - 1; it[5] = p.label_scale; it[6] = colour;
      it[7] = p.alpha; it[8] = id;
    }
  }
}

constexpr int kTileW = RTP_OVL_TILE_W, kTileH = RTP_OVL_TILE_H;
constexpr int kList = 2 * kThreads;   // the LDS list: a pass adds at most kThreads items
static_assert(kTileW * kTileH == 2 * kThreads && kThreads == 256, "two pixels per thread, four waves");

// 0: the (clamped) item does not cover (px, py); 1: with its colour; 2: with the text colour
__device__ __forceinline__ int covers(const int* it, const OverlayDrawParams& p, int px, int py) {
  const int kind = it[0], x0 = it[1], y0 = it[2], x1 = it[3], y1 = it[4], size = it[5];
  if (kind == kKindRect) {
    if (px < x0 || px > x1 || py < y0 || py > y1) return 0;
    return px - x0 < size || x1 - px < size || py - y0 < size || y1 - py < size;
  }
  if (kind == kKindCapsule) {
    const long long dx = (long long)x1 - x0, dy = (long long)y1 - y0, ux = (long long)px - x0, uy = (long long)py - y0, r2 = (long long)size * size;
    const long long L = dx * dx + dy * dy, t = ux * dx + uy * dy;
    if (L == 0 || t < 0) return ux * ux + uy * uy <= r2;
    if (t > L) { const long long vx = (long long)px - x1, vy = (long long)py - y1; return vx * vx + vy * vy <= r2; }
    long long cross = ux * dy - uy * dx;
    if (cross < 0) cross = -cross;
    if (cross > (1LL << 31)) cross = 1LL << 31;
    return cross * cross <= r2 * L;
  }
  // (the list holds no other kind but the label)
  if (px < x0 || px > x1 || py < y0 || py > y1) return 0;
  const int u = (px - x0) / size, v = (py - y0) / size;
  if (v < 1 || v > 7 || u < 1) return 1;
  const int c = (u - 1) % 6, i = (u - 1) / 6;
  const unsigned value = (unsigned)it[8];
  const int ndig = digits_of(value);
  if (c >= 5 || i >= ndig) return 1;
  unsigned q = value;
  for (int d = ndig - 1; d > i; --d) q /= 10u;
  return (p.font[q % 10u][v - 1] >> (4 - c)) & 1 ? 2 : 1;
}

__device__ __forceinline__ void blend(int c, const int* it, int& b, int& g, int& r) {
  const int col = it[6], a = it[7];
  int cb = col & 255, cg = (col >> 8) & 255, cr = (col >> 16) & 255;
  if (c == 2) cb = cg = cr = ((29 * cb + 150 * cg + 77 * cr) >> 8) >= 128 ? 0 : 255;
  b = (b * (256 - a) + cb * a + 128) >> 8;
  g = (g * (256 - a) + cg * a + 128) >> 8;
  r = (r * (256 - a) + cr * a + 128) >> 8;
}

__global__ __launch_bounds__(kThreads) void overlay_draw_kernel(OverlayDrawParams p) {
  __shared__ int s_item[kList][kInts];
  __shared__ int s_wave[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int tx1 = min(tx0 + kTileW, p.w) - 1, ty1 = min(ty0 + kTileH, p.h) - 1;   // the tile inside the image, inclusive
  const int px = tx0 + (tid & (kTileW - 1)), pya = ty0 + tid / kTileW, pyb = pya + kTileH / 2;
  const bool ina = px < p.w && pya < p.h, inb = px < p.w && pyb < p.h;
  unsigned char* qa = p.image + (size_t)pya * p.stride + (size_t)px * 3;
  unsigned char* qb = p.image + (size_t)pyb * p.stride + (size_t)px * 3;
  const int n = min(max(*p.num_items, 0), RTP_OVL_MAX_ITEMS);
  int count = 0;   // items in the LDS list (the same in every thread)
  bool loaded = false, dirty_a = false, dirty_b = false;
  int ba = 0, ga = 0, ra = 0, bb = 0, gb = 0, rb = 0;
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + tid;
    int it[kInts];
    bool hit = false;
    if (i < n) {
      const int* src = p.items + (size_t)i * kInts;
#pragma unroll
      for (int q = 0; q < kInts; ++q) it[q] = src[q];
      const int kind = it[0];
      if (kind == kKindCapsule || kind == kKindRect || kind == kKindLabel) {
#pragma unroll
        for (int q = 1; q <= 4; ++q) it[q] = clampi(it[q], -65535, 65535);
        it[5] = kind == kKindLabel ? clampi(it[5], 1, 8) : clampi(it[5], 0, 16);
        it[7] = clampi(it[7], 0, 256);
        const int grow = kind == kKindCapsule ? it[5] : 0;
        hit = min(it[1], it[3]) - grow <= tx1 && max(it[1], it[3]) + grow >= tx0 && min(it[2], it[4]) - grow <= ty1 && max(it[2], it[4]) + grow >= ty0;
      }
    }
    const unsigned long long ballot = __ballot(hit);
    if (lane == 0) s_wave[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < kThreads / 64; ++v) {
      const int c = s_wave[v];
      if (v < wave) before += c;
      total += c;
    }
    if (hit) {
      int* dst = s_item[count + before + __popcll(ballot & ((1ull << lane) - 1ull))];
#pragma unroll
      for (int q = 0; q < kInts; ++q) dst[q] = it[q];
    }
    count += total;
    __syncthreads();   // the list is complete up to `count`; s_wave may be written again
    if (count > kList - kThreads || base + kThreads >= n) {   // the next pass might not fit, or there is none
      if (count > 0) {
        if (!loaded) {
          if (ina) { ba = qa[0]; ga = qa[1]; ra = qa[2]; }
          if (inb) { bb = qb[0]; gb = qb[1]; rb = qb[2]; }
          loaded = true;
        }
        for (int s = 0; s < count; ++s) {
          const int* item = s_item[s];
          if (ina) { const int c = covers(item, p, px, pya); if (c) { blend(c, item, ba, ga, ra); dirty_a = true; } }
          if (inb) { const int c = covers(item, p, px, pyb); if (c) { blend(c, item, bb, gb, rb); dirty_b = true; } }
        }
        __syncthreads();   // every thread is through the list before the next pass overwrites it
      }
      count = 0;
    }
  }
  if (dirty_a) { qa[0] = (unsigned char)ba; qa[1] = (unsigned char)ga; qa[2] = (unsigned char)ra; }
  if (dirty_b) { qb[0] = (unsigned char)bb; qb[1] = (unsigned char)gb; qb[2] = (unsigned char)rb; }
}

}  // namespace

hipError_t launch_overlay_update(const OverlayUpdateParams& p, hipStream_t stream) {
  if (!p.joints || !p.num_people || !p.recs || !p.table || !p.items || !p.num_items || p.num_parts < 1 || p.num_parts > RTP_TRACK_MAX_PARTS ||
      p.what == 0 || (p.what & ~7u) || !(p.min_score >= 0.f) || p.box_margin < 0 || p.box_margin > 1024 || p.line_width < 1 || p.line_width > 16 ||
      p.label_scale < 1 || p.label_scale > 8 || p.trail_len < 0 || p.trail_len > RTP_OVL_TRAIL_MAX || p.trail_radius < 0 || p.trail_radius > 16 ||
      p.alpha < 0 || p.alpha > 256)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(overlay_update_kernel, dim3(1), dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_overlay_draw(const OverlayDrawParams& p, hipStream_t stream) {
  if (!p.items || !p.num_items || !p.image || p.w < 1 || p.h < 1 || p.w > 32768 || p.h > 32768 || p.stride < 3L * p.w) return hipErrorInvalidValue;
  hipLaunchKernelGGL(overlay_draw_kernel, dim3((p.w + kTileW - 1) / kTileW, (p.h + kTileH - 1) / kTileH), dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}

}  // namespace rtp

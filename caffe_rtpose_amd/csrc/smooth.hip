// smooth.hip — smoothing mode (rtp_set_smoothing): the frame's people, read in device memory behind the track kernel together with
// their track records, go through a One-Euro filter per (track slot, part).  One launch per frame, ONE workgroup: the filter table is
// a single sequence of states, and the launches of consecutive frames are ordered by the engine (an event behind each).  *num_people
// is read on the device (no host synchronisation; a negative value is connect's error code and counts as 0).
//
// The arithmetic is rtp_smooth_update's (host_util.cpp; include/rtpose_mi355x.h spells it out), float bit for float bit and byte for
// byte: every operation rounded on its own (this file is built with -ffp-contract=off, like track.hip), `/` is the correctly rounded
// division, and every (person, part) item is computed by one thread from its own cell, so no result depends on how the items are
// spread over lanes.  A record names each slot at most once (rtp_track_update's records do), so no two items share a cell.
//
// The one shared value is the table's `frames`: every thread reads the old value, a barrier, thread 0 writes the new one.  The
// workgroup then loops over the n * P <= 6720 items.  Built with 256 and with 1024 threads (kernels.h RTP_SMOOTH_*); both are
// measured (profiles/r14_smooth.txt, tools/bench_smooth.py).  A record whose slot is outside the table (rtp_smooth_update refuses
// it) is handled as an untracked person: nothing outside the table is addressed.  Table and outputs are written with ordinary
// vector stores.
#include "kernels.h"

namespace rtp {

namespace {

constexpr int kSlots = RTP_TRACK_SLOTS, kPeople = RTP_TRACK_MAX_PEOPLE;
constexpr float kTwoPi = 6.2831855f;   // 0x40C90FDB

// one coordinate of the FILTER step: *vh_out = the filtered value, *e_out = the filtered velocity
__device__ __forceinline__ void one_euro(float v, float vh, float dvh, float dt, float min_cutoff, float beta, float d_cutoff, float* vh_out, float* e_out) {
  const float d = v - vh;
  const float dv = d / dt;
  float rd = kTwoPi * d_cutoff;
  rd = rd * dt;
  const float rd1 = rd + 1.0f;
  const float ad = rd / rd1;
  const float t1 = ad * dv;
  const float ad1 = 1.0f - ad;
  const float t2 = ad1 * dvh;
  const float e = t1 + t2;
  float fc = beta * fabsf(e);
  fc = min_cutoff + fc;
  float r = kTwoPi * fc;
  r = r * dt;
  const float r1 = r + 1.0f;
  const float a = r / r1;
  const float u1 = a * v;
  const float a1 = 1.0f - a;
  const float u2 = a1 * vh;
  *vh_out = u1 + u2;
  *e_out = e;
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void smooth_kernel(SmoothParams p) {
  SmoothTable* tb = p.table;
  const int tid = threadIdx.x;
  const int P = p.num_parts;
  const int people = *p.num_people;
  const int n = min(max(people, 0), kPeople);
  unsigned now = tb->frames + 1u;
  if (now == 0u) now = 1u;
  __syncthreads();   // every thread has read the old `frames`
  if (tid == 0) tb->frames = now;
  const unsigned max_hold = (unsigned)p.max_hold;
  const int items = n * P;
  for (int i = tid; i < items; i += kThreads) {
    const int k = i / P, q = i - k * P;
    const int id = p.recs[4 * k], t = p.recs[4 * k + 1];
    const float x = p.joints[3 * i], y = p.joints[3 * i + 1], score = p.joints[3 * i + 2];
    const bool counts = score > p.min_score && __builtin_isfinite(x) && __builtin_isfinite(y);   // (a NaN score fails the comparison)
    float ox = x, oy = y, os = score, vx = 0.0f, vy = 0.0f;
    int flag;
    if (id == 0 || t < 0 || t >= kSlots) {
      flag = counts ? 1 : 0;
    } else {
      SmoothCell* c = &tb->cell[t][q];
      const int owner = c->owner;
      const unsigned last = c->last;
      const bool live = owner == id && last != 0u;
      const unsigned g = now - last;
      bool start = counts && (!live || g - 1u > max_hold);
      flag = 0;
      if (counts && !start) {
        const float dt = (float)g;
        float nx, ny, ex, ey;
        one_euro(x, c->pos[0], c->vel[0], dt, p.min_cutoff, p.beta, p.d_cutoff, &nx, &ex);
        one_euro(y, c->pos[1], c->vel[1], dt, p.min_cutoff, p.beta, p.d_cutoff, &ny, &ey);
        if (__builtin_isfinite(nx) && __builtin_isfinite(ny) && __builtin_isfinite(ex) && __builtin_isfinite(ey)) {
          c->pos[0] = nx; c->pos[1] = ny; c->vel[0] = ex; c->vel[1] = ey; c->score = score; c->last = now;
          ox = nx; oy = ny; vx = ex; vy = ey;
          flag = 2;
        } else {
          start = true;
        }
      }
      if (start) {
        c->owner = id; c->last = now; c->pos[0] = x; c->pos[1] = y; c->vel[0] = 0.0f; c->vel[1] = 0.0f; c->score = score;
        flag = 1;
      } else if (!counts && live && g <= max_hold) {
        ox = c->pos[0]; oy = c->pos[1]; os = c->score; vx = c->vel[0]; vy = c->vel[1];
        flag = 3;
      }
    }
    p.joints_s[3 * i] = ox; p.joints_s[3 * i + 1] = oy; p.joints_s[3 * i + 2] = os;
    p.vel[2 * i] = vx; p.vel[2 * i + 1] = vy;
    p.flags[i] = (unsigned char)flag;
  }
}

}  // namespace

hipError_t launch_smooth(const SmoothParams& p, hipStream_t stream) {
  if (!p.joints || !p.num_people || !p.recs || !p.table || !p.joints_s || !p.vel || !p.flags || p.num_parts < 1 || p.num_parts > RTP_TRACK_MAX_PARTS ||
      p.max_hold < 0 || p.max_hold > 1000 || !(p.min_score >= 0.f) || !(p.min_cutoff > 0.f) || !(p.beta >= 0.f) || !(p.d_cutoff > 0.f) || p.variant < 0 ||
      p.variant >= RTP_SMOOTH_VARIANTS)
    return hipErrorInvalidValue;
  if (p.variant == RTP_SMOOTH_1024) hipLaunchKernelGGL((smooth_kernel<1024>), dim3(1), dim3(1024), 0, stream, p);
  else hipLaunchKernelGGL((smooth_kernel<256>), dim3(1), dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace rtp

// track.hip — tracking mode (rtp_set_tracking): the frame's people, read in device memory behind the connect kernels, are associated
// with the engine's track table.  One launch per frame, ONE workgroup: the table is a single sequence of states, and the launches of
// consecutive frames are ordered by the engine (an event behind each).  *num_people is read on the device (no host synchronisation;
// a negative value is connect's error code and counts as 0).
//
// The arithmetic is rtp_track_update's (host_util.cpp; include/rtpose_mi355x.h spells it out), integer for integer and float bit
// for float bit: every operation rounded on its own (this file is built with -ffp-contract=off, like crops.hip), and every sum
// is taken by ONE thread that walks the parts in order, so no result depends on how work is spread over lanes.
//
// Phases, a barrier between each; every loop is bounded by the live counts (nl live slots, np trackable people, n people):
//   A  threads 0..127 take a slot each (live? the track's size d), threads 128..223 a person each (trackable?); ballots compact the
//      live slots and the trackable people into ascending lists.
//   B  one thread per (live slot, trackable person) pair runs the sequential part loop; the cost's bits go to LDS at
//      [ti * np + ki] (ti, ki = positions in the two lists), 0xffffffff for a pair that is no candidate.  96 x 128 pairs = 48 KB.
//      Joints are read from global memory: 96 people of 70 parts are 80 KB and would not fit next to the keys.
//   C  greedy assignment on the keys (cost bits << 32 | index; the lists are ascending, so index order is (slot, person) order),
//      in one of two forms (kernels.h RTP_TRACK_*):
//      ARGMIN  the repeated global minimum: each round is a workgroup-wide argmin over the keys, then the winner's row and column
//              are struck out.  At most min(nl, np) rounds of two barriers each.
//      SORT    phase B also appends every candidate's index to a list (an LDS counter: the list's order is arbitrary, the keys are
//              distinct).  The M candidates, padded to the next power of two with a sentinel, are sorted once (bitonic network over
//              16-bit indices, compared through their keys: one barrier per stage, 6 stages for 8 candidates, 28 for 96), then
//              thread 0 walks the list and accepts a candidate when neither its slot nor its person is taken.  Up to 12288
//              candidates are 32 KB of indices behind the 48 KB of keys: dynamic LDS above 64 KB, opted into once per device.
//      Both are built with 256 and with 1024 threads and all four are measured (profiles/r13_track.txt, tools/bench_track.py).
//   D  one thread per slot: hits / misses, slots freed.   E  thread 0: births in person order, each into the lowest free slot.
//   F  the joints of every tracked person into its slot, zeros into freed slots, the records.
// Table and records are written with ordinary vector stores.
//
// The appearance form (rtp_set_track_appearance; rtp_track_update_appearance is its definition) is the same body with a third template
// parameter: phase B adds the 128-bin L1 distance between the slot's descriptor and the person's to a pair that passed the motion gate,
// phase F blends or replaces the descriptors of the slots that took a person.  It has instantiations of its own (a second kernel argument); the
// four track_kernel instantiations instantiate none of it.
#include <atomic>

#include "kernels.h"

namespace rtp {

namespace {

constexpr int kSlots = RTP_TRACK_SLOTS, kPeople = RTP_TRACK_MAX_PEOPLE, kPairs = kSlots * kPeople, kMaxSort = 16384;
constexpr unsigned kPad = 0xffffu;   // the sort's sentinel index: its key is the largest
constexpr unsigned kNone = 0xffffffffu;

__device__ __forceinline__ bool part_counts(float x, float y, float s, float min_score) {
  return s > min_score && __builtin_isfinite(x) && __builtin_isfinite(y);   // (a NaN score fails the comparison)
}

__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

// THE COST's appearance term on two packed uint16: |desc - 16 * bins| of both halves
__device__ __forceinline__ int l1_pair(unsigned d, unsigned b) {
  const int lo = (int)(d & 0xffffu) - 16 * (int)(b & 0xffffu), hi = (int)(d >> 16) - 16 * (int)(b >> 16);
  return (lo < 0 ? -lo : lo) + (hi < 0 ? -hi : hi);
}
// THE TABLE UPDATE on two packed uint16 (rate 256 replaces: (16 * bins * 256 + 128) >> 8 = 16 * bins); each half is cut to 16 bits as the host's cast does
__device__ __forceinline__ unsigned blend_pair(unsigned d, unsigned b, int rate) {
  const unsigned lo = ((d & 0xffffu) * (unsigned)(256 - rate) + 16u * (b & 0xffffu) * (unsigned)rate + 128u) >> 8;
  const unsigned hi = ((d >> 16) * (unsigned)(256 - rate) + 16u * (b >> 16) * (unsigned)rate + 128u) >> 8;
  return (lo & 0xffffu) | (hi << 16);
}
// The key of a pair (slot t, person k) that passed the motion gate with `cost`: the bits of total + 0.0f, or kNone where the pair is no
// candidate.  One thread sums the 128 bins in order of integers, so nothing depends on how work is spread.  Table and descriptors come
// through L2 as 16 + 16 loads of 16 bytes.
__device__ __forceinline__ unsigned appear_key(const TrackAppearParams& a, int t, int k, bool has, float cost) {
  float dist = a.unknown;
  if (has && a.valid[k]) {
    const uint4* d = reinterpret_cast<const uint4*>(&a.table->desc[t][0]);
    const uint4* b = reinterpret_cast<const uint4*>(a.bins + (long)k * RTP_APPEAR_BINS);
    int L = 0;
#pragma unroll 4
    for (int i = 0; i < RTP_APPEAR_BINS / 8; ++i) {
      const uint4 dv = d[i], bv = b[i];
      L += l1_pair(dv.x, bv.x) + l1_pair(dv.y, bv.y) + l1_pair(dv.z, bv.z) + l1_pair(dv.w, bv.w);
    }
    dist = (float)L / 32768.0f;
    if (!(dist <= a.max_dist)) return kNone;
  }
  const float wa = a.weight * dist;
  const float total = cost + wa;
  if (!__builtin_isfinite(total)) return kNone;
  return __float_as_uint(total + 0.0f);
}

struct NoAppear {};
__device__ __forceinline__ NoAppear appear_args() { return {}; }
__device__ __forceinline__ const TrackAppearParams& appear_args(const TrackAppearParams& a) { return a; }

// A = nothing: the plain form, track_kernel<SORT, kThreads>(TrackParams).  A = TrackAppearParams: the appearance form, a second kernel
// argument: phase A notes which slots HAVE a descriptor, phase B takes THE COST's key where the plain form takes the motion cost's, and
// phase F gains THE TABLE UPDATE.  In the plain form none of it is instantiated.
template <bool SORT, int kThreads, class... A>
__global__ __launch_bounds__(kThreads) void track_kernel(TrackParams p, A... appear) {
  constexpr bool APPEAR = sizeof...(A) != 0;
  const auto& a = appear_args(appear...);
  constexpr int kWaves = kThreads / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  unsigned* const s_cost = reinterpret_cast<unsigned*>(s_dyn);                                      // [kPairs]
  unsigned short* const s_idx = reinterpret_cast<unsigned short*>(s_dyn + kPairs * sizeof(unsigned));   // SORT: [kMaxSort]
  __shared__ unsigned long long s_wmin[kWaves];
  __shared__ int s_count;
  __shared__ float s_d[kSlots];
  __shared__ unsigned s_cost_of[kPeople];
  __shared__ int s_rec_id[kPeople], s_rec_hits[kPeople];
  __shared__ int s_wtot[4];
  __shared__ short s_slots[kSlots], s_pers[kPeople];
  __shared__ short s_person_of[kSlots], s_slot_of[kPeople];
  __shared__ unsigned char s_free[kSlots], s_freed[kSlots], s_born[kPeople];
  __shared__ unsigned char s_has[APPEAR ? kSlots : 1], s_upd[APPEAR ? kPeople : 1];   // slot t has a descriptor; person k's table update: 0 none, 1 blend, 2 replace

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  TrackTable* tb = p.table;
  const int P = p.num_parts, P3 = P * 3;
  const int people = *p.num_people;
  const int n = min(max(people, 0), kPeople);

  // ---- A
  bool flag = false;
  if (tid == 0) s_count = 0;
  if (tid < kSlots) {
    const int t = tid;
    s_person_of[t] = -1;
    s_freed[t] = 0;
    flag = tb->id[t] != 0;
    if (flag) {
      const float* tj = &tb->joints[t][0][0];
      float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
      for (int q = 0; q < P; ++q) {
        const float x = tj[3 * q], y = tj[3 * q + 1], s = tj[3 * q + 2];
        if (!part_counts(x, y, s, p.min_score)) continue;
        const float xz = x + 0.0f, yz = y + 0.0f;
        x0 = fminf(x0, xz); x1 = fmaxf(x1, xz); y0 = fminf(y0, yz); y1 = fmaxf(y1, yz);
      }
      const float w = x1 - x0, h = y1 - y0;
      const float ww = w * w, hh = h * h;
      const float wh = ww + hh;
      s_d[t] = fmaxf(wh, 1.0f);
    }
    if constexpr (APPEAR) s_has[t] = flag && a.table->owner[t] == tb->id[t] ? 1 : 0;
  } else if (tid < kSlots + kPeople) {
    const int k = tid - kSlots;
    s_slot_of[k] = -1;
    s_cost_of[k] = 0;
    s_born[k] = 0;
    s_rec_id[k] = 0;
    s_rec_hits[k] = 0;
    if (k < n) {
      const float* pj = p.joints + (long)k * P3;
      int c = 0;
      for (int q = 0; q < P; ++q) c += part_counts(pj[3 * q], pj[3 * q + 1], pj[3 * q + 2], p.min_score) ? 1 : 0;
      flag = c >= p.min_parts;
    }
  }
  const unsigned long long ballot = __ballot(flag);
  const int prefix = __popcll(ballot & ((1ull << lane) - 1ull));
  if (lane == 0 && wave < 4) s_wtot[wave] = __popcll(ballot);   // (slots: waves 0 and 1, people: waves 2 and 3)
  __syncthreads();
  const int nl = s_wtot[0] + s_wtot[1], np = s_wtot[2] + s_wtot[3];   // <= 128, <= 96
  if (flag) {
    const int pos = prefix + ((wave & 1) ? s_wtot[wave - 1] : 0);
    if (wave < 2) s_slots[pos] = (short)tid;
    else s_pers[pos] = (short)(tid - kSlots);
  }
  __syncthreads();

  // ---- B
  const int C = nl * np;
  for (int idx = tid; idx < C; idx += kThreads) {
    const int ti = idx / np, ki = idx - ti * np;
    const int t = s_slots[ti], k = s_pers[ki];
    const float* tj = &tb->joints[t][0][0];
    const float* pj = p.joints + (long)k * P3;
    float s = 0.0f;
    int m = 0;
    for (int q = 0; q < P; ++q) {
      const float px = pj[3 * q], py = pj[3 * q + 1], ps = pj[3 * q + 2];
      const float tx = tj[3 * q], ty = tj[3 * q + 1], ts = tj[3 * q + 2];
      if (!part_counts(px, py, ps, p.min_score) || !part_counts(tx, ty, ts, p.min_score)) continue;
      const float dx = px - tx, dy = py - ty;
      const float a = dx * dx, b = dy * dy;
      const float c = a + b;
      s = s + c;
      ++m;
    }
    unsigned key = kNone;
    if (m >= p.min_common) {
      const float q = s / (float)m;
      const float cost = q / s_d[t];
      if (__builtin_isfinite(cost) && cost <= p.max_cost) {
        if constexpr (APPEAR) key = appear_key(a, t, k, s_has[t] != 0, cost);
        else key = __float_as_uint(cost + 0.0f);
      }
    }
    s_cost[idx] = key;
    if (SORT && key != kNone) s_idx[atomicAdd(&s_count, 1)] = (unsigned short)idx;   // (at most C <= 12288 entries)
  }
  __syncthreads();

  // ---- C
  if (SORT) {
    const int M = s_count;
    int N = 1;
    while (N < M) N <<= 1;                                      // <= kMaxSort
    for (int i = M + tid; i < N; i += kThreads) s_idx[i] = (unsigned short)kPad;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int q = tid; q < (N >> 1); q += kThreads) {
          const int lo = ((q & ~(j - 1)) << 1) | (q & (j - 1)), hi = lo | j;
          const unsigned a = s_idx[lo], b = s_idx[hi];
          const unsigned long long ka = a == kPad ? ~0ull : ((unsigned long long)s_cost[a] << 32) | a;
          const unsigned long long kb = b == kPad ? ~0ull : ((unsigned long long)s_cost[b] << 32) | b;
          if ((ka > kb) == ((lo & k) == 0)) { s_idx[lo] = (unsigned short)b; s_idx[hi] = (unsigned short)a; }
        }
        __syncthreads();
      }
    if (tid == 0) {
      const int most = min(nl, np);
      int matched = 0;
      for (int r = 0; r < M && matched < most; ++r) {
        const int idx = s_idx[r];
        const int ti = idx / np, ki = idx - ti * np;
        const int t = s_slots[ti], k = s_pers[ki];
        if (s_person_of[t] >= 0 || s_slot_of[k] >= 0) continue;
        s_person_of[t] = (short)k;
        s_slot_of[k] = (short)t;
        s_cost_of[k] = s_cost[idx];
        ++matched;
      }
    }
    __syncthreads();
  } else
  for (;;) {
    unsigned long long best = ~0ull;
#pragma unroll 4
    for (int idx = tid; idx < C; idx += kThreads) {
      const unsigned b = s_cost[idx];
      const unsigned long long key = ((unsigned long long)b << 32) | (unsigned)idx;
      if (b != kNone && key < best) best = key;
    }
    best = wave_min64(best);
    if (lane == 0) s_wmin[wave] = best;
    __syncthreads();
    best = s_wmin[0];
#pragma unroll
    for (int i = 1; i < kWaves; ++i) best = s_wmin[i] < best ? s_wmin[i] : best;
    if ((unsigned)(best >> 32) == kNone) break;   // (the same values in every thread: the whole workgroup leaves)
    const int idx = (int)(unsigned)best;
    const int ti = idx / np, ki = idx - ti * np;
    if (tid == 0) {
      const int t = s_slots[ti], k = s_pers[ki];
      s_person_of[t] = (short)k;
      s_slot_of[k] = (short)t;
      s_cost_of[k] = (unsigned)(best >> 32);
    }
    if (tid < np) s_cost[ti * np + tid] = kNone;                                   // the slot's row
    if (tid >= kSlots && tid - kSlots < nl) s_cost[(tid - kSlots) * np + ki] = kNone;   // the person's column
    __syncthreads();
  }

  // ---- D
  if (tid < kSlots) {
    const int t = tid;
    const int id = tb->id[t];
    bool is_free = id == 0;
    if (id != 0) {
      const int k = s_person_of[t];
      if (k >= 0) {
        const int hits = tb->hits[t] + 1;
        tb->hits[t] = hits;
        tb->misses[t] = 0;
        s_rec_id[k] = id;
        s_rec_hits[k] = hits;
      } else {
        const int misses = tb->misses[t] + 1;
        if (misses > p.max_misses) {
          tb->id[t] = 0; tb->hits[t] = 0; tb->misses[t] = 0;
          s_freed[t] = 1;
          is_free = true;
        } else {
          tb->misses[t] = misses;
        }
      }
    }
    s_free[t] = is_free ? 1 : 0;
  }
  __syncthreads();

  // ---- E
  if (tid == 0) {
    unsigned next = tb->next_id;
    int ft = 0;
    for (int ki = 0; ki < np; ++ki) {
      const int k = s_pers[ki];
      if (s_slot_of[k] >= 0) continue;
      while (ft < kSlots && !s_free[ft]) ++ft;
      if (ft == kSlots) break;
      if (next == 0u) next = 1u;
      const int id = (int)next++;
      if (next == 0u) next = 1u;
      tb->id[ft] = id; tb->hits[ft] = 1; tb->misses[ft] = 0;
      s_free[ft] = 0;
      s_freed[ft] = 0;   // (its joints are overwritten below; beyond num_parts they are zeros already)
      s_slot_of[k] = (short)ft;
      s_born[k] = 1;
      s_rec_id[k] = id;
      s_rec_hits[k] = 1;
    }
    tb->next_id = next;
    tb->frames = tb->frames + 1u;
  }
  __syncthreads();

  // ---- F
  for (int e = tid; e < n * P3; e += kThreads) {
    const int k = e / P3, j = e - k * P3;
    const int t = s_slot_of[k];
    if (t >= 0) (&tb->joints[t][0][0])[j] = p.joints[e];
  }
  constexpr int kRow = RTP_TRACK_MAX_PARTS * 3;   // (the whole row, as the host's memset)
  for (int e = tid; e < nl * kRow; e += kThreads) {
    const int ti = e / kRow, j = e - ti * kRow;
    const int t = s_slots[ti];
    if (s_freed[t]) (&tb->joints[t][0][0])[j] = 0.0f;
  }
  if (tid < n) {
    const int k = tid;
    const int t = s_slot_of[k];
    int4 r;
    if (t < 0) r = make_int4(0, -1, 0, 0);
    else r = make_int4(s_rec_id[k], t, s_rec_hits[k], s_born[k] ? 0 : (int)s_cost_of[k]);
    reinterpret_cast<int4*>(p.recs)[k] = r;
  }
  if constexpr (APPEAR) {
    // THE TABLE UPDATE: what happens to each person's slot is decided on the owners as they stand (s_rec_id = the slot's id now), then,
    // behind a barrier, one thread per 8 bins blends or replaces them and the first of a replaced slot's threads writes the owner
    if (tid < n) {
      const int t = s_slot_of[tid];
      s_upd[tid] = (t >= 0 && a.valid[tid]) ? (a.table->owner[t] == s_rec_id[tid] ? 1 : 2) : 0;
    }
    __syncthreads();
    for (int e = tid; e < n * (RTP_APPEAR_BINS / 8); e += kThreads) {
      const int k = e >> 4, g = e & 15;
      const int u = s_upd[k];
      if (!u) continue;
      const int t = s_slot_of[k];
      const int rate = u == 1 ? a.rate : 256;
      uint4* dp = reinterpret_cast<uint4*>(&a.table->desc[t][0]) + g;
      const uint4 bv = reinterpret_cast<const uint4*>(a.bins + (long)k * RTP_APPEAR_BINS)[g];
      uint4 dv = *dp;
      dv.x = blend_pair(dv.x, bv.x, rate); dv.y = blend_pair(dv.y, bv.y, rate); dv.z = blend_pair(dv.z, bv.z, rate); dv.w = blend_pair(dv.w, bv.w, rate);
      *dp = dv;
      if (g == 0 && u == 2) a.table->owner[t] = s_rec_id[k];
    }
  }
}


// > 64 KiB of dynamic LDS is an opt-in per kernel and device: one driver call, cached
template <bool SORT, int kThreads>
hipError_t launch_one(const TrackParams& p, hipStream_t stream) {
  const size_t lds = kPairs * sizeof(unsigned) + (SORT ? kMaxSort * sizeof(unsigned short) : 0);
  if (lds > 60 * 1024) {   // (the kernel declares about 3 KB statically)
    static std::atomic<unsigned> have{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned bit = 1u << (dev & 31);
    if (!(have.load(std::memory_order_relaxed) & bit)) {
      const hipError_t e = hipFuncSetAttribute((const void*)track_kernel<SORT, kThreads>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      have.fetch_or(bit, std::memory_order_relaxed);
    }
  }
  hipLaunchKernelGGL((track_kernel<SORT, kThreads>), dim3(1), dim3(kThreads), lds, stream, p);
  return hipGetLastError();
}

// The appearance form: the same dynamic LDS (table and descriptors are read through L2, nothing is staged), opted into for its own kernel
template <bool SORT, int kThreads>
hipError_t launch_one_appear(const TrackParams& p, const TrackAppearParams& a, hipStream_t stream) {
  const size_t lds = kPairs * sizeof(unsigned) + (SORT ? kMaxSort * sizeof(unsigned short) : 0);
  if (lds > 60 * 1024) {
    static std::atomic<unsigned> have{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned bit = 1u << (dev & 31);
    if (!(have.load(std::memory_order_relaxed) & bit)) {
      const hipError_t e = hipFuncSetAttribute((const void*)track_kernel<SORT, kThreads, TrackAppearParams>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      have.fetch_or(bit, std::memory_order_relaxed);
    }
  }
  hipLaunchKernelGGL((track_kernel<SORT, kThreads, TrackAppearParams>), dim3(1), dim3(kThreads), lds, stream, p, a);
  return hipGetLastError();
}

bool track_params_ok(const TrackParams& p) {
  return p.joints && p.num_people && p.table && p.recs && p.num_parts >= 1 && p.num_parts <= RTP_TRACK_MAX_PARTS && p.min_parts >= 1 && p.min_common >= 1 &&
         p.max_misses >= 0 && p.min_score >= 0.f && p.max_cost > 0.f && (unsigned long long)(uintptr_t)p.recs % 16 == 0 && p.variant >= 0 &&
         p.variant < RTP_TRACK_VARIANTS;
}

}  // namespace

hipError_t launch_track_appearance(const TrackParams& p, const TrackAppearParams& a, hipStream_t stream) {
  if (!track_params_ok(p) || !a.bins || !a.valid || !a.table || (unsigned long long)(uintptr_t)a.bins % 16 != 0 || (unsigned long long)(uintptr_t)a.table % 16 != 0 ||
      !(a.weight >= 0.f) || !(a.max_dist > 0.f && a.max_dist <= 1.f) || !(a.unknown >= 0.f && a.unknown <= 1.f) || a.rate < 1 || a.rate > 256)
    return hipErrorInvalidValue;
  switch (p.variant) {
    case RTP_TRACK_ARGMIN_256: return launch_one_appear<false, 256>(p, a, stream);
    case RTP_TRACK_ARGMIN_1024: return launch_one_appear<false, 1024>(p, a, stream);
    case RTP_TRACK_SORT_256: return launch_one_appear<true, 256>(p, a, stream);
    default: return launch_one_appear<true, 1024>(p, a, stream);
  }
}

hipError_t launch_track(const TrackParams& p, hipStream_t stream) {
  if (!p.joints || !p.num_people || !p.table || !p.recs || p.num_parts < 1 || p.num_parts > RTP_TRACK_MAX_PARTS || p.min_parts < 1 || p.min_common < 1 ||
      p.max_misses < 0 || !(p.min_score >= 0.f) || !(p.max_cost > 0.f) || (unsigned long long)(uintptr_t)p.recs % 16 != 0 || p.variant < 0 ||
      p.variant >= RTP_TRACK_VARIANTS)
    return hipErrorInvalidValue;
  switch (p.variant) {
    case RTP_TRACK_ARGMIN_256: return launch_one<false, 256>(p, stream);
    case RTP_TRACK_ARGMIN_1024: return launch_one<false, 1024>(p, stream);
    case RTP_TRACK_SORT_256: return launch_one<true, 256>(p, stream);
    default: return launch_one<true, 1024>(p, stream);
  }
}

}  // namespace rtp

// engine_smooth.cpp — the engine's side of smoothing mode (smooth.hip): the mode switch, the device-resident filter table, the per-slot
// output buffers, the kernel each submitted frame's post-processing chain gains behind its track kernel while the mode is on, the peek
// entry, the state entries and the parity tap.  Outputs and table are rtp_smooth_update's (host_util.cpp) bit for bit.
//
// The filter table is one per engine and is updated in submit order, like the track table, and by the same chain of events
// (engine_track.cpp: ORDERING): while the mode is on, the event the next frame's track kernel waits on is recorded behind this
// frame's SMOOTH kernel, which runs on the same stream as its track kernel.
#include "engine_internal.h"

static_assert(sizeof(SmoothTable) == sizeof(rtp_smooth_state) && sizeof(SmoothCell) == sizeof(rtp_smooth_cell), "SmoothTable is rtp_smooth_state's layout");
static_assert(offsetof(SmoothTable, num_parts) == offsetof(rtp_smooth_state, num_parts) && offsetof(SmoothTable, frames) == offsetof(rtp_smooth_state, frames) &&
              offsetof(SmoothTable, cell) == offsetof(rtp_smooth_state, cell), "SmoothTable is rtp_smooth_state's layout");
static_assert(offsetof(SmoothCell, owner) == offsetof(rtp_smooth_cell, owner) && offsetof(SmoothCell, last) == offsetof(rtp_smooth_cell, last) &&
              offsetof(SmoothCell, pos) == offsetof(rtp_smooth_cell, pos) && offsetof(SmoothCell, vel) == offsetof(rtp_smooth_cell, vel) &&
              offsetof(SmoothCell, score) == offsetof(rtp_smooth_cell, score), "SmoothCell is rtp_smooth_cell's layout");

namespace rtp {
namespace eng __attribute__((visibility("hidden"))) {

namespace {

size_t items(const rtp_engine* e) { return (size_t)RTP_MAX_PEOPLE * e->plan.num_parts; }

// the kernel on slot sj's joints and records -> the slot's output buffers, on `stream`
int smooth_enqueue(rtp_engine* e, Ctx& cx, int sj, hipStream_t stream) {
  Slot& sl = cx.slot[sj];
  const rtp_smooth_config& c = e->smooth_cfg;
  SmoothParams p;
  memset(&p, 0, sizeof p);
  p.joints = sl.joints; p.num_people = sl.num_people; p.recs = sl.track.recs_dev;
  p.table = e->smooth_dev;
  p.joints_s = sl.smooth.joints_dev; p.vel = sl.smooth.vel_dev; p.flags = sl.smooth.flags_dev;
  p.num_parts = e->plan.num_parts; p.max_hold = c.max_hold;
  p.min_score = c.min_score; p.min_cutoff = c.min_cutoff; p.beta = c.beta; p.d_cutoff = c.d_cutoff;
  p.variant = e->smooth_variant;
  HIPCHK(e, launch_smooth(p, stream));   // no residency stamp: every slot of a frame's chain is taken (StampKind)
  return RTP_OK;
}

// an empty table (or the caller's) into the device copy; the engine is idle
int table_upload(rtp_engine* e, const rtp_smooth_state* st) {
  SYNC_GUARD;
  if (!e->smooth_dev) HIPCHK(e, hipMalloc((void**)&e->smooth_dev, sizeof(SmoothTable)));
  HIPCHK(e, hipMemcpy(e->smooth_dev, st, sizeof *st, hipMemcpyHostToDevice));
  track_forget_chain(e);
  return RTP_OK;
}

int table_reset(rtp_engine* e) {
  std::vector<unsigned char> buf(sizeof(rtp_smooth_state));
  rtp_smooth_state* st = reinterpret_cast<rtp_smooth_state*>(buf.data());
  if (rtp_smooth_state_init(st, e->plan.num_parts) != RTP_OK) return fail(e, RTP_EINVAL, "smoothing: the model has %d parts", e->plan.num_parts);
  return table_upload(e, st);
}

// what the state entries refuse: mode off, frames in flight, a busy device
int state_checks(rtp_engine* e, const char* fn) {
  if (!e->smooth_on) return fail(e, RTP_EINVAL, "%s: smoothing mode is off (rtp_set_smoothing)", fn);
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  return need_idle(e);
}

}  // namespace

void SmoothOut::free() {
  if (joints_dev) (void)hipFree(joints_dev);
  if (vel_dev) (void)hipFree(vel_dev);
  if (flags_dev) (void)hipFree(flags_dev);
  if (host) (void)hipHostFree(host);
  joints_dev = vel_dev = nullptr;
  flags_dev = nullptr;
  host = nullptr;
}

void smooth_free(rtp_engine* e) {
  if (e->smooth_dev) (void)hipFree(e->smooth_dev);
  e->smooth_dev = nullptr;
}

// The output buffers of the first nframes slots, before their batch is launched (frame_outputs_ensure, and the tap).  The pinned
// copy is one block: [joints_s][vel][flags].
int smooth_ensure(rtp_engine* e, Ctx& cx, int nframes) {
  const size_t n = items(e);
  for (int j = 0; j < nframes; ++j) {
    SmoothOut& s = cx.slot[j].smooth;
    if (s.joints_dev) continue;
    SYNC_GUARD;
    HIPCHK(e, hipMalloc((void**)&s.joints_dev, n * 3 * sizeof(float)));
    HIPCHK(e, hipMalloc((void**)&s.vel_dev, n * 2 * sizeof(float)));
    HIPCHK(e, hipMalloc((void**)&s.flags_dev, n));
    HIPCHK(e, hipHostMalloc((void**)&s.host, n * (5 * sizeof(float) + 1), hipHostMallocDefault));
  }
  return RTP_OK;
}

// frame_outputs_launch: frame sj's filter step on the frame's own stream behind its track kernel (track_launch with smooth_follows),
// the event the next frame's chain waits on behind it, and the three arrays -> pinned memory in front of the frame's last event
int smooth_launch(rtp_engine* e, Ctx& cx, int sj, bool table_kernel_follows) {
  Slot& sl = cx.slot[sj];
  int rc;
  if ((rc = smooth_enqueue(e, cx, sj, sl.stream))) return rc;
  if (!table_kernel_follows) {   // (otherwise overlay_update_launch records it, behind its kernel)
    HIPCHK(e, hipEventRecord(sl.track.ev, sl.stream));
    e->track_prev = sl.track.ev;
    e->track_prev_stream = sl.stream;
  }
  const size_t n = items(e);
  unsigned char* h = sl.smooth.host;
  HIPCHK(e, hipMemcpyAsync(h, sl.smooth.joints_dev, n * 3 * sizeof(float), hipMemcpyDeviceToHost, sl.stream));
  HIPCHK(e, hipMemcpyAsync(h + n * 3 * sizeof(float), sl.smooth.vel_dev, n * 2 * sizeof(float), hipMemcpyDeviceToHost, sl.stream));
  HIPCHK(e, hipMemcpyAsync(h + n * 5 * sizeof(float), sl.smooth.flags_dev, n, hipMemcpyDeviceToHost, sl.stream));
  return RTP_OK;
}

}  // namespace eng
}  // namespace rtp

namespace {

// n people of the slot's pinned block into the caller's arrays
void copy_out(const rtp_engine* e, const Slot& sl, int n, float* joints_s, float* vel, unsigned char* flags) {
  const size_t all = (size_t)RTP_MAX_PEOPLE * e->plan.num_parts, m = (size_t)n * e->plan.num_parts;
  const unsigned char* h = sl.smooth.host;
  memcpy(joints_s, h, m * 3 * sizeof(float));
  if (vel) memcpy(vel, h + all * 3 * sizeof(float), m * 2 * sizeof(float));
  if (flags) memcpy(flags, h + all * 5 * sizeof(float), m);
}

}  // namespace

extern "C" {

// The workgroup's size, kernels.h RTP_SMOOTH_* (idle engine; not part of the public header — tools/bench_smooth.py times both,
// tests/test_smooth.py holds both to rtp_smooth_update).  Returns the previous value.
extern "C" int rtp_internal_smooth_variant(rtp_engine* e, int variant) {
  static const char* fn = "rtp_internal_smooth_variant";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (variant < 0 || variant >= RTP_SMOOTH_VARIANTS) return fail(e, RTP_EINVAL, "%s: variant %d outside 0 .. %d", fn, variant, RTP_SMOOTH_VARIANTS - 1);
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  const int before = e->smooth_variant;
  e->smooth_variant = variant;
  return before;
}

// The kernel alone (idle engine, context 0; not part of the public header — tools/bench_smooth.py): `people` people with their records
// against the table as it stands, `launches` (at most 400: they are enqueued within 4 ms) launches back to back on the slot's stream
// between two events; the table is restored afterwards.  *period_us = one launch's period.
extern "C" int rtp_internal_smooth_time(rtp_engine* e, const float* joints_host, const int* recs_host, int num_people, int launches, float* period_us) {
  static const char* fn = "rtp_internal_smooth_time";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!period_us || launches < 1 || launches > 400 || num_people < 0 || num_people > RTP_MAX_PEOPLE || (num_people > 0 && (!joints_host || !recs_host)))
    return fail(e, RTP_EINVAL, "%s: bad argument", fn);
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if ((rc = track_ensure(e, cx, 1)) || (rc = smooth_ensure(e, cx, 1))) return rc;
  if (num_people > 0) {
    HIPCHK(e, hipMemcpy(sl.joints, joints_host, (size_t)num_people * e->plan.num_parts * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(sl.track.recs_dev, recs_host, (size_t)num_people * RTP_TRACK_REC_INTS * sizeof(int), hipMemcpyHostToDevice));
  }
  HIPCHK(e, hipMemcpy(sl.num_people, &num_people, sizeof(int), hipMemcpyHostToDevice));
  std::vector<unsigned char> keep(sizeof(rtp_smooth_state));
  HIPCHK(e, hipMemcpy(keep.data(), e->smooth_dev, keep.size(), hipMemcpyDeviceToHost));
  // (from here on every HIP status is kept in `s` and checked once everything is released)
  hipEvent_t ev[2] = {nullptr, nullptr};
  unsigned long long* hold = nullptr;
  hipError_t s = hipEventCreate(&ev[0]);
  if (s == hipSuccess) s = hipEventCreate(&ev[1]);
  if (s == hipSuccess) s = hipMalloc((void**)&hold, 2 * sizeof(unsigned long long));
  for (int i = 0; i < 3 && !rc && s == hipSuccess; ++i) rc = smooth_enqueue(e, cx, 0, sl.stream);   // warm-up
  // a wave that waits 4 ms holds the stream while the train is enqueued, so that the event pair brackets device work only
  if (s == hipSuccess) s = hipStreamSynchronize(sl.stream);
  if (s == hipSuccess && !rc) s = launch_queue_wait(400000, hold, sl.stream);
  if (s == hipSuccess && !rc) s = hipEventRecord(ev[0], sl.stream);
  for (int i = 0; i < launches && !rc && s == hipSuccess; ++i) rc = smooth_enqueue(e, cx, 0, sl.stream);
  if (s == hipSuccess && !rc) s = hipEventRecord(ev[1], sl.stream);
  if (s == hipSuccess && !rc) s = hipEventSynchronize(ev[1]);
  float ms = 0.f;
  if (s == hipSuccess && !rc) s = hipEventElapsedTime(&ms, ev[0], ev[1]);
  const hipError_t sync = hipStreamSynchronize(sl.stream);   // (nothing of the train is pending when the buffers go and the table comes back)
  if (s == hipSuccess) s = sync;
  for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
  if (hold) (void)hipFree(hold);
  const hipError_t back = hipMemcpy(e->smooth_dev, keep.data(), keep.size(), hipMemcpyHostToDevice);
  if (s == hipSuccess) s = back;
  if (rc) return rc;
  HIPCHK(e, s);
  *period_us = ms * 1e3f / (float)launches;
  return RTP_OK;
}

// The switch needs an idle engine, like tracking's.  Nothing is changed by a refused call.
int rtp_set_smoothing(rtp_engine* e, const rtp_smooth_config* cfg) {
  static const char* fn = "rtp_set_smoothing";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (cfg) {
    if (cfg->struct_size != sizeof(rtp_smooth_config))
      return fail(e, RTP_EINVAL, "%s: rtp_smooth_config.struct_size is %u, this library's rtp_smooth_config has %zu bytes", fn, cfg->struct_size, sizeof(rtp_smooth_config));
    const char* bad = rtp_internal_smooth_check(cfg);
    if (bad) return fail(e, RTP_EINVAL, "%s: %s (min_score %g, min_cutoff %g, beta %g, d_cutoff %g, max_hold %d, apply %u)", fn, bad, (double)cfg->min_score,
                         (double)cfg->min_cutoff, (double)cfg->beta, (double)cfg->d_cutoff, cfg->max_hold, cfg->apply);
    if (!e->track_on) return fail(e, RTP_EINVAL, "%s: tracking mode is off (rtp_set_tracking first)", fn);
  }
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (!cfg && !e->smooth_on) return RTP_OK;
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  SYNC_GUARD;
  int rc;
  if ((rc = need_idle(e))) return rc;
  if (cfg && !e->smooth_on && (rc = table_reset(e))) return rc;   // off -> on: an empty state
  if (!cfg) {
    for (Ctx& cx : e->ctx)
      for (Slot& sl : cx.slot) sl.smooth.free();
    smooth_free(e);
  }
  e->smooth_on = cfg != nullptr;
  e->smooth_cfg = cfg ? *cfg : rtp_smooth_config{};
  return RTP_OK;
}

int rtp_smooth_reset(rtp_engine* e) {
  static const char* fn = "rtp_smooth_reset";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  return table_reset(e);
}

int rtp_smooth_get_state(rtp_engine* e, rtp_smooth_state* state) {
  static const char* fn = "rtp_smooth_get_state";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!state) return fail(e, RTP_EINVAL, "%s: NULL state", fn);
  SYNC_GUARD;
  HIPCHK(e, hipDeviceSynchronize());
  HIPCHK(e, hipMemcpy(state, e->smooth_dev, sizeof *state, hipMemcpyDeviceToHost));
  track_forget_chain(e);
  return RTP_OK;
}

int rtp_smooth_set_state(rtp_engine* e, const rtp_smooth_state* state) {
  static const char* fn = "rtp_smooth_set_state";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!state) return fail(e, RTP_EINVAL, "%s: NULL state", fn);
  if (state->struct_size != sizeof(rtp_smooth_state))
    return fail(e, RTP_EINVAL, "%s: rtp_smooth_state.struct_size is %u, this library's rtp_smooth_state has %zu bytes", fn, state->struct_size, sizeof(rtp_smooth_state));
  if (state->num_parts != e->plan.num_parts) return fail(e, RTP_EINVAL, "%s: the state has %d parts per person, the engine's model %d", fn, state->num_parts, e->plan.num_parts);
  SYNC_GUARD;
  HIPCHK(e, hipDeviceSynchronize());
  return table_upload(e, state);
}

// Every refusal but RTP_ERANGE happens before anything is waited for; the frame stays in the FIFO either way.
int rtp_peek_smoothed(rtp_engine* e, uint64_t* tag, float* joints_s_host, float* vel_host, unsigned char* flags_host, int* num_people, int capacity) {
  static const char* fn = "rtp_peek_smoothed";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->smooth_on) return fail(e, RTP_EINVAL, "%s: smoothing mode is off (rtp_set_smoothing)", fn);
  if (!joints_s_host || !num_people || capacity < 0) return fail(e, RTP_EINVAL, "%s: NULL joints_s_host or num_people, or a negative capacity", fn);
  int rc, ci = 0, sj = 0;
  if ((rc = need_weights(e))) return rc;
  if ((rc = wait_oldest(e, &ci, &sj))) return rc;   // (refuses "nothing in flight" before it waits)
  const Slot& sl = e->ctx[ci].slot[sj];
  int people;
  memcpy(&people, sl.host_out, sizeof people);
  const int n = std::min(std::max(people, 0), RTP_MAX_PEOPLE);
  *num_people = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, the frame has %d people", fn, capacity, n);
  copy_out(e, sl, n, joints_s_host, vel_host, flags_host);
  if (tag) *tag = sl.tag;
  return RTP_OK;
}

// Parity tap: the two kernels of the async path on caller-supplied joints, context 0, slot 0; both tables advance by one frame
int rtp_smooth_from_joints(rtp_engine* e, const float* joints_host, int num_people, int* recs_host, float* joints_s_host, float* vel_host,
                           unsigned char* flags_host, int* num_out, int capacity) {
  static const char* fn = "rtp_smooth_from_joints";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->smooth_on) return fail(e, RTP_EINVAL, "%s: smoothing mode is off (rtp_set_smoothing)", fn);
  // (num_people goes to the device as it is: above RTP_MAX_PEOPLE and negative values are what the kernels have to clamp)
  const int n = std::min(std::max(num_people, 0), RTP_MAX_PEOPLE);
  if (!joints_s_host || !num_out || capacity < 0 || (n > 0 && !joints_host)) return fail(e, RTP_EINVAL, "%s: NULL joints_s_host, num_out or joints, or a negative capacity", fn);
  *num_out = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, %d people", fn, capacity, n);
  int rc;
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  if ((rc = need_idle(e))) return rc;
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if (n > 0) HIPCHK(e, hipMemcpy(sl.joints, joints_host, (size_t)n * e->plan.num_parts * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.num_people, &num_people, sizeof(int), hipMemcpyHostToDevice));
  if ((rc = track_ensure(e, cx, 1)) || (rc = smooth_ensure(e, cx, 1))) return rc;
  if ((rc = track_launch(e, cx, 0, true))) return rc;
  if ((rc = smooth_launch(e, cx, 0))) return rc;
  HIPCHK(e, hipStreamSynchronize(sl.stream));
  track_forget_chain(e);   // (complete: the next frame waits on nothing)
  if (recs_host) memcpy(recs_host, sl.track.recs_host, (size_t)n * RTP_TRACK_REC_INTS * sizeof(int));
  copy_out(e, sl, n, joints_s_host, vel_host, flags_host);
  return RTP_OK;
}

}  // extern "C"

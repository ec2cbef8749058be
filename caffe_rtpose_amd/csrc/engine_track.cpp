// engine_track.cpp — the engine's side of tracking mode (track.hip): the mode switch, the device-resident track table, the per-slot
// record buffers, the kernel each submitted frame's post-processing chain gains while the mode is on, the peek entry, the state
// entries and the parity tap.  Records and table are rtp_track_update's (host_util.cpp) integer for integer and bit for bit.
//
// ORDERING.  The table is one per engine, and frames must update it in submit order, while their chains run on different slot
// streams and contexts.  Frame n's kernel therefore waits (hipStreamWaitEvent on its slot's stream) on the event recorded behind
// frame n-1's kernel; rtp_engine::track_prev is that event.  Batches are launched in submit order (launch_open, pump) and
// launch_batch_body walks a batch's slots in slot order, so LAUNCH order is SUBMIT order, and the chain of events built at launch
// time is the chain of frames.  Whoever changes either order has to keep this one.  The first frame after a reset, and after every
// entry that synchronises with the device on an idle engine, waits on nothing.
// Smoothing mode (engine_smooth.cpp) has a table of its own with the same rule.  While it is on, a frame's smooth kernel follows its
// track kernel on the same stream, and the event (track_prev) is recorded behind the SMOOTH kernel instead: frame n's track kernel
// then waits for both of frame n-1's kernels, and this one chain of events orders both tables.  With smoothing off the event is
// recorded behind the track kernel.  Overlay mode (engine_overlay.cpp) adds a third table and a third kernel by the same rule: the
// event is recorded behind the LAST table kernel of the frame's chain (track -> smooth where on -> overlay_update where on).
#include "engine_internal.h"

static_assert(sizeof(TrackTable) == sizeof(rtp_track_state), "TrackTable is rtp_track_state's layout");
static_assert(offsetof(TrackTable, next_id) == offsetof(rtp_track_state, next_id) && offsetof(TrackTable, id) == offsetof(rtp_track_state, id) &&
              offsetof(TrackTable, hits) == offsetof(rtp_track_state, hits) && offsetof(TrackTable, misses) == offsetof(rtp_track_state, misses) &&
              offsetof(TrackTable, joints) == offsetof(rtp_track_state, joints), "TrackTable is rtp_track_state's layout");
static_assert(RTP_TRACK_SLOTS == RTP_MAX_TRACKS && RTP_TRACK_MAX_PARTS == RTP_MAX_NUM_PARTS && RTP_TRACK_MAX_PEOPLE == RTP_MAX_PEOPLE, "kernels.h mirrors the header");

namespace rtp {
namespace eng __attribute__((visibility("hidden"))) {

namespace {

constexpr size_t kRecBytes = (size_t)RTP_MAX_PEOPLE * RTP_TRACK_REC_INTS * sizeof(int);

// the kernel on slot sj's joints -> the slot's record buffer, on `stream`
int track_enqueue(rtp_engine* e, Ctx& cx, int sj, hipStream_t stream) {
  Slot& sl = cx.slot[sj];
  const rtp_track_config& c = e->track_cfg;
  TrackParams p;
  memset(&p, 0, sizeof p);
  p.joints = sl.joints; p.num_people = sl.num_people;
  p.table = e->track_dev; p.recs = sl.track.recs_dev;
  p.num_parts = e->plan.num_parts; p.min_parts = c.min_parts; p.min_common = c.min_common; p.max_misses = c.max_misses;
  p.min_score = c.min_score; p.max_cost = c.max_cost;
  p.variant = e->track_variant;
  if (e->appear_on) {   // the appearance form of the same kernel (engine_appearance.cpp): the frame's descriptors against the descriptor table
    TrackAppearParams a;
    appear_track_params(e, sl, &a);
    HIPCHK(e, launch_track_appearance(p, a, stream));
    return RTP_OK;
  }
  HIPCHK(e, launch_track(p, stream));   // no residency stamp: every slot of a frame's chain is taken (StampKind)
  return RTP_OK;
}

// an empty table (or the caller's) into the device copy; the engine is idle and nothing of the tracker is pending
int table_upload(rtp_engine* e, const rtp_track_state* st) {
  SYNC_GUARD;
  if (!e->track_dev) HIPCHK(e, hipMalloc((void**)&e->track_dev, sizeof(TrackTable)));
  HIPCHK(e, hipMemcpy(e->track_dev, st, sizeof *st, hipMemcpyHostToDevice));
  e->track_prev = nullptr;
  e->track_prev_stream = nullptr;
  return RTP_OK;
}

int table_reset(rtp_engine* e) {
  std::vector<unsigned char> buf(sizeof(rtp_track_state));
  rtp_track_state* st = reinterpret_cast<rtp_track_state*>(buf.data());
  if (rtp_track_state_init(st, e->plan.num_parts) != RTP_OK) return fail(e, RTP_EINVAL, "tracking: the model has %d parts", e->plan.num_parts);
  return table_upload(e, st);
}

// what the state entries refuse: mode off, frames in flight, a busy device
int state_checks(rtp_engine* e, const char* fn) {
  if (!e->track_on) return fail(e, RTP_EINVAL, "%s: tracking mode is off (rtp_set_tracking)", fn);
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);   // (a failed re-plan leaves the mode on and no contexts)
  return need_idle(e);
}

}  // namespace

void TrackOut::free() {
  if (recs_dev) (void)hipFree(recs_dev);
  if (recs_host) (void)hipHostFree(recs_host);
  if (ev) (void)hipEventDestroy(ev);
  recs_dev = recs_host = nullptr;
  ev = nullptr;
}

// the tracker's engine-wide pieces (drop_plan: the contexts and their events go, the table stays; rtp_engine_destroy: everything)
void track_forget_chain(rtp_engine* e) { e->track_prev = nullptr; e->track_prev_stream = nullptr; }
void track_free(rtp_engine* e) {
  track_forget_chain(e);
  if (e->track_dev) (void)hipFree(e->track_dev);
  e->track_dev = nullptr;
}

// The record buffers and events of the first nframes slots, before their batch is launched (frame_outputs_ensure, and the tap)
int track_ensure(rtp_engine* e, Ctx& cx, int nframes) {
  for (int j = 0; j < nframes; ++j) {
    TrackOut& t = cx.slot[j].track;
    if (t.recs_dev) continue;
    SYNC_GUARD;
    HIPCHK(e, hipMalloc((void**)&t.recs_dev, kRecBytes));
    HIPCHK(e, hipHostMalloc((void**)&t.recs_host, kRecBytes, hipHostMallocDefault));
    HIPCHK(e, hipEventCreateWithFlags(&t.ev, hipEventDisableTiming));
  }
  if (e->appear_on) return appear_ensure(e, cx, nframes);   // the appearance form reads the slot's descriptors
  return RTP_OK;
}

// frame_outputs_launch: frame sj's association on the frame's own stream behind the connect kernels, behind the previous frame's
// association wherever that ran (ORDERING above), and its records -> pinned memory in front of the frame's last event
int track_launch(rtp_engine* e, Ctx& cx, int sj, bool table_kernel_follows) {
  Slot& sl = cx.slot[sj];
  int rc;
  // appearance mode: a caller that has not described the frame (the joints-only taps) gets a frame without a display image
  if (e->appear_on && !sl.appear.fresh && (rc = appear_launch(e, cx, sj, false))) return rc;
  sl.appear.fresh = false;
  if (e->track_prev && e->track_prev_stream != sl.stream) HIPCHK(e, hipStreamWaitEvent(sl.stream, e->track_prev, 0));
  if ((rc = track_enqueue(e, cx, sj, sl.stream))) return rc;
  if (!table_kernel_follows) {   // (otherwise the last table kernel of the frame's chain records it, behind itself: smooth_launch, overlay_update_launch)
    HIPCHK(e, hipEventRecord(sl.track.ev, sl.stream));
    e->track_prev = sl.track.ev;
    e->track_prev_stream = sl.stream;
  }
  HIPCHK(e, hipMemcpyAsync(sl.track.recs_host, sl.track.recs_dev, kRecBytes, hipMemcpyDeviceToHost, sl.stream));
  return RTP_OK;
}

}  // namespace eng
}  // namespace rtp

extern "C" {

// The form of the assignment and the workgroup's size, kernels.h RTP_TRACK_* (idle engine; not part of the public header —
// tools/bench_track.py times all four, tests/test_track.py holds all four to rtp_track_update).  Returns the previous value.
extern "C" int rtp_internal_track_variant(rtp_engine* e, int variant) {
  static const char* fn = "rtp_internal_track_variant";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (variant < 0 || variant >= RTP_TRACK_VARIANTS) return fail(e, RTP_EINVAL, "%s: variant %d outside 0 .. %d", fn, variant, RTP_TRACK_VARIANTS - 1);
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  const int before = e->track_variant;
  e->track_variant = variant;
  return before;
}

// The kernel alone (idle engine, context 0; not part of the public header — tools/bench_track.py): `people` people against the table
// as it stands, `launches` (at most 400: they are enqueued within 4 ms) launches back to back on the slot's stream between two events; the table is restored afterwards.
// *period_us = one launch's period.
extern "C" int rtp_internal_track_time(rtp_engine* e, const float* joints_host, int num_people, int launches, float* period_us) {
  static const char* fn = "rtp_internal_track_time";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!period_us || launches < 1 || launches > 400 || num_people < 0 || num_people > RTP_MAX_PEOPLE || (num_people > 0 && !joints_host)) return fail(e, RTP_EINVAL, "%s: bad argument", fn);
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if (num_people > 0) HIPCHK(e, hipMemcpy(sl.joints, joints_host, (size_t)num_people * e->plan.num_parts * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.num_people, &num_people, sizeof(int), hipMemcpyHostToDevice));
  if ((rc = track_ensure(e, cx, 1))) return rc;
  std::vector<unsigned char> keep(sizeof(rtp_track_state));
  HIPCHK(e, hipMemcpy(keep.data(), e->track_dev, keep.size(), hipMemcpyDeviceToHost));
  // appearance mode: the train runs the appearance form on the descriptors slot 0 holds (rtp_appearance_from_joints stages them) and
  // the descriptor table comes back with the track table
  std::vector<unsigned char> keep_appear(e->appear_on ? sizeof(AppearTable) : 0);
  if (e->appear_on) HIPCHK(e, hipMemcpy(keep_appear.data(), e->appear_dev, keep_appear.size(), hipMemcpyDeviceToHost));
  // (from here on every HIP status is kept in `s` and checked once everything is released)
  hipEvent_t ev[2] = {nullptr, nullptr};
  unsigned long long* hold = nullptr;
  hipError_t s = hipEventCreate(&ev[0]);
  if (s == hipSuccess) s = hipEventCreate(&ev[1]);
  if (s == hipSuccess) s = hipMalloc((void**)&hold, 2 * sizeof(unsigned long long));
  for (int i = 0; i < 3 && !rc && s == hipSuccess; ++i) rc = track_enqueue(e, cx, 0, sl.stream);   // warm-up
  // a wave that waits 4 ms holds the stream while the train is enqueued, so that the event pair brackets device work only
  if (s == hipSuccess) s = hipStreamSynchronize(sl.stream);
  if (s == hipSuccess && !rc) s = launch_queue_wait(400000, hold, sl.stream);
  if (s == hipSuccess && !rc) s = hipEventRecord(ev[0], sl.stream);
  for (int i = 0; i < launches && !rc && s == hipSuccess; ++i) rc = track_enqueue(e, cx, 0, sl.stream);
  if (s == hipSuccess && !rc) s = hipEventRecord(ev[1], sl.stream);
  if (s == hipSuccess && !rc) s = hipEventSynchronize(ev[1]);
  float ms = 0.f;
  if (s == hipSuccess && !rc) s = hipEventElapsedTime(&ms, ev[0], ev[1]);
  const hipError_t sync = hipStreamSynchronize(sl.stream);   // (nothing of the train is pending when the buffers go and the table comes back)
  if (s == hipSuccess) s = sync;
  for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
  if (hold) (void)hipFree(hold);
  const hipError_t back = hipMemcpy(e->track_dev, keep.data(), keep.size(), hipMemcpyHostToDevice);
  if (s == hipSuccess) s = back;
  if (e->appear_on) {
    const hipError_t back_appear = hipMemcpy(e->appear_dev, keep_appear.data(), keep_appear.size(), hipMemcpyHostToDevice);
    if (s == hipSuccess) s = back_appear;
  }
  if (rc) return rc;
  HIPCHK(e, s);
  *period_us = ms * 1e3f / (float)launches;
  return RTP_OK;
}

// The switch needs an idle engine, like crops mode's.  Nothing is changed by a refused call.
int rtp_set_tracking(rtp_engine* e, const rtp_track_config* cfg) {
  static const char* fn = "rtp_set_tracking";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (cfg) {
    if (cfg->struct_size != sizeof(rtp_track_config))
      return fail(e, RTP_EINVAL, "%s: rtp_track_config.struct_size is %u, this library's rtp_track_config has %zu bytes", fn, cfg->struct_size, sizeof(rtp_track_config));
    const char* bad = rtp_internal_track_check(cfg);
    if (bad) return fail(e, RTP_EINVAL, "%s: %s (min_score %g, min_parts %d, min_common %d, max_cost %g, max_misses %d)", fn, bad, (double)cfg->min_score, cfg->min_parts,
                         cfg->min_common, (double)cfg->max_cost, cfg->max_misses);
  }
  if (!cfg && e->appear_on) return fail(e, RTP_EINVAL, "%s: appearance mode is on and needs the tracker: rtp_set_track_appearance(e, NULL) first", fn);
  if (!cfg && e->smooth_on) return fail(e, RTP_EINVAL, "%s: smoothing mode is on and needs the tracker: rtp_set_smoothing(e, NULL) first", fn);
  if (!cfg && e->overlay_on) return fail(e, RTP_EINVAL, "%s: overlay mode is on and needs the tracker: rtp_set_track_overlay(e, NULL) first", fn);
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (!cfg && !e->track_on) return RTP_OK;
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  SYNC_GUARD;
  int rc;
  if ((rc = need_idle(e))) return rc;
  if (!cfg || !e->track_on) {
    // RTP_GRAPH_POST=1: the chains live inside the batch graphs while the mode is off and are launched eagerly while it is on (the
    // wait in front of the kernel names another event every frame): the graphs captured in the other state go
    if (cfg && (rc = table_reset(e))) return rc;   // off -> on: an empty state (first: a refusal here has changed nothing the engine uses)
    if (e->graph_post && (rc = invalidate_graphs(e))) return rc;
  }
  if (!cfg) {
    for (Ctx& cx : e->ctx)
      for (Slot& sl : cx.slot) sl.track.free();
    track_free(e);
  }
  e->track_on = cfg != nullptr;
  e->track_cfg = cfg ? *cfg : rtp_track_config{};
  return RTP_OK;
}

int rtp_track_reset(rtp_engine* e) {
  static const char* fn = "rtp_track_reset";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  return table_reset(e);
}

int rtp_track_get_state(rtp_engine* e, rtp_track_state* state) {
  static const char* fn = "rtp_track_get_state";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!state) return fail(e, RTP_EINVAL, "%s: NULL state", fn);
  SYNC_GUARD;
  HIPCHK(e, hipDeviceSynchronize());
  HIPCHK(e, hipMemcpy(state, e->track_dev, sizeof *state, hipMemcpyDeviceToHost));
  track_forget_chain(e);
  return RTP_OK;
}

int rtp_track_set_state(rtp_engine* e, const rtp_track_state* state) {
  static const char* fn = "rtp_track_set_state";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!state) return fail(e, RTP_EINVAL, "%s: NULL state", fn);
  if (state->struct_size != sizeof(rtp_track_state))
    return fail(e, RTP_EINVAL, "%s: rtp_track_state.struct_size is %u, this library's rtp_track_state has %zu bytes", fn, state->struct_size, sizeof(rtp_track_state));
  if (state->num_parts != e->plan.num_parts) return fail(e, RTP_EINVAL, "%s: the state has %d parts per person, the engine's model %d", fn, state->num_parts, e->plan.num_parts);
  SYNC_GUARD;
  HIPCHK(e, hipDeviceSynchronize());
  return table_upload(e, state);
}

// Every refusal but RTP_ERANGE happens before anything is waited for; the frame stays in the FIFO either way.
int rtp_peek_tracks(rtp_engine* e, uint64_t* tag, int* recs_host, int* num_recs, int capacity) {
  static const char* fn = "rtp_peek_tracks";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->track_on) return fail(e, RTP_EINVAL, "%s: tracking mode is off (rtp_set_tracking)", fn);
  if (!recs_host || !num_recs || capacity < 0) return fail(e, RTP_EINVAL, "%s: NULL recs_host or num_recs, or a negative capacity", fn);
  int rc, ci = 0, sj = 0;
  if ((rc = need_weights(e))) return rc;
  if ((rc = wait_oldest(e, &ci, &sj))) return rc;   // (refuses "nothing in flight" before it waits)
  const Slot& sl = e->ctx[ci].slot[sj];
  int people;
  memcpy(&people, sl.host_out, sizeof people);
  const int n = std::min(std::max(people, 0), RTP_MAX_PEOPLE);
  *num_recs = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, the frame has %d records", fn, capacity, n);
  memcpy(recs_host, sl.track.recs_host, (size_t)n * RTP_TRACK_REC_INTS * sizeof(int));
  if (tag) *tag = sl.tag;
  return RTP_OK;
}

// Parity tap: the kernel of the async path on caller-supplied joints, context 0, slot 0; the engine's table advances by one frame
int rtp_track_from_joints(rtp_engine* e, const float* joints_host, int num_people, int* recs_host, int* num_recs, int capacity) {
  static const char* fn = "rtp_track_from_joints";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->track_on) return fail(e, RTP_EINVAL, "%s: tracking mode is off (rtp_set_tracking)", fn);
  // (num_people goes to the device as it is: above RTP_MAX_PEOPLE and negative values are what the kernel has to clamp)
  const int n = std::min(std::max(num_people, 0), RTP_MAX_PEOPLE);
  if (!recs_host || !num_recs || capacity < 0 || (n > 0 && !joints_host)) return fail(e, RTP_EINVAL, "%s: NULL recs_host, num_recs or joints, or a negative capacity", fn);
  *num_recs = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, %d records", fn, capacity, n);
  int rc;
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  if ((rc = need_idle(e))) return rc;
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if (n > 0) HIPCHK(e, hipMemcpy(sl.joints, joints_host, (size_t)n * e->plan.num_parts * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.num_people, &num_people, sizeof(int), hipMemcpyHostToDevice));
  if ((rc = track_ensure(e, cx, 1))) return rc;
  if ((rc = track_launch(e, cx, 0))) return rc;
  HIPCHK(e, hipStreamSynchronize(sl.stream));
  track_forget_chain(e);   // (complete: the next frame waits on nothing)
  memcpy(recs_host, sl.track.recs_host, (size_t)n * RTP_TRACK_REC_INTS * sizeof(int));
  return RTP_OK;
}

}  // extern "C"

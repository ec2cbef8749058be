// engine_appearance.cpp — the engine's side of appearance-aided tracking (appearance.hip, track.hip's appearance form): the mode
// switch, the device-resident descriptor table, the per-slot descriptor buffers, the describe kernel each submitted frame's chain gains
// while the mode is on, the peek entry, the state entries and the two parity taps.  Descriptors, records and both tables are
// rtp_appearance_describe's and rtp_track_update_appearance's (host_util.cpp) integer for integer and bit for bit.
//
// ORDERING.  The describe kernel is stateless: it runs on the frame's own stream behind the connect kernels and IN FRONT OF the wait on
// the previous frame's table event (track_launch enqueues that wait), so it overlaps the previous frame's chain.  The descriptor table
// is read and written by the track kernel alone, in the same launch that reads and writes the track table: the tracker's one chain of
// events (engine_track.cpp: ORDERING) orders it, and no event of its own is needed.
#include "engine_internal.h"

static_assert(sizeof(AppearTable) == sizeof(rtp_appearance_state), "AppearTable is rtp_appearance_state's layout");
static_assert(offsetof(AppearTable, owner) == offsetof(rtp_appearance_state, owner) && offsetof(AppearTable, desc) == offsetof(rtp_appearance_state, desc) &&
              offsetof(AppearTable, desc) % 16 == 0, "AppearTable is rtp_appearance_state's layout");
static_assert(RTP_APPEAR_BINS == RTP_APPEARANCE_BINS && RTP_APPEAR_GRID == RTP_APPEARANCE_GRID, "kernels.h mirrors the header");

namespace rtp {
namespace eng __attribute__((visibility("hidden"))) {

namespace {

constexpr size_t kBinsBytes = (size_t)RTP_MAX_PEOPLE * RTP_APPEARANCE_BINS * sizeof(uint16_t);
constexpr size_t kBlockBytes = kBinsBytes + RTP_MAX_PEOPLE;   // [bins][valid]

// the describe kernel on slot sj's joints and `src` (nullptr: no display image) -> the slot's block, on `stream`
int describe_enqueue(rtp_engine* e, Ctx& cx, int sj, const unsigned char* src, hipStream_t stream) {
  Slot& sl = cx.slot[sj];
  const rtp_appearance_config& c = e->appear_cfg;
  AppearDescribeParams p;
  memset(&p, 0, sizeof p);
  p.src = src; p.w = e->cfg.disp_w; p.h = e->cfg.disp_h;
  p.joints = sl.joints; p.num_people = sl.num_people;
  p.bins = reinterpret_cast<unsigned short*>(sl.appear.dev); p.valid = sl.appear.dev + kBinsBytes;
  p.num_parts = e->plan.num_parts; p.nlist = (int)e->appear_list.size(); p.min_parts = c.min_parts;
  p.min_score = c.min_score; p.margin = c.margin;
  for (int i = 0; i < p.nlist; ++i) p.list[i] = (unsigned char)e->appear_list[i];
  HIPCHK(e, launch_appear_describe(p, stream));   // no residency stamp: every slot of a frame's chain is taken (StampKind)
  return RTP_OK;
}

// an empty table (or the caller's) into the device copy; the engine is idle
int table_upload(rtp_engine* e, const rtp_appearance_state* st) {
  SYNC_GUARD;
  if (!e->appear_dev) HIPCHK(e, hipMalloc((void**)&e->appear_dev, sizeof(AppearTable)));
  HIPCHK(e, hipMemcpy(e->appear_dev, st, sizeof *st, hipMemcpyHostToDevice));
  track_forget_chain(e);
  return RTP_OK;
}

int table_reset(rtp_engine* e) {
  std::vector<unsigned char> buf(sizeof(rtp_appearance_state));
  rtp_appearance_state* st = reinterpret_cast<rtp_appearance_state*>(buf.data());
  rtp_appearance_state_init(st);
  return table_upload(e, st);
}

// what the state entries and the taps refuse: mode off, frames in flight, a busy device
int state_checks(rtp_engine* e, const char* fn) {
  if (!e->appear_on) return fail(e, RTP_EINVAL, "%s: appearance mode is off (rtp_set_track_appearance)", fn);
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  return need_idle(e);
}

// caller data into context 0, slot 0 (idle engine): the joints, num_people as it is, and the display image (nullptr: none)
int stage_tap(rtp_engine* e, const unsigned char* display_bgr_host, const float* joints_host, int num_people, int n) {
  Slot& sl = e->ctx[0].slot[0];
  if (display_bgr_host) {
    const size_t dbytes = (size_t)e->cfg.disp_w * e->cfg.disp_h * 3;
    if (!sl.disp_dev) HIPCHK(e, hipMalloc((void**)&sl.disp_dev, dbytes));
    HIPCHK(e, hipMemcpy(sl.disp_dev, display_bgr_host, dbytes, hipMemcpyHostToDevice));
    sl.disp_cur = sl.disp_dev;
  }
  if (n > 0) HIPCHK(e, hipMemcpy(sl.joints, joints_host, (size_t)n * e->plan.num_parts * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.num_people, &num_people, sizeof(int), hipMemcpyHostToDevice));
  return RTP_OK;
}

void copy_out(const Slot& sl, int n, uint16_t* bins_host, unsigned char* valid_host) {
  memcpy(bins_host, sl.appear.host, (size_t)n * RTP_APPEARANCE_BINS * sizeof(uint16_t));
  memcpy(valid_host, sl.appear.host + kBinsBytes, (size_t)n);
}

}  // namespace

void AppearOut::free() {
  if (dev) (void)hipFree(dev);
  if (host) (void)hipHostFree(host);
  dev = host = nullptr;
  fresh = false;
}

void appear_free(rtp_engine* e) {
  if (e->appear_dev) (void)hipFree(e->appear_dev);
  e->appear_dev = nullptr;
}

// The descriptor blocks of the first nframes slots, before their batch is launched (frame_outputs_ensure, track_ensure for the taps)
int appear_ensure(rtp_engine* e, Ctx& cx, int nframes) {
  for (int j = 0; j < nframes; ++j) {
    AppearOut& a = cx.slot[j].appear;
    if (a.dev) continue;
    SYNC_GUARD;
    HIPCHK(e, hipMalloc((void**)&a.dev, kBlockBytes));
    HIPCHK(e, hipMemset(a.dev, 0, kBlockBytes));   // (rtp_internal_track_time may run the appearance form before anything has described the slot: nobody valid)
    HIPCHK(e, hipHostMalloc((void**)&a.host, kBlockBytes, hipHostMallocDefault));
  }
  return RTP_OK;
}

int appear_launch(rtp_engine* e, Ctx& cx, int sj, bool with_image) {
  Slot& sl = cx.slot[sj];
  int rc;
  if ((rc = describe_enqueue(e, cx, sj, with_image ? sl.disp_cur : nullptr, sl.stream))) return rc;
  HIPCHK(e, hipMemcpyAsync(sl.appear.host, sl.appear.dev, kBlockBytes, hipMemcpyDeviceToHost, sl.stream));
  sl.appear.fresh = true;
  return RTP_OK;
}

void appear_track_params(const rtp_engine* e, const Slot& sl, TrackAppearParams* a) {
  const rtp_appearance_config& c = e->appear_cfg;
  a->bins = reinterpret_cast<const unsigned short*>(sl.appear.dev);
  a->valid = sl.appear.dev ? sl.appear.dev + kBinsBytes : nullptr;
  a->table = e->appear_dev;
  a->weight = c.weight; a->max_dist = c.max_dist; a->unknown = c.unknown;
  a->rate = c.rate;
}

}  // namespace eng
}  // namespace rtp

extern "C" {

// The describe kernel alone (idle engine, context 0; not part of the public header — tools/bench_appearance.py): caller data as in
// rtp_appearance_from_joints, `launches` (at most 400: they are enqueued within 4 ms) launches back to back on the slot's stream
// between two events; *period_us = one launch's period.
extern "C" int rtp_internal_appearance_time(rtp_engine* e, const unsigned char* display_bgr_host, const float* joints_host, int num_people, int launches, float* period_us) {
  static const char* fn = "rtp_internal_appearance_time";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!display_bgr_host || !period_us || launches < 1 || launches > 400 || num_people < 0 || num_people > RTP_MAX_PEOPLE || (num_people > 0 && !joints_host))
    return fail(e, RTP_EINVAL, "%s: bad argument", fn);
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if ((rc = stage_tap(e, display_bgr_host, joints_host, num_people, num_people)) || (rc = appear_ensure(e, cx, 1))) return rc;
  hipEvent_t ev[2] = {nullptr, nullptr};
  unsigned long long* hold = nullptr;
  hipError_t s = hipEventCreate(&ev[0]);
  if (s == hipSuccess) s = hipEventCreate(&ev[1]);
  if (s == hipSuccess) s = hipMalloc((void**)&hold, 2 * sizeof(unsigned long long));
  for (int i = 0; i < 3 && !rc && s == hipSuccess; ++i) rc = describe_enqueue(e, cx, 0, sl.disp_cur, sl.stream);   // warm-up
  // a wave that waits 4 ms holds the stream while the train is enqueued, so that the event pair brackets device work only
  if (s == hipSuccess) s = hipStreamSynchronize(sl.stream);
  if (s == hipSuccess && !rc) s = launch_queue_wait(400000, hold, sl.stream);
  if (s == hipSuccess && !rc) s = hipEventRecord(ev[0], sl.stream);
  for (int i = 0; i < launches && !rc && s == hipSuccess; ++i) rc = describe_enqueue(e, cx, 0, sl.disp_cur, sl.stream);
  if (s == hipSuccess && !rc) s = hipEventRecord(ev[1], sl.stream);
  if (s == hipSuccess && !rc) s = hipEventSynchronize(ev[1]);
  float ms = 0.f;
  if (s == hipSuccess && !rc) s = hipEventElapsedTime(&ms, ev[0], ev[1]);
  const hipError_t sync = hipStreamSynchronize(sl.stream);
  if (s == hipSuccess) s = sync;
  for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
  if (hold) (void)hipFree(hold);
  if (rc) return rc;
  HIPCHK(e, s);
  *period_us = ms * 1e3f / (float)launches;
  return RTP_OK;
}

// The switch needs an idle engine, like smoothing's.  Nothing is changed by a refused call.  While tracking mode is on the frames'
// chains are launched eagerly under the experiments build's RTP_GRAPH_POST=1 too (rtp_set_tracking dropped the graphs that held them),
// so no captured graph holds a kernel of either state of this mode.
int rtp_set_track_appearance(rtp_engine* e, const rtp_appearance_config* cfg) {
  static const char* fn = "rtp_set_track_appearance";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  std::vector<int> list;
  if (cfg) {
    if (cfg->struct_size != sizeof(rtp_appearance_config))
      return fail(e, RTP_EINVAL, "%s: rtp_appearance_config.struct_size is %u, this library's rtp_appearance_config has %zu bytes", fn, cfg->struct_size,
                  sizeof(rtp_appearance_config));
    const char* bad = rtp_internal_appearance_check(cfg, e->plan.num_parts);
    if (bad) return fail(e, RTP_EINVAL, "%s: %s (num_parts %d, min_score %g, min_parts %d, margin %g, weight %g, max_dist %g, unknown %g, rate %d)", fn, bad, cfg->num_parts,
                         (double)cfg->min_score, cfg->min_parts, (double)cfg->margin, (double)cfg->weight, (double)cfg->max_dist, (double)cfg->unknown, cfg->rate);
    if (!e->track_on) return fail(e, RTP_EINVAL, "%s: tracking mode is off (rtp_set_tracking first)", fn);
    int l[RTP_MAX_NUM_PARTS];
    const int nl = rtp_internal_appearance_list(cfg, e->plan.num_parts, l);
    list.assign(l, l + nl);
  }
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (!cfg && !e->appear_on) return RTP_OK;
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  SYNC_GUARD;
  int rc;
  if ((rc = need_idle(e))) return rc;
  if (cfg && !e->appear_on && (rc = table_reset(e))) return rc;   // off -> on: an empty descriptor table; the track table is kept
  if (!cfg) {
    for (Ctx& cx : e->ctx)
      for (Slot& sl : cx.slot) sl.appear.free();
    appear_free(e);
  }
  e->appear_on = cfg != nullptr;
  e->appear_cfg = cfg ? *cfg : rtp_appearance_config{};
  e->appear_cfg.parts = nullptr;
  e->appear_cfg.num_parts = (int)list.size();
  e->appear_list = list;
  return RTP_OK;
}

int rtp_appearance_reset(rtp_engine* e) {
  static const char* fn = "rtp_appearance_reset";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  return table_reset(e);
}

int rtp_appearance_get_state(rtp_engine* e, rtp_appearance_state* state) {
  static const char* fn = "rtp_appearance_get_state";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!state) return fail(e, RTP_EINVAL, "%s: NULL state", fn);
  SYNC_GUARD;
  HIPCHK(e, hipDeviceSynchronize());
  HIPCHK(e, hipMemcpy(state, e->appear_dev, sizeof *state, hipMemcpyDeviceToHost));
  track_forget_chain(e);
  return RTP_OK;
}

int rtp_appearance_set_state(rtp_engine* e, const rtp_appearance_state* state) {
  static const char* fn = "rtp_appearance_set_state";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!state) return fail(e, RTP_EINVAL, "%s: NULL state", fn);
  if (state->struct_size != sizeof(rtp_appearance_state))
    return fail(e, RTP_EINVAL, "%s: rtp_appearance_state.struct_size is %u, this library's rtp_appearance_state has %zu bytes", fn, state->struct_size,
                sizeof(rtp_appearance_state));
  SYNC_GUARD;
  HIPCHK(e, hipDeviceSynchronize());
  return table_upload(e, state);
}

// Every refusal but RTP_ERANGE happens before anything is waited for; the frame stays in the FIFO either way.
int rtp_peek_appearance(rtp_engine* e, uint64_t* tag, uint16_t* bins_host, unsigned char* valid_host, int* num, int capacity) {
  static const char* fn = "rtp_peek_appearance";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->appear_on) return fail(e, RTP_EINVAL, "%s: appearance mode is off (rtp_set_track_appearance)", fn);
  if (!bins_host || !valid_host || !num || capacity < 0) return fail(e, RTP_EINVAL, "%s: NULL bins_host, valid_host or num, or a negative capacity", fn);
  int rc, ci = 0, sj = 0;
  if ((rc = need_weights(e))) return rc;
  if ((rc = wait_oldest(e, &ci, &sj))) return rc;   // (refuses "nothing in flight" before it waits)
  const Slot& sl = e->ctx[ci].slot[sj];
  int people;
  memcpy(&people, sl.host_out, sizeof people);
  const int n = std::min(std::max(people, 0), RTP_MAX_PEOPLE);
  *num = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, the frame has %d descriptors", fn, capacity, n);
  copy_out(sl, n, bins_host, valid_host);
  if (tag) *tag = sl.tag;
  return RTP_OK;
}

// Parity tap: the describe kernel of the async path on caller-supplied joints and display image, context 0, slot 0; no table is touched
int rtp_appearance_from_joints(rtp_engine* e, const unsigned char* display_bgr_host, const float* joints_host, int num_people, uint16_t* bins_host,
                               unsigned char* valid_host, int* num, int capacity) {
  static const char* fn = "rtp_appearance_from_joints";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->appear_on) return fail(e, RTP_EINVAL, "%s: appearance mode is off (rtp_set_track_appearance)", fn);
  // (num_people goes to the device as it is: above RTP_MAX_PEOPLE and negative values are what the kernel has to clamp)
  const int n = std::min(std::max(num_people, 0), RTP_MAX_PEOPLE);
  if (!bins_host || !valid_host || !num || capacity < 0 || (n > 0 && !joints_host))
    return fail(e, RTP_EINVAL, "%s: NULL bins_host, valid_host, num or joints, or a negative capacity", fn);
  *num = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, %d descriptors", fn, capacity, n);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if ((rc = stage_tap(e, display_bgr_host, joints_host, num_people, n)) || (rc = appear_ensure(e, cx, 1))) return rc;
  if ((rc = appear_launch(e, cx, 0, display_bgr_host != nullptr))) return rc;
  HIPCHK(e, hipStreamSynchronize(sl.stream));
  sl.appear.fresh = false;
  copy_out(sl, n, bins_host, valid_host);
  return RTP_OK;
}

// Parity tap: the describe kernel and the track kernel's appearance form of the async path on caller data, context 0, slot 0; the
// engine's two tables advance by one frame
int rtp_track_from_frame(rtp_engine* e, const unsigned char* display_bgr_host, const float* joints_host, int num_people, int* recs_host,
                         uint16_t* bins_host, unsigned char* valid_host, int* num, int capacity) {
  static const char* fn = "rtp_track_from_frame";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->appear_on) return fail(e, RTP_EINVAL, "%s: appearance mode is off (rtp_set_track_appearance)", fn);
  const int n = std::min(std::max(num_people, 0), RTP_MAX_PEOPLE);
  if (!recs_host || !num || capacity < 0 || (n > 0 && !joints_host) || (bins_host != nullptr) != (valid_host != nullptr))
    return fail(e, RTP_EINVAL, "%s: NULL recs_host, num or joints, bins_host without valid_host, or a negative capacity", fn);
  *num = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, %d records", fn, capacity, n);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if ((rc = stage_tap(e, display_bgr_host, joints_host, num_people, n)) || (rc = track_ensure(e, cx, 1))) return rc;
  if ((rc = appear_launch(e, cx, 0, display_bgr_host != nullptr))) return rc;
  if ((rc = track_launch(e, cx, 0))) return rc;
  HIPCHK(e, hipStreamSynchronize(sl.stream));
  track_forget_chain(e);   // (complete: the next frame waits on nothing)
  memcpy(recs_host, sl.track.recs_host, (size_t)n * RTP_TRACK_REC_INTS * sizeof(int));
  if (bins_host) copy_out(sl, n, bins_host, valid_host);
  return RTP_OK;
}

}  // extern "C"

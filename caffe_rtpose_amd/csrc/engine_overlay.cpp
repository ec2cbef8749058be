// engine_overlay.cpp — the engine's side of overlay mode (overlay.hip): the mode switch, the device-resident trail table, the per-slot
// draw list, the two kernels each submitted frame's chain gains while the mode is on, the peek entry, the state entries and the
// parity tap.  List, table and pixels are rtp_overlay_update's and rtp_overlay_draw's (host_util.cpp) integer for integer and byte
// for byte.
//
// The trail table is one per engine and is updated in submit order, like the track table, and by the same chain of events
// (engine_track.cpp: ORDERING): while the mode is on, the event the next frame's track kernel waits on is recorded behind this
// frame's UPDATE kernel, the last table kernel of its chain.  The DRAW kernel reads only what the slot owns (its list, its rendered
// image), so it is not part of that chain: the next frame's table kernels may run while it draws.
#include "engine_internal.h"

static_assert(sizeof(TrailTable) == sizeof(rtp_trail_state) && sizeof(TrailSlot) == sizeof(rtp_trail_slot), "TrailTable is rtp_trail_state's layout");
static_assert(offsetof(TrailTable, num_parts) == offsetof(rtp_trail_state, num_parts) && offsetof(TrailTable, frames) == offsetof(rtp_trail_state, frames) &&
              offsetof(TrailTable, slot) == offsetof(rtp_trail_state, slot), "TrailTable is rtp_trail_state's layout");
static_assert(offsetof(TrailSlot, owner) == offsetof(rtp_trail_slot, owner) && offsetof(TrailSlot, count) == offsetof(rtp_trail_slot, count) &&
              offsetof(TrailSlot, head) == offsetof(rtp_trail_slot, head) && offsetof(TrailSlot, pts) == offsetof(rtp_trail_slot, pts), "TrailSlot is rtp_trail_slot's layout");
static_assert(RTP_OVL_TRAIL_MAX == RTP_TRAIL_MAX && RTP_OVL_ITEM_INTS == RTP_OVERLAY_ITEM_INTS && RTP_OVL_MAX_ITEMS == RTP_OVERLAY_MAX_ITEMS, "kernels.h mirrors the header");

namespace rtp {
namespace eng __attribute__((visibility("hidden"))) {

namespace {

constexpr size_t kListInts = (size_t)RTP_OVERLAY_MAX_ITEMS * RTP_OVERLAY_ITEM_INTS;   // the list; its length is the int behind it
constexpr size_t kListBytes = (kListInts + 1) * sizeof(int);
const int kPalette[16] = RTP_OVERLAY_PALETTE;
const unsigned char kFont[10][7] = RTP_OVERLAY_FONT;

// the update kernel on the joints `poses` and slot sj's records -> the slot's draw list, on `stream`
int update_enqueue(rtp_engine* e, Ctx& cx, int sj, const float* poses, hipStream_t stream) {
  Slot& sl = cx.slot[sj];
  const rtp_overlay_config& c = e->overlay_cfg;
  OverlayUpdateParams p;
  memset(&p, 0, sizeof p);
  p.joints = poses; p.num_people = sl.num_people; p.recs = sl.track.recs_dev;
  p.table = e->overlay_dev;
  p.items = sl.overlay.dev; p.num_items = sl.overlay.dev + kListInts;
  p.num_parts = e->plan.num_parts; p.what = c.what; p.min_score = c.min_score;
  p.box_margin = c.box_margin; p.line_width = c.line_width; p.label_scale = c.label_scale; p.trail_len = c.trail_len;
  p.trail_radius = c.trail_radius; p.alpha = c.alpha;
  memcpy(p.palette, kPalette, sizeof kPalette);
  HIPCHK(e, launch_overlay_update(p, stream));   // no residency stamp: every slot of a frame's chain is taken (StampKind)
  return RTP_OK;
}

// the draw kernel: slot sj's list into `image` (w x h, dense), on `stream`
int draw_enqueue(rtp_engine* e, Ctx& cx, int sj, unsigned char* image, int w, int h, hipStream_t stream) {
  Slot& sl = cx.slot[sj];
  OverlayDrawParams p;
  memset(&p, 0, sizeof p);
  p.items = sl.overlay.dev; p.num_items = sl.overlay.dev + kListInts;
  p.image = image; p.w = w; p.h = h; p.stride = 3L * w;
  memcpy(p.font, kFont, sizeof kFont);
  HIPCHK(e, launch_overlay_draw(p, stream));
  return RTP_OK;
}

// an empty table (or the caller's) into the device copy; the engine is idle
int table_upload(rtp_engine* e, const rtp_trail_state* st) {
  SYNC_GUARD;
  if (!e->overlay_dev) HIPCHK(e, hipMalloc((void**)&e->overlay_dev, sizeof(TrailTable)));
  HIPCHK(e, hipMemcpy(e->overlay_dev, st, sizeof *st, hipMemcpyHostToDevice));
  track_forget_chain(e);
  return RTP_OK;
}

int table_reset(rtp_engine* e) {
  std::vector<unsigned char> buf(sizeof(rtp_trail_state));
  rtp_trail_state* st = reinterpret_cast<rtp_trail_state*>(buf.data());
  if (rtp_trail_state_init(st, e->plan.num_parts) != RTP_OK) return fail(e, RTP_EINVAL, "overlay: the model has %d parts", e->plan.num_parts);
  return table_upload(e, st);
}

// what the state entries refuse: mode off, frames in flight, a busy device
int state_checks(rtp_engine* e, const char* fn) {
  if (!e->overlay_on) return fail(e, RTP_EINVAL, "%s: overlay mode is off (rtp_set_track_overlay)", fn);
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  return need_idle(e);
}

}  // namespace

void OverlayOut::free() {
  if (dev) (void)hipFree(dev);
  if (host) (void)hipHostFree(host);
  dev = host = nullptr;
}

void overlay_free(rtp_engine* e) {
  if (e->overlay_dev) (void)hipFree(e->overlay_dev);
  e->overlay_dev = nullptr;
}

// The draw lists of the first nframes slots, before their batch is launched (frame_outputs_ensure, and the tap)
int overlay_ensure(rtp_engine* e, Ctx& cx, int nframes) {
  for (int j = 0; j < nframes; ++j) {
    OverlayOut& o = cx.slot[j].overlay;
    if (o.dev) continue;
    SYNC_GUARD;
    HIPCHK(e, hipMalloc((void**)&o.dev, kListBytes));
    HIPCHK(e, hipHostMalloc((void**)&o.host, kListBytes, hipHostMallocDefault));
  }
  return RTP_OK;
}

// frame_outputs_launch: frame sj's update on the frame's own stream behind its track (and smooth) kernel, the event the next frame's
// chain waits on behind it, and the list with its length -> pinned memory in front of the frame's last event
int overlay_update_launch(rtp_engine* e, Ctx& cx, int sj, const float* poses) {
  Slot& sl = cx.slot[sj];
  int rc;
  if ((rc = update_enqueue(e, cx, sj, poses, sl.stream))) return rc;
  HIPCHK(e, hipEventRecord(sl.track.ev, sl.stream));
  e->track_prev = sl.track.ev;
  e->track_prev_stream = sl.stream;
  HIPCHK(e, hipMemcpyAsync(sl.overlay.host, sl.overlay.dev, kListBytes, hipMemcpyDeviceToHost, sl.stream));
  return RTP_OK;
}

// frame_outputs_launch: frame sj's list into its rendered image, behind the pose overlay and in front of the image's export
int overlay_draw_launch(rtp_engine* e, Ctx& cx, int sj) {
  Slot& sl = cx.slot[sj];
  return draw_enqueue(e, cx, sj, sl.render.dev, e->cfg.disp_w, e->cfg.disp_h, sl.stream);
}

}  // namespace eng
}  // namespace rtp

extern "C" {

// One of the two kernels alone (idle engine, context 0; not part of the public header — tools/bench_overlay.py): `people` people with
// their records against the table as it stands, `launches` (at most 400: they are enqueued within 4 ms) launches back to back on the
// slot's stream between two events; the table is restored afterwards.  draw == 0: the update kernel; draw != 0: one update, then the
// draw kernel on the slot's rendered image (display size).  *period_us = one launch's period, *num_items = the list's length.
extern "C" int rtp_internal_overlay_time(rtp_engine* e, const float* joints_host, const int* recs_host, int num_people, int draw, int launches, float* period_us,
                                         int* num_items) {
  static const char* fn = "rtp_internal_overlay_time";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!period_us || launches < 1 || launches > 400 || num_people < 0 || num_people > RTP_MAX_PEOPLE || (num_people > 0 && (!joints_host || !recs_host)))
    return fail(e, RTP_EINVAL, "%s: bad argument", fn);
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if ((rc = track_ensure(e, cx, 1)) || (rc = overlay_ensure(e, cx, 1))) return rc;
  if (num_people > 0) {
    HIPCHK(e, hipMemcpy(sl.joints, joints_host, (size_t)num_people * e->plan.num_parts * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(sl.track.recs_dev, recs_host, (size_t)num_people * RTP_TRACK_REC_INTS * sizeof(int), hipMemcpyHostToDevice));
  }
  HIPCHK(e, hipMemcpy(sl.num_people, &num_people, sizeof(int), hipMemcpyHostToDevice));
  std::vector<unsigned char> keep(sizeof(rtp_trail_state));
  HIPCHK(e, hipMemcpy(keep.data(), e->overlay_dev, keep.size(), hipMemcpyDeviceToHost));
  auto one = [&]() { return draw ? draw_enqueue(e, cx, 0, sl.render.dev, e->cfg.disp_w, e->cfg.disp_h, sl.stream) : update_enqueue(e, cx, 0, sl.joints, sl.stream); };
  if (draw && (rc = update_enqueue(e, cx, 0, sl.joints, sl.stream))) return rc;
  // (from here on every HIP status is kept in `s` and checked once everything is released)
  hipEvent_t ev[2] = {nullptr, nullptr};
  unsigned long long* hold = nullptr;
  hipError_t s = hipEventCreate(&ev[0]);
  if (s == hipSuccess) s = hipEventCreate(&ev[1]);
  if (s == hipSuccess) s = hipMalloc((void**)&hold, 2 * sizeof(unsigned long long));
  for (int i = 0; i < 3 && !rc && s == hipSuccess; ++i) rc = one();   // warm-up
  // a wave that waits 4 ms holds the stream while the train is enqueued, so that the event pair brackets device work only
  if (s == hipSuccess) s = hipStreamSynchronize(sl.stream);
  if (s == hipSuccess && !rc) s = launch_queue_wait(400000, hold, sl.stream);
  if (s == hipSuccess && !rc) s = hipEventRecord(ev[0], sl.stream);
  for (int i = 0; i < launches && !rc && s == hipSuccess; ++i) rc = one();
  if (s == hipSuccess && !rc) s = hipEventRecord(ev[1], sl.stream);
  if (s == hipSuccess && !rc) s = hipEventSynchronize(ev[1]);
  float ms = 0.f;
  if (s == hipSuccess && !rc) s = hipEventElapsedTime(&ms, ev[0], ev[1]);
  const hipError_t sync = hipStreamSynchronize(sl.stream);   // (nothing of the train is pending when the buffers go and the table comes back)
  if (s == hipSuccess) s = sync;
  for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
  if (hold) (void)hipFree(hold);
  int items = 0;
  const hipError_t got = hipMemcpy(&items, sl.overlay.dev + kListInts, sizeof(int), hipMemcpyDeviceToHost);
  if (s == hipSuccess) s = got;
  const hipError_t back = hipMemcpy(e->overlay_dev, keep.data(), keep.size(), hipMemcpyHostToDevice);
  if (s == hipSuccess) s = back;
  if (rc) return rc;
  HIPCHK(e, s);
  *period_us = ms * 1e3f / (float)launches;
  if (num_items) *num_items = items;
  return RTP_OK;
}

// The draw kernel alone on a caller's list (idle engine, context 0, mode on; not part of the public header — tests/test_overlay.py runs
// hand-written lists through it: kinds that do not exist, fields out of their range, every label scale): items_host [num_items][9]
// into image_host_in_out, dense w x h BGR up to the display size.  num_items goes to the device as it is (the kernel clamps it); at
// most RTP_OVERLAY_MAX_ITEMS items are uploaded.  No table is touched.
extern "C" int rtp_internal_overlay_draw_list(rtp_engine* e, const int* items_host, int num_items, unsigned char* image_host_in_out, int w, int h) {
  static const char* fn = "rtp_internal_overlay_draw_list";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  const int n = std::min(std::max(num_items, 0), (int)RTP_OVERLAY_MAX_ITEMS);
  if (!image_host_in_out || (n > 0 && !items_host) || w < 1 || h < 1 || w > e->cfg.disp_w || h > e->cfg.disp_h) return fail(e, RTP_EINVAL, "%s: bad argument", fn);
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if (!sl.render.dev) return fail(e, RTP_EINVAL, "%s: the engine does not render", fn);
  if ((rc = overlay_ensure(e, cx, 1))) return rc;
  if (n > 0) HIPCHK(e, hipMemcpy(sl.overlay.dev, items_host, (size_t)n * RTP_OVERLAY_ITEM_INTS * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.overlay.dev + kListInts, &num_items, sizeof(int), hipMemcpyHostToDevice));
  const size_t ibytes = (size_t)w * h * 3;
  HIPCHK(e, hipMemcpy(sl.render.dev, image_host_in_out, ibytes, hipMemcpyHostToDevice));
  if ((rc = draw_enqueue(e, cx, 0, sl.render.dev, w, h, sl.stream))) return rc;
  HIPCHK(e, hipStreamSynchronize(sl.stream));
  HIPCHK(e, hipMemcpy(image_host_in_out, sl.render.dev, ibytes, hipMemcpyDeviceToHost));
  return RTP_OK;
}

// The switch needs an idle engine, like smoothing's.  Nothing is changed by a refused call.
int rtp_set_track_overlay(rtp_engine* e, const rtp_overlay_config* cfg) {
  static const char* fn = "rtp_set_track_overlay";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (cfg) {
    if (cfg->struct_size != sizeof(rtp_overlay_config))
      return fail(e, RTP_EINVAL, "%s: rtp_overlay_config.struct_size is %u, this library's rtp_overlay_config has %zu bytes", fn, cfg->struct_size, sizeof(rtp_overlay_config));
    const char* bad = rtp_internal_overlay_check(cfg);
    if (bad) return fail(e, RTP_EINVAL, "%s: %s (what %u, min_score %g, box_margin %d, line_width %d, label_scale %d, trail_len %d, trail_radius %d, alpha %d)", fn, bad, cfg->what,
                         (double)cfg->min_score, cfg->box_margin, cfg->line_width, cfg->label_scale, cfg->trail_len, cfg->trail_radius, cfg->alpha);
    if (!e->track_on) return fail(e, RTP_EINVAL, "%s: tracking mode is off (rtp_set_tracking first)", fn);
    if (!e->cfg.render) return fail(e, RTP_EINVAL, "%s: the engine does not render (rtp_config.render is 0): there is no image to draw into", fn);
  }
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (!cfg && !e->overlay_on) return RTP_OK;
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  SYNC_GUARD;
  int rc;
  if ((rc = need_idle(e))) return rc;
  if (cfg && !e->overlay_on && (rc = table_reset(e))) return rc;   // off -> on: an empty table
  if (!cfg) {
    for (Ctx& cx : e->ctx)
      for (Slot& sl : cx.slot) sl.overlay.free();
    overlay_free(e);
  }
  e->overlay_on = cfg != nullptr;
  e->overlay_cfg = cfg ? *cfg : rtp_overlay_config{};
  return RTP_OK;
}

int rtp_overlay_reset(rtp_engine* e) {
  static const char* fn = "rtp_overlay_reset";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  return table_reset(e);
}

int rtp_overlay_get_state(rtp_engine* e, rtp_trail_state* state) {
  static const char* fn = "rtp_overlay_get_state";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!state) return fail(e, RTP_EINVAL, "%s: NULL state", fn);
  SYNC_GUARD;
  HIPCHK(e, hipDeviceSynchronize());
  HIPCHK(e, hipMemcpy(state, e->overlay_dev, sizeof *state, hipMemcpyDeviceToHost));
  track_forget_chain(e);
  return RTP_OK;
}

int rtp_overlay_set_state(rtp_engine* e, const rtp_trail_state* state) {
  static const char* fn = "rtp_overlay_set_state";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc;
  if ((rc = state_checks(e, fn))) return rc;
  if (!state) return fail(e, RTP_EINVAL, "%s: NULL state", fn);
  if (state->struct_size != sizeof(rtp_trail_state))
    return fail(e, RTP_EINVAL, "%s: rtp_trail_state.struct_size is %u, this library's rtp_trail_state has %zu bytes", fn, state->struct_size, sizeof(rtp_trail_state));
  if (state->num_parts != e->plan.num_parts) return fail(e, RTP_EINVAL, "%s: the state has %d parts per person, the engine's model %d", fn, state->num_parts, e->plan.num_parts);
  const char* bad = rtp_internal_trail_check(state);
  if (bad) return fail(e, RTP_EINVAL, "%s: %s", fn, bad);
  SYNC_GUARD;
  HIPCHK(e, hipDeviceSynchronize());
  return table_upload(e, state);
}

// Every refusal but RTP_ERANGE happens before anything is waited for; the frame stays in the FIFO either way.
int rtp_peek_overlay_items(rtp_engine* e, uint64_t* tag, int* items_host, int* num_items, int capacity) {
  static const char* fn = "rtp_peek_overlay_items";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->overlay_on) return fail(e, RTP_EINVAL, "%s: overlay mode is off (rtp_set_track_overlay)", fn);
  if (!items_host || !num_items || capacity < 0) return fail(e, RTP_EINVAL, "%s: NULL items_host or num_items, or a negative capacity", fn);
  int rc, ci = 0, sj = 0;
  if ((rc = need_weights(e))) return rc;
  if ((rc = wait_oldest(e, &ci, &sj))) return rc;   // (refuses "nothing in flight" before it waits)
  const Slot& sl = e->ctx[ci].slot[sj];
  const int n = std::min(std::max(sl.overlay.host[kListInts], 0), (int)RTP_OVERLAY_MAX_ITEMS);
  *num_items = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, the frame has %d items", fn, capacity, n);
  memcpy(items_host, sl.overlay.host, (size_t)n * RTP_OVERLAY_ITEM_INTS * sizeof(int));
  if (tag) *tag = sl.tag;
  return RTP_OK;
}

// Parity tap: the kernels of the async path on caller data, context 0, slot 0; the track table and the trail table advance by one frame
int rtp_overlay_from_joints(rtp_engine* e, const float* joints_host, int num_people, unsigned char* image_host_in_out, int w, int h, int* recs_out, int* items_out,
                            int* num_items, int capacity) {
  static const char* fn = "rtp_overlay_from_joints";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->overlay_on) return fail(e, RTP_EINVAL, "%s: overlay mode is off (rtp_set_track_overlay)", fn);
  // (num_people goes to the device as it is: above RTP_MAX_PEOPLE and negative values are what the kernels have to clamp)
  const int n = std::min(std::max(num_people, 0), RTP_MAX_PEOPLE);
  if (!items_out || !num_items || capacity < 0 || (n > 0 && !joints_host)) return fail(e, RTP_EINVAL, "%s: NULL items_out, num_items or joints, or a negative capacity", fn);
  if (image_host_in_out && (w < 1 || h < 1 || w > e->cfg.disp_w || h > e->cfg.disp_h))
    return fail(e, RTP_EINVAL, "%s: the image is %d x %d, the engine's display size %d x %d", fn, w, h, e->cfg.disp_w, e->cfg.disp_h);
  int rc;
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  if ((rc = need_idle(e))) return rc;
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if (!sl.render.dev) return fail(e, RTP_EINVAL, "%s: the engine does not render", fn);
  if (n > 0) HIPCHK(e, hipMemcpy(sl.joints, joints_host, (size_t)n * e->plan.num_parts * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.num_people, &num_people, sizeof(int), hipMemcpyHostToDevice));
  if ((rc = track_ensure(e, cx, 1)) || (rc = overlay_ensure(e, cx, 1))) return rc;
  const size_t ibytes = image_host_in_out ? (size_t)w * h * 3 : 0;
  if (ibytes) HIPCHK(e, hipMemcpy(sl.render.dev, image_host_in_out, ibytes, hipMemcpyHostToDevice));
  if ((rc = track_launch(e, cx, 0, true))) return rc;
  if ((rc = overlay_update_launch(e, cx, 0, sl.joints))) return rc;
  if (ibytes && (rc = draw_enqueue(e, cx, 0, sl.render.dev, w, h, sl.stream))) return rc;
  HIPCHK(e, hipStreamSynchronize(sl.stream));
  track_forget_chain(e);   // (complete: the next frame waits on nothing)
  const int m = std::min(std::max(sl.overlay.host[kListInts], 0), (int)RTP_OVERLAY_MAX_ITEMS);
  *num_items = m;
  if (recs_out) memcpy(recs_out, sl.track.recs_host, (size_t)n * RTP_TRACK_REC_INTS * sizeof(int));
  if (capacity < m) return fail(e, RTP_ERANGE, "%s: capacity %d, the frame has %d items (both tables have advanced)", fn, capacity, m);
  memcpy(items_out, sl.overlay.host, (size_t)m * RTP_OVERLAY_ITEM_INTS * sizeof(int));
  if (ibytes) HIPCHK(e, hipMemcpy(image_host_in_out, sl.render.dev, ibytes, hipMemcpyDeviceToHost));
  return RTP_OK;
}

}  // extern "C"

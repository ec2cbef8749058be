// engine_redact.cpp — the engine's side of redaction mode (redact.hip): the mode switch, the per-slot records and scratch image, the
// kernels each submitted frame's chain gains while the mode is on, the peek entry and the parity tap.  Records and pixels are
// rtp_redact_regions' and rtp_redact_apply's (host_util.cpp) integer for integer and byte for byte.
//
// The mode has no table: both kernels read and write only what the frame's slot owns (its joints, its records, its rendered image, its
// scratch image), so there is no submit-order chain of its own and nothing here touches the tracker's events.
#include "engine_internal.h"

static_assert(RTP_RDC_REGION_INTS == RTP_REDACT_REGION_INTS && RTP_RDC_MAX_RADIUS == RTP_REDACT_MAX_RADIUS && RTP_TRACK_MAX_PEOPLE == RTP_MAX_PEOPLE &&
              RTP_TRACK_MAX_PARTS == RTP_MAX_NUM_PARTS, "kernels.h mirrors the header");
static_assert(RTP_RDC_MOSAIC == RTP_REDACT_MOSAIC && RTP_RDC_BLUR == RTP_REDACT_BLUR && RTP_RDC_FILL == RTP_REDACT_FILL, "kernels.h mirrors the header");

namespace rtp {
namespace eng __attribute__((visibility("hidden"))) {

namespace {

constexpr size_t kRecInts = (size_t)RTP_MAX_PEOPLE * RTP_REDACT_REGION_INTS;   // the records; their number is the int behind them
constexpr size_t kRecBytes = (kRecInts + 1) * sizeof(int);

// the regions kernel on the joints `poses` -> slot sj's records, on `stream`
int regions_enqueue(rtp_engine* e, Ctx& cx, int sj, const float* poses, hipStream_t stream) {
  Slot& sl = cx.slot[sj];
  const rtp_redact_config& c = e->redact_cfg;
  RedactRegionsParams p;
  memset(&p, 0, sizeof p);
  p.joints = poses; p.num_people = sl.num_people;
  p.regions = sl.redact.dev; p.num_regions = sl.redact.dev + kRecInts;
  p.num_parts = e->plan.num_parts; p.nlist = (int)e->redact_list.size(); p.min_parts = c.min_parts; p.min_score = c.min_score;
  p.scale_q8 = c.scale_q8; p.aspect_q8 = c.aspect_q8; p.pad = c.pad; p.min_radius = c.min_radius;
  for (int i = 0; i < p.nlist; ++i) p.list[i] = (unsigned char)e->redact_list[i];
  HIPCHK(e, launch_redact_regions(p, stream));   // no residency stamp: every slot of a frame's chain is taken (StampKind)
  return RTP_OK;
}

// the apply kernel (the blur: its two launches): slot sj's records into `image` (w x h, dense), on `stream`
int apply_enqueue(rtp_engine* e, Ctx& cx, int sj, unsigned char* image, int w, int h, hipStream_t stream) {
  Slot& sl = cx.slot[sj];
  const rtp_redact_config& c = e->redact_cfg;
  RedactApplyParams p;
  memset(&p, 0, sizeof p);
  p.regions = sl.redact.dev; p.num_regions = sl.redact.dev + kRecInts;
  p.image = image; p.scratch = sl.redact.scratch; p.w = w; p.h = h; p.stride = 3L * w;
  p.effect = c.effect; p.ellipse = c.shape == RTP_REDACT_ELLIPSE; p.cell = c.cell; p.radius = c.radius; p.colour = c.colour;
  HIPCHK(e, launch_redact_apply(p, stream));
  return RTP_OK;
}

void redact_free_all(rtp_engine* e) {
  for (Ctx& cx : e->ctx)
    for (Slot& sl : cx.slot) sl.redact.free();
}

// n of a finished launch's records in pinned memory
int host_count(const Slot& sl) { return std::min(std::max(sl.redact.host[kRecInts], 0), (int)RTP_MAX_PEOPLE); }

}  // namespace

void RedactOut::free() {
  if (dev) (void)hipFree(dev);
  if (host) (void)hipHostFree(host);
  if (scratch) (void)hipFree(scratch);
  dev = host = nullptr;
  scratch = nullptr;
}

// The records (and, for the blur, the scratch image) of the first nframes slots.  rtp_set_redaction calls it for every slot, so the frame
// path (frame_outputs_ensure) finds them there; only the slots of a new plan are allocated by their first batch.
int redact_ensure(rtp_engine* e, Ctx& cx, int nframes) {
  const bool blur = e->redact_cfg.effect == RTP_REDACT_BLUR;
  for (int j = 0; j < nframes; ++j) {
    RedactOut& o = cx.slot[j].redact;
    if (o.dev && (!blur || o.scratch)) continue;
    SYNC_GUARD;
    if (!o.dev) {
      HIPCHK(e, hipMalloc((void**)&o.dev, kRecBytes));
      HIPCHK(e, hipHostMalloc((void**)&o.host, kRecBytes, hipHostMallocDefault));
      HIPCHK(e, hipMemset(o.dev, 0, kRecBytes));
      memset(o.host, 0, kRecBytes);
    }
    if (blur && !o.scratch) HIPCHK(e, hipMalloc((void**)&o.scratch, (size_t)e->cfg.disp_w * e->cfg.disp_h * 3));
  }
  return RTP_OK;
}

// frame_outputs_launch: frame sj's records on the frame's own stream behind the kernels that produce `poses`, the redaction of its rendered
// image behind the pose overlay and in front of overlay mode's drawing and the image's export, and the records -> pinned memory in front of
// the frame's last event.  A frame without a display image gets records only.
int redact_launch(rtp_engine* e, Ctx& cx, int sj, const float* poses, bool with_image) {
  Slot& sl = cx.slot[sj];
  int rc;
  if ((rc = regions_enqueue(e, cx, sj, poses, sl.stream))) return rc;
  if (with_image && (rc = apply_enqueue(e, cx, sj, sl.render.dev, e->cfg.disp_w, e->cfg.disp_h, sl.stream))) return rc;
  HIPCHK(e, hipMemcpyAsync(sl.redact.host, sl.redact.dev, kRecBytes, hipMemcpyDeviceToHost, sl.stream));
  return RTP_OK;
}

}  // namespace eng
}  // namespace rtp

extern "C" {

// The apply kernel alone (idle engine, context 0, mode on; not part of the public header — tools/bench_redact.py): the regions kernel
// once on the caller's people, then `launches` (at most 400: they are enqueued within 4 ms) applications back to back on the slot's
// rendered image (display size; the blur: both launches each time) between two events.  *period_us = one application's period,
// *num_valid = the valid regions.  regions != 0: the regions kernel is timed instead.
extern "C" int rtp_internal_redact_time(rtp_engine* e, const float* joints_host, int num_people, int regions, int launches, float* period_us, int* num_valid) {
  static const char* fn = "rtp_internal_redact_time";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->redact_on) return fail(e, RTP_EINVAL, "%s: redaction mode is off (rtp_set_redaction)", fn);
  if (!period_us || launches < 1 || launches > 400 || num_people < 0 || num_people > RTP_MAX_PEOPLE || (num_people > 0 && !joints_host)) return fail(e, RTP_EINVAL, "%s: bad argument", fn);
  int rc;
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  if ((rc = need_idle(e))) return rc;
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if (!sl.render.dev) return fail(e, RTP_EINVAL, "%s: the engine does not render", fn);
  if ((rc = redact_ensure(e, cx, 1))) return rc;
  if (num_people > 0) HIPCHK(e, hipMemcpy(sl.joints, joints_host, (size_t)num_people * e->plan.num_parts * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.num_people, &num_people, sizeof(int), hipMemcpyHostToDevice));
  auto one = [&]() { return regions ? regions_enqueue(e, cx, 0, sl.joints, sl.stream) : apply_enqueue(e, cx, 0, sl.render.dev, e->cfg.disp_w, e->cfg.disp_h, sl.stream); };
  if ((rc = regions_enqueue(e, cx, 0, sl.joints, sl.stream))) return rc;
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
  const hipError_t sync = hipStreamSynchronize(sl.stream);   // (nothing of the train is pending when the buffers go)
  if (s == hipSuccess) s = sync;
  for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
  if (hold) (void)hipFree(hold);
  std::vector<int> recs(kRecInts + 1, 0);
  const hipError_t got = hipMemcpy(recs.data(), sl.redact.dev, kRecBytes, hipMemcpyDeviceToHost);
  if (s == hipSuccess) s = got;
  if (rc) return rc;
  HIPCHK(e, s);
  *period_us = ms * 1e3f / (float)launches;
  if (num_valid) {
    *num_valid = 0;
    for (int k = 0; k < std::min(std::max(recs[kRecInts], 0), (int)RTP_MAX_PEOPLE); ++k) *num_valid += recs[(size_t)k * RTP_REDACT_REGION_INTS + 5] != 0;
  }
  return RTP_OK;
}

// The switch needs an idle engine, like the other modes'.  Nothing is changed by a refused call.  The records and the blur's scratch
// images of every frame slot are allocated here, so that the frame path allocates nothing.
int rtp_set_redaction(rtp_engine* e, const rtp_redact_config* cfg) {
  static const char* fn = "rtp_set_redaction";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  std::vector<int> list;
  if (cfg) {
    if (cfg->struct_size != sizeof(rtp_redact_config))
      return fail(e, RTP_EINVAL, "%s: rtp_redact_config.struct_size is %u, this library's rtp_redact_config has %zu bytes", fn, cfg->struct_size, sizeof(rtp_redact_config));
    const char* bad = rtp_internal_redact_check(cfg, e->plan.num_parts);
    if (bad) return fail(e, RTP_EINVAL, "%s: %s (effect %d, shape %d, num_parts %d, min_score %g, min_parts %d, scale_q8 %d, aspect_q8 %d, pad %d, min_radius %d, cell %d, radius %d)", fn,
                         bad, cfg->effect, cfg->shape, cfg->num_parts, (double)cfg->min_score, cfg->min_parts, cfg->scale_q8, cfg->aspect_q8, cfg->pad, cfg->min_radius, cfg->cell,
                         cfg->radius);
    if (!e->cfg.render) return fail(e, RTP_EINVAL, "%s: the engine does not render (rtp_config.render is 0): there is no image to redact", fn);
    int parts[RTP_MAX_NUM_PARTS];
    const int n = rtp_internal_redact_list(cfg, e->plan.num_parts, parts);
    if (n < 1) return fail(e, RTP_EINVAL, "%s: NULL parts, and a model of %d parts has no head parts (rtp_crops_head_parts)", fn, e->plan.num_parts);
    list.assign(parts, parts + n);
  }
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (!cfg && !e->redact_on) return RTP_OK;
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  SYNC_GUARD;
  int rc;
  if ((rc = need_idle(e))) return rc;
  // RTP_GRAPH_POST=1, as crops mode: graphs captured in the other state go.  (A rendering engine launches every batch eagerly, so
  // there are none today; the line keeps that true whatever launch_batch decides later.)
  if (e->graph_post && (rc = invalidate_graphs(e))) return rc;
  const bool was_on = e->redact_on;
  const rtp_redact_config old_cfg = e->redact_cfg;
  if (!cfg) redact_free_all(e);
  e->redact_on = cfg != nullptr;
  e->redact_cfg = cfg ? *cfg : rtp_redact_config{};
  e->redact_cfg.parts = nullptr;
  e->redact_cfg.num_parts = (int)list.size();
  for (Ctx& cx : e->ctx)
    if (cfg && (rc = redact_ensure(e, cx, (int)cx.slot.size()))) {   // (out of memory: the mode stays as it was; what was allocated stays for the next call)
      e->redact_on = was_on;
      e->redact_cfg = old_cfg;
      return rc;
    }
  e->redact_list = list;
  return RTP_OK;
}

int rtp_redaction_info(const rtp_engine* e, rtp_redact_config* cfg, int* parts) {
  if (!e || !e->redact_on) return RTP_EINVAL;
  if (cfg) *cfg = e->redact_cfg;
  if (parts) memcpy(parts, e->redact_list.data(), e->redact_list.size() * sizeof(int));
  return RTP_OK;
}

// Every refusal but RTP_ERANGE happens before anything is waited for; the frame stays in the FIFO either way.
int rtp_peek_redactions(rtp_engine* e, uint64_t* tag, int* regions_host, int* num_regions, int capacity) {
  static const char* fn = "rtp_peek_redactions";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->redact_on) return fail(e, RTP_EINVAL, "%s: redaction mode is off (rtp_set_redaction)", fn);
  if (!regions_host || !num_regions || capacity < 0) return fail(e, RTP_EINVAL, "%s: NULL regions_host or num_regions, or a negative capacity", fn);
  int rc, ci = 0, sj = 0;
  if ((rc = need_weights(e))) return rc;
  if ((rc = wait_oldest(e, &ci, &sj))) return rc;   // (refuses "nothing in flight" before it waits)
  const Slot& sl = e->ctx[ci].slot[sj];
  const int n = host_count(sl);
  *num_regions = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, the frame has %d records", fn, capacity, n);
  memcpy(regions_host, sl.redact.host, (size_t)n * RTP_REDACT_REGION_INTS * sizeof(int));
  if (tag) *tag = sl.tag;
  return RTP_OK;
}

// Parity tap: the kernels of the async path on caller data, context 0, slot 0
int rtp_redact_from_joints(rtp_engine* e, const float* joints_host, int num_people, unsigned char* image_host_in_out, int w, int h, int* regions_out, int* num_regions,
                           int capacity) {
  static const char* fn = "rtp_redact_from_joints";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->redact_on) return fail(e, RTP_EINVAL, "%s: redaction mode is off (rtp_set_redaction)", fn);
  // (num_people goes to the device as it is: above RTP_MAX_PEOPLE and negative values are what the kernels have to clamp)
  const int n = std::min(std::max(num_people, 0), RTP_MAX_PEOPLE);
  if (!regions_out || !num_regions || capacity < 0 || (n > 0 && !joints_host)) return fail(e, RTP_EINVAL, "%s: NULL regions_out, num_regions or joints, or a negative capacity", fn);
  if (image_host_in_out && (w < 1 || h < 1 || w > e->cfg.disp_w || h > e->cfg.disp_h))
    return fail(e, RTP_EINVAL, "%s: the image is %d x %d, the engine's display size %d x %d", fn, w, h, e->cfg.disp_w, e->cfg.disp_h);
  *num_regions = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, %d records", fn, capacity, n);
  int rc;
  if (e->ctx.empty()) return fail(e, RTP_EINVAL, "%s: the engine has no plan", fn);
  if ((rc = need_idle(e))) return rc;
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  if (!sl.render.dev) return fail(e, RTP_EINVAL, "%s: the engine does not render", fn);
  if ((rc = redact_ensure(e, cx, 1))) return rc;
  if (n > 0) HIPCHK(e, hipMemcpy(sl.joints, joints_host, (size_t)n * e->plan.num_parts * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.num_people, &num_people, sizeof(int), hipMemcpyHostToDevice));
  const size_t ibytes = image_host_in_out ? (size_t)w * h * 3 : 0;
  if (ibytes) HIPCHK(e, hipMemcpy(sl.render.dev, image_host_in_out, ibytes, hipMemcpyHostToDevice));
  if ((rc = regions_enqueue(e, cx, 0, sl.joints, sl.stream))) return rc;
  if (ibytes && (rc = apply_enqueue(e, cx, 0, sl.render.dev, w, h, sl.stream))) return rc;
  HIPCHK(e, hipMemcpyAsync(sl.redact.host, sl.redact.dev, kRecBytes, hipMemcpyDeviceToHost, sl.stream));
  HIPCHK(e, hipStreamSynchronize(sl.stream));
  if (host_count(sl) != n) return fail(e, RTP_EHIP, "%s: the kernel wrote %d records, expected %d", fn, host_count(sl), n);
  memcpy(regions_out, sl.redact.host, (size_t)n * RTP_REDACT_REGION_INTS * sizeof(int));
  if (ibytes) HIPCHK(e, hipMemcpy(image_host_in_out, sl.render.dev, ibytes, hipMemcpyDeviceToHost));
  return RTP_OK;
}

}  // extern "C"

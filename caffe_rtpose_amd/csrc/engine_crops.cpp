// engine_crops.cpp — the engine's side of crops mode (crops.hip): the mode switch, the per-slot buffers, the kernel each frame's
// post-processing chain gains while the mode is on, the two peek entries and the parity tap.  Boxes and pixels are rtp_crop_people's
// (host_util.cpp) bit for bit.
#include "engine_internal.h"

namespace rtp {
namespace eng __attribute__((visibility("hidden"))) {

namespace {

size_t crop_bytes(const rtp_engine* e) { return (size_t)e->crops_cfg.crop_w * e->crops_cfg.crop_h * 3; }
size_t boxes_bytes(const rtp_engine* e) { return (size_t)e->crops_cfg.max_crops * RTP_CROP_BOX_FLOATS * sizeof(float); }

// frame sj's boxes -> boxes (or nullptr), its crops -> dst (or nullptr: boxes only) on `stream`, from the joints `poses`
int crops_enqueue(rtp_engine* e, Ctx& cx, int sj, const float* poses, float* boxes, unsigned char* dst, long crop_stride, hipStream_t stream) {
  Slot& sl = cx.slot[sj];
  const rtp_crops_config& c = e->crops_cfg;
  CropsParams p;
  memset(&p, 0, sizeof p);
  p.src = dst ? sl.disp_cur : nullptr; p.w = e->cfg.disp_w; p.h = e->cfg.disp_h;
  p.joints = poses; p.num_people = sl.num_people;
  p.boxes = boxes; p.dst = p.src ? dst : nullptr; p.crop_stride = crop_stride;
  p.num_parts = e->plan.num_parts; p.nlist = (int)e->crops_list.size(); p.min_parts = c.min_parts;
  p.crop_w = c.crop_w; p.crop_h = c.crop_h; p.max_crops = c.max_crops; p.layout = c.layout;
  p.wide = p.dst ? crops_wide(c.crop_w, p.dst, crop_stride) : 0;
  p.min_score = c.min_score; p.margin = c.margin;
  for (int i = 0; i < p.nlist; ++i) p.list[i] = (unsigned char)e->crops_list[i];
  HIPCHK(e, launch_crops(p, stream));   // no residency stamp: every slot of a frame's chain is taken (StampKind: 64 + 8 * sj + 0..7)
  return RTP_OK;
}

void crops_free_all(rtp_engine* e) {
  for (Ctx& cx : e->ctx)
    for (Slot& sl : cx.slot) sl.crops.free();
}

// rtp_crops_view against the current mode: fields only (no HIP call); *hi = the highest byte offset from data the view addresses
int check_crops_view(rtp_engine* e, const rtp_crops_view* v, const char* fn, long* hi) {
  if (!v) return fail(e, RTP_EINVAL, "%s: NULL crops view", fn);
  if (v->struct_size != sizeof(rtp_crops_view))
    return fail(e, RTP_EINVAL, "%s: rtp_crops_view.struct_size is %u, this library's rtp_crops_view has %zu bytes", fn, v->struct_size, sizeof(rtp_crops_view));
  if (!v->data) return fail(e, RTP_EINVAL, "%s: NULL data", fn);
  const long cb = (long)crop_bytes(e);
  if (v->crop_stride < cb) return fail(e, RTP_EINVAL, "%s: crop_stride %ld, a crop has %ld bytes", fn, v->crop_stride, cb);
  if (__builtin_mul_overflow((long)(e->crops_cfg.max_crops - 1), v->crop_stride, hi) || __builtin_add_overflow(*hi, cb - 1, hi))
    return fail(e, RTP_EINVAL, "%s: the view's extent overflows", fn);
  return RTP_OK;
}

// what the peek entries refuse before they wait for anything
int peek_checks(rtp_engine* e, const char* fn, const float* boxes_host, const int* num_boxes, int capacity) {
  if (!e->crops_on) return fail(e, RTP_EINVAL, "%s: crops mode is off (rtp_set_crops_output)", fn);
  if (!boxes_host || !num_boxes || capacity < 0) return fail(e, RTP_EINVAL, "%s: NULL boxes_host or num_boxes, or a negative capacity", fn);
  return need_weights(e);
}

// the finished frame's n; RTP_ERANGE where the caller's buffers hold fewer
int frame_boxes(rtp_engine* e, const char* fn, const Slot& sl, int capacity, int* num_boxes) {
  int people;
  memcpy(&people, sl.host_out, sizeof people);
  const int n = std::min(std::max(people, 0), e->crops_cfg.max_crops);
  *num_boxes = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, the frame has %d boxes", fn, capacity, n);
  return RTP_OK;
}

}  // namespace

void CropsOut::free() {
  if (boxes_dev) (void)hipFree(boxes_dev);
  if (boxes_host) (void)hipHostFree(boxes_host);
  if (dev) (void)hipFree(dev);
  if (host) (void)hipHostFree(host);
  boxes_dev = boxes_host = nullptr;
  dev = host = dst = nullptr;
}

// The buffers of the first nframes slots, before their batch is launched (frame_outputs_ensure, and the taps)
int crops_ensure(rtp_engine* e, Ctx& cx, int nframes) {
  const size_t bytes = crop_bytes(e) * e->crops_cfg.max_crops;
  for (int j = 0; j < nframes; ++j) {
    CropsOut& c = cx.slot[j].crops;
    if (c.dst) continue;
    SYNC_GUARD;
    HIPCHK(e, hipMalloc((void**)&c.boxes_dev, boxes_bytes(e)));
    HIPCHK(e, hipHostMalloc((void**)&c.boxes_host, boxes_bytes(e), hipHostMallocDefault));
    if (e->crops_direct) {   // the kernel stores across PCIe: only real crops travel
      HIPCHK(e, hipHostMalloc((void**)&c.host, bytes, hipHostMallocMapped));
      HIPCHK(e, hipHostGetDevicePointer((void**)&c.dst, c.host, 0));
    } else {
      HIPCHK(e, hipMalloc((void**)&c.dev, bytes));
      HIPCHK(e, hipHostMalloc((void**)&c.host, bytes, hipHostMallocDefault));
      c.dst = c.dev;
    }
  }
  return RTP_OK;
}

// frame_outputs_launch: frame sj's boxes and crops -> the slot's buffers -> pinned memory, on the frame's own stream behind the connect
// kernels and in front of the frame's last event.  A frame without a display image gets boxes only.
int crops_launch(rtp_engine* e, Ctx& cx, int sj, const float* poses) {
  Slot& sl = cx.slot[sj];
  sl.crops.pixels = sl.has_disp && sl.disp_cur;
  sl.crops.poses = poses ? poses : sl.joints;
  int rc;
  if ((rc = crops_enqueue(e, cx, sj, sl.crops.poses, sl.crops.boxes_dev, sl.crops.pixels ? sl.crops.dst : nullptr, (long)crop_bytes(e), sl.stream))) return rc;
  HIPCHK(e, hipMemcpyAsync(sl.crops.boxes_host, sl.crops.boxes_dev, boxes_bytes(e), hipMemcpyDeviceToHost, sl.stream));
  if (sl.crops.pixels && !e->crops_direct)
    HIPCHK(e, hipMemcpyAsync(sl.crops.host, sl.crops.dev, crop_bytes(e) * e->crops_cfg.max_crops, hipMemcpyDeviceToHost, sl.stream));
  return RTP_OK;
}

}  // namespace eng
}  // namespace rtp

extern "C" {

// Which store path the kernel would take for the view in the engine's current mode: 1 = 16-byte stores, 0 = byte by byte, or
// RTP_EINVAL.  Host only (field checks and crops_wide, no HIP call, the pointer is never dereferenced); not part of the public header —
// the tests use it to see that both paths are reached.  v == NULL: the engine's own per-slot buffer (16-byte aligned, dense).
extern "C" int rtp_internal_crops_layout(rtp_engine* e, const rtp_crops_view* v) {
  static const char* fn = "rtp_internal_crops_layout";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->crops_on) return fail(e, RTP_EINVAL, "%s: crops mode is off (rtp_set_crops_output)", fn);
  if (!v) return crops_wide(e->crops_cfg.crop_w, nullptr, (long)((size_t)e->crops_cfg.crop_w * e->crops_cfg.crop_h * 3));
  long hi = 0;
  int rc;
  if ((rc = check_crops_view(e, v, fn, &hi))) return rc;
  return crops_wide(e->crops_cfg.crop_w, v->data, v->crop_stride);
}

// How the chain's pixels reach the host (idle engine; not part of the public header — tools/bench_crops.py measures both):
// 0 = the kernel writes device memory and max_crops slots are copied behind it, 1 = the kernel stores into mapped pinned memory
extern "C" int rtp_internal_crops_direct(rtp_engine* e, int on) {
  static const char* fn = "rtp_internal_crops_direct";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (!e->ctx.empty()) {
    SYNC_GUARD;
    int rc;
    if ((rc = need_idle(e))) return rc;
    crops_free_all(e);
  }
  e->crops_direct = on ? 1 : 0;
  return RTP_OK;
}

// The kernel alone (idle engine, context 0; not part of the public header — tools/bench_crops.py): caller data as in
// rtp_crops_from_joints, `launches` (at most a few hundred: they are enqueued within 4 ms) launches back to back on the slot's stream between two events; *period_us = one launch's period
extern "C" int rtp_internal_crops_time(rtp_engine* e, const unsigned char* display_bgr_host, const float* joints_host, int num_people, int launches, float* period_us) {
  static const char* fn = "rtp_internal_crops_time";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->crops_on) return fail(e, RTP_EINVAL, "%s: crops mode is off (rtp_set_crops_output)", fn);
  if (!display_bgr_host || !period_us || launches < 1 || num_people < 0 || num_people > RTP_MAX_PEOPLE || (num_people > 0 && !joints_host)) return fail(e, RTP_EINVAL, "%s: bad argument", fn);
  int rc;
  if ((rc = need_idle(e))) return rc;
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  const size_t dbytes = (size_t)e->cfg.disp_w * e->cfg.disp_h * 3;
  if (!sl.disp_dev) HIPCHK(e, hipMalloc((void**)&sl.disp_dev, dbytes));
  HIPCHK(e, hipMemcpy(sl.disp_dev, display_bgr_host, dbytes, hipMemcpyHostToDevice));
  sl.disp_cur = sl.disp_dev;
  if (num_people > 0) HIPCHK(e, hipMemcpy(sl.joints, joints_host, (size_t)num_people * e->plan.num_parts * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.num_people, &num_people, sizeof(int), hipMemcpyHostToDevice));
  if ((rc = crops_ensure(e, cx, 1))) return rc;
  hipEvent_t ev[2];
  HIPCHK(e, hipEventCreate(&ev[0]));
  HIPCHK(e, hipEventCreate(&ev[1]));
  for (int i = 0; i < 3 && !rc; ++i) rc = crops_enqueue(e, cx, 0, sl.joints, sl.crops.boxes_dev, sl.crops.dst, (long)crop_bytes(e), sl.stream);   // warm-up
  // a wave that waits 4 ms holds the stream while the train is enqueued, so that the event pair brackets device work only
  unsigned long long* hold = nullptr;
  hipError_t s = hipMalloc((void**)&hold, 2 * sizeof(unsigned long long));
  if (s == hipSuccess) s = hipStreamSynchronize(sl.stream);
  if (s == hipSuccess) s = launch_queue_wait(400000, hold, sl.stream);
  if (s == hipSuccess) s = hipEventRecord(ev[0], sl.stream);
  for (int i = 0; i < launches && !rc; ++i) rc = crops_enqueue(e, cx, 0, sl.joints, sl.crops.boxes_dev, sl.crops.dst, (long)crop_bytes(e), sl.stream);
  if (s == hipSuccess) s = hipEventRecord(ev[1], sl.stream);
  if (s == hipSuccess) s = hipEventSynchronize(ev[1]);
  float ms = 0.f;
  if (s == hipSuccess) s = hipEventElapsedTime(&ms, ev[0], ev[1]);
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  if (hold) (void)hipFree(hold);
  if (rc) return rc;
  HIPCHK(e, s);
  *period_us = ms * 1e3f / (float)launches;
  return RTP_OK;
}

// The switch needs an idle engine, like the renderer's modes.  Nothing is changed by a refused call.  The buffers of an earlier mode
// are freed here (no copy into them is pending: the engine is idle) and allocated again by the next batch.
int rtp_set_crops_output(rtp_engine* e, const rtp_crops_config* cfg) {
  static const char* fn = "rtp_set_crops_output";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  std::vector<int> list;
  if (cfg) {
    if (cfg->struct_size != sizeof(rtp_crops_config))
      return fail(e, RTP_EINVAL, "%s: rtp_crops_config.struct_size is %u, this library's rtp_crops_config has %zu bytes", fn, cfg->struct_size, sizeof(rtp_crops_config));
    const char* bad = rtp_internal_crops_check(cfg, e->plan.num_parts);
    if (bad) return fail(e, RTP_EINVAL, "%s: %s (crop %dx%d, max_crops %d, num_parts %d, min_score %g, min_parts %d, margin %g, layout %d)", fn, bad, cfg->crop_w, cfg->crop_h,
                         cfg->max_crops, cfg->num_parts, (double)cfg->min_score, cfg->min_parts, (double)cfg->margin, cfg->layout);
    if (cfg->parts) list.assign(cfg->parts, cfg->parts + cfg->num_parts);
    else for (int p = 0; p < e->plan.num_parts; ++p) list.push_back(p);
  }
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (!cfg && !e->crops_on) return RTP_OK;
  if (!e->ctx.empty()) {
    SYNC_GUARD;
    int rc;
    if ((rc = need_idle(e))) return rc;   // (also: no rtp_peek_crops_device of the old mode is still reading a display image)
    // RTP_GRAPH_POST=1: the chains live inside the batch graphs while the mode is off and are launched eagerly while it is on
    // (disp_cur differs from frame to frame, a graph would bake it): either way the graphs captured in the other state go
    if (e->graph_post && (rc = invalidate_graphs(e))) return rc;
    crops_free_all(e);
  }
  e->crops_on = cfg != nullptr;
  e->crops_cfg = cfg ? *cfg : rtp_crops_config{};
  e->crops_cfg.parts = nullptr;
  e->crops_cfg.num_parts = (int)list.size();
  e->crops_list = list;
  return RTP_OK;
}

int rtp_crops_info(const rtp_engine* e, int* crop_w, int* crop_h, int* max_crops, int* layout, size_t* bytes) {
  if (!e || !e->crops_on) return RTP_EINVAL;
  if (crop_w) *crop_w = e->crops_cfg.crop_w;
  if (crop_h) *crop_h = e->crops_cfg.crop_h;
  if (max_crops) *max_crops = e->crops_cfg.max_crops;
  if (layout) *layout = e->crops_cfg.layout;
  if (bytes) *bytes = crop_bytes(e);
  return RTP_OK;
}

// Every refusal but RTP_ERANGE happens before anything is waited for; the frame stays in the FIFO either way.
int rtp_peek_crops(rtp_engine* e, uint64_t* tag, float* boxes_host, int* num_boxes, unsigned char* crops_host, int capacity, int* has_pixels) {
  static const char* fn = "rtp_peek_crops";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc, ci = 0, sj = 0;
  if ((rc = peek_checks(e, fn, boxes_host, num_boxes, capacity))) return rc;
  if ((rc = wait_oldest(e, &ci, &sj))) return rc;   // (refuses "nothing in flight" before it waits)
  const Slot& sl = e->ctx[ci].slot[sj];
  if ((rc = frame_boxes(e, fn, sl, capacity, num_boxes))) return rc;
  const int n = *num_boxes;
  memcpy(boxes_host, sl.crops.boxes_host, (size_t)n * RTP_CROP_BOX_FLOATS * sizeof(float));
  if (sl.crops.pixels && crops_host) memcpy(crops_host, sl.crops.host, (size_t)n * crop_bytes(e));
  if (has_pixels) *has_pixels = sl.crops.pixels ? 1 : 0;
  if (tag) *tag = sl.tag;
  return RTP_OK;
}

// The kernel runs again, from the frame's display image and the joints its chain cropped from (complete, and untouched until the slot's next frame is staged)
// into the caller's view, on the caller's stream (NULL: on the frame's own stream, waited for here).
int rtp_peek_crops_device(rtp_engine* e, uint64_t* tag, float* boxes_host, int* num_boxes, int capacity, const rtp_crops_view* out_dev, void* stream) {
  static const char* fn = "rtp_peek_crops_device";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc, ci = 0, sj = 0;
  if ((rc = peek_checks(e, fn, boxes_host, num_boxes, capacity))) return rc;
  long hi = 0;
  size_t avail = 0;
  if ((rc = check_crops_view(e, out_dev, fn, &hi))) return rc;
  if ((rc = check_caller_stream(e, stream, fn))) return rc;
  if ((rc = use_device(e))) return rc;
  if ((rc = check_device_range(e, fn, "data", out_dev->data, hi, &avail))) return rc;
  if ((rc = wait_oldest(e, &ci, &sj))) return rc;   // (refuses "nothing in flight" before it waits)
  Ctx& cx = e->ctx[ci];
  Slot& sl = cx.slot[sj];
  if (!sl.crops.pixels) return fail(e, RTP_EINVAL, "%s: the frame has no display image (it was submitted as a net input): rtp_peek_crops gives its boxes", fn);
  if ((rc = frame_boxes(e, fn, sl, capacity, num_boxes))) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : sl.stream;
  if ((rc = crops_enqueue(e, cx, sj, sl.crops.poses ? sl.crops.poses : sl.joints, nullptr, (unsigned char*)out_dev->data, out_dev->crop_stride, st))) return rc;
  if ((rc = fence_arm(e, sl.crops.fence, st, !stream))) return rc;
  memcpy(boxes_host, sl.crops.boxes_host, (size_t)*num_boxes * RTP_CROP_BOX_FLOATS * sizeof(float));
  if (tag) *tag = sl.tag;
  return RTP_OK;
}

// Parity tap: the kernel of the async path on caller-supplied joints and display image, context 0, slot 0
int rtp_crops_from_joints(rtp_engine* e, const unsigned char* display_bgr_host, const float* joints_host, int num_people, float* boxes_host,
                          int* num_boxes, unsigned char* crops_host, int capacity) {
  static const char* fn = "rtp_crops_from_joints";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->crops_on) return fail(e, RTP_EINVAL, "%s: crops mode is off (rtp_set_crops_output)", fn);
  if (!boxes_host || !num_boxes || num_people < 0 || num_people > RTP_MAX_PEOPLE || (num_people > 0 && !joints_host) || (crops_host && !display_bgr_host))
    return fail(e, RTP_EINVAL, "%s: NULL boxes_host, num_boxes, joints or display image, or num_people %d outside 0 .. %d", fn, num_people, RTP_MAX_PEOPLE);
  const int n = std::min(num_people, e->crops_cfg.max_crops);
  *num_boxes = n;
  if (capacity < n) return fail(e, RTP_ERANGE, "%s: capacity %d, %d boxes", fn, capacity, n);
  int rc;
  if ((rc = need_idle(e))) return rc;
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  const size_t dbytes = (size_t)e->cfg.disp_w * e->cfg.disp_h * 3;
  if (crops_host) {
    if (!sl.disp_dev) HIPCHK(e, hipMalloc((void**)&sl.disp_dev, dbytes));
    HIPCHK(e, hipMemcpy(sl.disp_dev, display_bgr_host, dbytes, hipMemcpyHostToDevice));
    sl.disp_cur = sl.disp_dev;
  }
  sl.has_disp = crops_host != nullptr;
  if (num_people > 0) HIPCHK(e, hipMemcpy(sl.joints, joints_host, (size_t)num_people * e->plan.num_parts * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(sl.num_people, &num_people, sizeof(int), hipMemcpyHostToDevice));
  if ((rc = crops_ensure(e, cx, 1))) return rc;
  if ((rc = crops_launch(e, cx, 0))) return rc;
  HIPCHK(e, hipStreamSynchronize(sl.stream));
  sl.has_disp = false;
  memcpy(boxes_host, sl.crops.boxes_host, (size_t)n * RTP_CROP_BOX_FLOATS * sizeof(float));
  if (crops_host) memcpy(crops_host, sl.crops.host, (size_t)n * crop_bytes(e));
  return RTP_OK;
}

}  // extern "C"

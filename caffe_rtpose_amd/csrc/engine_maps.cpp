// engine_maps.cpp — the engine's side of maps mode (maps_export.hip): the mode switch, the per-slot buffers, the kernel each frame's
// post-processing chain gains while the mode is on, the two peek entries and the parity tap.  The values are rtp_resize's (NET
// grid) or rtp_forward_heatmaps' (LOWRES grid) bit for bit, the narrow formats those of host_util.cpp's rtp_maps_quantize_u8 and
// rtp_maps_to_f16.
#include "engine_internal.h"

namespace rtp {
namespace eng __attribute__((visibility("hidden"))) {

namespace {

// One frame's payload in the current mode: `planes` planes of H x W elements
struct MapsGeo {
  int planes, H, W;
  int shape[4];
  size_t elem, bytes;
};
MapsGeo maps_geo(const rtp_engine* e) {
  MapsGeo g;
  const int nch = (int)e->maps_chan.size();
  const bool net = e->maps_grid == RTP_MAPS_GRID_NET;
  g.planes = net ? nch : e->N * nch;
  g.H = net ? e->cfg.net_h : e->plan.low_h;
  g.W = net ? e->cfg.net_w : e->plan.low_w;
  g.shape[0] = net ? 1 : e->N; g.shape[1] = nch; g.shape[2] = g.H; g.shape[3] = g.W;
  g.elem = (size_t)maps_elem_bytes(e->maps_format);
  g.bytes = (size_t)g.planes * g.H * g.W * g.elem;
  return g;
}
size_t lowres_floats(const rtp_engine* e) { return (size_t)e->N * e->plan.heat_channels * e->plan.low_h * e->plan.low_w; }
// LOWRES, F32, every channel in its natural order: the payload IS the frame's slice of the context's low-res buffer
bool maps_is_lowres_copy(const rtp_engine* e) {
  if (e->maps_grid != RTP_MAPS_GRID_LOWRES || e->maps_format != RTP_MAPS_F32 || (int)e->maps_chan.size() != e->plan.heat_channels) return false;
  for (size_t i = 0; i < e->maps_chan.size(); ++i)
    if (e->maps_chan[i] != (int)i) return false;
  return true;
}

// frame sj's maps -> the view (dst, channel_stride, row_stride) on `stream`
int maps_enqueue(rtp_engine* e, Ctx& cx, int sj, unsigned char* dst, long channel_stride, long row_stride, hipStream_t stream) {
  const MapsGeo g = maps_geo(e);
  MapsParams p;
  memset(&p, 0, sizeof p);
  p.r.src = cx.lowres + (size_t)sj * lowres_floats(e);
  p.r.dst = nullptr; p.r.num = e->N; p.r.C = e->plan.heat_channels;
  p.r.h = e->plan.low_h; p.r.w = e->plan.low_w; p.r.tw = e->cfg.net_w; p.r.th = e->cfg.net_h;
  p.r.start_scale = e->start_scale; p.r.scale_gap = e->scale_gap;
  p.dst = dst; p.channel_stride = channel_stride; p.row_stride = row_stride;
  p.grid = e->maps_grid; p.format = e->maps_format; p.nch = (int)e->maps_chan.size(); p.num_parts = e->plan.num_parts;
  p.wide = maps_export_wide(e->maps_grid, e->maps_format, g.W, dst, channel_stride, row_stride);
  for (int i = 0; i < p.nch; ++i) p.chan[i] = (unsigned short)e->maps_chan[i];
  p.stamp = nullptr;   // every residency slot of a frame's chain is taken (StampKind: 64 + 8 * sj + 0..7)
  HIPCHK(e, launch_maps_export(p, stream));
  return RTP_OK;
}

// rtp_maps_view against the current mode: fields only (no HIP call); *hi = the highest byte offset from data the view addresses
int check_maps_view(rtp_engine* e, const rtp_maps_view* v, const char* fn, const MapsGeo& g, long* hi) {
  if (!v) return fail(e, RTP_EINVAL, "%s: NULL maps view", fn);
  if (v->struct_size != sizeof(rtp_maps_view))
    return fail(e, RTP_EINVAL, "%s: rtp_maps_view.struct_size is %u, this library's rtp_maps_view has %zu bytes", fn, v->struct_size, sizeof(rtp_maps_view));
  if (!v->data) return fail(e, RTP_EINVAL, "%s: NULL data", fn);
  const long row_min = (long)g.W * (long)g.elem;
  long plane_min = 0, a = 0, b = 0;
  if (v->row_stride < row_min) return fail(e, RTP_EINVAL, "%s: row_stride %ld, a row of %d elements has %ld bytes", fn, v->row_stride, g.W, row_min);
  if (__builtin_mul_overflow((long)g.H, v->row_stride, &plane_min) || v->channel_stride < plane_min)
    return fail(e, RTP_EINVAL, "%s: channel_stride %ld, a plane of %d rows of %ld bytes needs %ld", fn, v->channel_stride, g.H, v->row_stride, plane_min);
  if (__builtin_mul_overflow((long)(g.planes - 1), v->channel_stride, &a) || __builtin_mul_overflow((long)(g.H - 1), v->row_stride, &b) ||
      __builtin_add_overflow(a, b, hi) || __builtin_add_overflow(*hi, row_min - 1, hi))
    return fail(e, RTP_EINVAL, "%s: the view's extent overflows", fn);
  return RTP_OK;
}

// what both peek entries refuse before they wait for anything
int peek_checks(rtp_engine* e, const char* fn) {
  if (!e->maps_on) return fail(e, RTP_EINVAL, "%s: maps mode is off (rtp_set_maps_output)", fn);
  int rc;
  if ((rc = need_weights(e))) return rc;
  return RTP_OK;
}

}  // namespace

void MapsOut::free() {
  if (dev) (void)hipFree(dev);
  if (host) (void)hipHostFree(host);
  dev = host = nullptr;
  cap = 0;
}

// The buffers of the first nframes slots, before their batch is launched (frame_outputs_ensure, and the tap)
int maps_ensure(rtp_engine* e, Ctx& cx, int nframes) {
  const size_t bytes = maps_geo(e).bytes;
  const bool copy = maps_is_lowres_copy(e);
  for (int j = 0; j < nframes; ++j) {
    MapsOut& m = cx.slot[j].maps;
    if (m.host && (copy || m.dev)) continue;
    SYNC_GUARD;
    if (!copy && !m.dev) HIPCHK(e, hipMalloc((void**)&m.dev, bytes));
    if (!m.host) HIPCHK(e, hipHostMalloc((void**)&m.host, bytes, hipHostMallocDefault));
    m.cap = bytes;
  }
  return RTP_OK;
}

// frame_outputs_launch: frame sj's maps -> the slot's device buffer -> its pinned buffer, on the frame's own stream behind the
// post-processing chain and in front of the frame's last event
int maps_launch(rtp_engine* e, Ctx& cx, int sj) {
  Slot& sl = cx.slot[sj];
  const MapsGeo g = maps_geo(e);
  if (maps_is_lowres_copy(e)) {
    HIPCHK(e, hipMemcpyAsync(sl.maps.host, cx.lowres + (size_t)sj * lowres_floats(e), g.bytes, hipMemcpyDeviceToHost, sl.stream));
    return RTP_OK;
  }
  const long rs = (long)g.W * (long)g.elem;
  int rc;
  if ((rc = maps_enqueue(e, cx, sj, sl.maps.dev, rs * g.H, rs, sl.stream))) return rc;
  HIPCHK(e, hipMemcpyAsync(sl.maps.host, sl.maps.dev, g.bytes, hipMemcpyDeviceToHost, sl.stream));
  return RTP_OK;
}

}  // namespace eng
}  // namespace rtp

extern "C" {

// Which store path the kernel would take for the view in the engine's current mode: 1 = wide stores, 0 = byte by byte, or RTP_EINVAL.
// Host only (field checks and maps_export_wide, no HIP call, the pointer is never dereferenced); not part of the public header — the
// tests use it to see that an aligned dense tensor really takes the wide path and an odd base or pitch the byte-wise one.
extern "C" int rtp_internal_maps_export_layout(rtp_engine* e, const rtp_maps_view* v) {
  static const char* fn = "rtp_internal_maps_export_layout";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->maps_on) return fail(e, RTP_EINVAL, "%s: maps mode is off (rtp_set_maps_output)", fn);
  const MapsGeo g = maps_geo(e);
  long hi = 0;
  int rc;
  if ((rc = check_maps_view(e, v, fn, g, &hi))) return rc;
  return maps_export_wide(e->maps_grid, e->maps_format, g.W, v->data, v->channel_stride, v->row_stride);
}

// The switch needs an idle engine, like the renderer's modes.  Nothing is changed by a refused call.  The buffers of an earlier mode
// are freed here (no copy into them is pending: the engine is idle) and allocated again by the next batch.
int rtp_set_maps_output(rtp_engine* e, const rtp_maps_config* cfg) {
  static const char* fn = "rtp_set_maps_output";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  std::vector<int> chan;
  if (cfg) {
    if (cfg->struct_size != sizeof(rtp_maps_config))
      return fail(e, RTP_EINVAL, "%s: rtp_maps_config.struct_size is %u, this library's rtp_maps_config has %zu bytes", fn, cfg->struct_size, sizeof(rtp_maps_config));
    if (cfg->grid != RTP_MAPS_GRID_NET && cfg->grid != RTP_MAPS_GRID_LOWRES) return fail(e, RTP_EINVAL, "%s: grid %d (0 = net resolution, 1 = low resolution)", fn, cfg->grid);
    if (cfg->format != RTP_MAPS_F32 && cfg->format != RTP_MAPS_F16 && cfg->format != RTP_MAPS_U8)
      return fail(e, RTP_EINVAL, "%s: format %d (0 = f32, 1 = f16, 2 = u8)", fn, cfg->format);
    const int C = e->plan.heat_channels;
    if (!cfg->channels) {
      if (C > RTP_MAPS_MAX_CHANNELS) return fail(e, RTP_EINVAL, "%s: this net has %d channels, one mode takes at most %d: name them", fn, C, RTP_MAPS_MAX_CHANNELS);
      for (int c = 0; c < C; ++c) chan.push_back(c);
    } else {
      if (cfg->num_channels < 1 || cfg->num_channels > RTP_MAPS_MAX_CHANNELS)
        return fail(e, RTP_EINVAL, "%s: num_channels %d (1 .. %d)", fn, cfg->num_channels, RTP_MAPS_MAX_CHANNELS);
      for (int i = 0; i < cfg->num_channels; ++i) {
        if (cfg->channels[i] < 0 || cfg->channels[i] >= C) return fail(e, RTP_EINVAL, "%s: channels[%d] = %d is outside [0, %d)", fn, i, cfg->channels[i], C);
        chan.push_back(cfg->channels[i]);
      }
    }
  }
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "%s: %zu frames in flight (collect them first)", fn, e->fifo.size());
  if (!cfg && !e->maps_on) return RTP_OK;
  if (!e->ctx.empty()) {
    SYNC_GUARD;
    int rc;
    if ((rc = need_idle(e))) return rc;   // (also: no rtp_peek_maps_device of the old mode is still reading the low-res maps)
    if (e->graph_post && (rc = invalidate_graphs(e))) return rc;   // the chains live inside the batch graphs: the new kernel must join or leave them
    for (Ctx& cx : e->ctx)
      for (Slot& sl : cx.slot) sl.maps.free();
  }
  e->maps_on = cfg != nullptr;
  e->maps_grid = cfg ? cfg->grid : 0;
  e->maps_format = cfg ? cfg->format : 0;
  e->maps_chan = chan;
  return RTP_OK;
}

int rtp_maps_info(const rtp_engine* e, int shape[4], int* format, size_t* bytes) {
  if (!e) return RTP_EINVAL;
  if (!e->maps_on) return RTP_EINVAL;
  const MapsGeo g = maps_geo(e);
  if (shape) memcpy(shape, g.shape, sizeof g.shape);
  if (format) *format = e->maps_format;
  if (bytes) *bytes = g.bytes;
  return RTP_OK;
}

// Every refusal happens before anything is waited for; the frame stays in the FIFO either way.
int rtp_peek_maps(rtp_engine* e, uint64_t* tag, void* maps_host, size_t capacity) {
  static const char* fn = "rtp_peek_maps";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc, ci = 0, sj = 0;
  if ((rc = peek_checks(e, fn))) return rc;
  const MapsGeo g = maps_geo(e);
  if (!maps_host || capacity < g.bytes) return fail(e, RTP_EINVAL, "%s: capacity %zu, the maps have %zu bytes (rtp_maps_info)", fn, maps_host ? capacity : (size_t)0, g.bytes);
  if ((rc = wait_oldest(e, &ci, &sj))) return rc;   // (refuses "nothing in flight" before it waits)
  const Slot& sl = e->ctx[ci].slot[sj];
  memcpy(maps_host, sl.maps.host, g.bytes);
  if (tag) *tag = sl.tag;
  return RTP_OK;
}

// The kernel runs again, from the frame's low-res maps (complete: the host has waited for the frame's last event) into the caller's
// view, on the caller's stream (NULL: on the frame's own stream, waited for here).
int rtp_peek_maps_device(rtp_engine* e, uint64_t* tag, const rtp_maps_view* out_dev, void* stream) {
  static const char* fn = "rtp_peek_maps_device";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  int rc, ci = 0, sj = 0;
  if ((rc = peek_checks(e, fn))) return rc;
  const MapsGeo g = maps_geo(e);
  long hi = 0;
  size_t avail = 0;
  if ((rc = check_maps_view(e, out_dev, fn, g, &hi))) return rc;
  if ((rc = check_caller_stream(e, stream, fn))) return rc;
  if ((rc = use_device(e))) return rc;
  if ((rc = check_device_range(e, fn, "data", out_dev->data, hi, &avail))) return rc;
  if ((rc = wait_oldest(e, &ci, &sj))) return rc;   // (refuses "nothing in flight" before it waits)
  Ctx& cx = e->ctx[ci];
  Slot& sl = cx.slot[sj];
  hipStream_t st = stream ? (hipStream_t)stream : sl.stream;
  if ((rc = maps_enqueue(e, cx, sj, (unsigned char*)out_dev->data, out_dev->channel_stride, out_dev->row_stride, st))) return rc;
  if ((rc = fence_arm(e, sl.maps.fence, st, !stream))) return rc;
  if (tag) *tag = sl.tag;
  return RTP_OK;
}

// Parity tap: the kernel of the async path on caller-supplied low-res maps, context 0, slot 0
int rtp_maps_from_lowres(rtp_engine* e, const float* lowres, void* maps_host, size_t capacity) {
  static const char* fn = "rtp_maps_from_lowres";
  SYNC_GUARD;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->maps_on) return fail(e, RTP_EINVAL, "%s: maps mode is off (rtp_set_maps_output)", fn);
  const MapsGeo g = maps_geo(e);
  if (!lowres || !maps_host || capacity < g.bytes) return fail(e, RTP_EINVAL, "%s: capacity %zu, the maps have %zu bytes (rtp_maps_info)", fn, maps_host ? capacity : (size_t)0, g.bytes);
  int rc;
  if ((rc = need_idle(e))) return rc;
  Ctx& cx = e->ctx[0];
  Slot& sl = cx.slot[0];
  HIPCHK(e, hipMemcpy(cx.lowres, lowres, lowres_floats(e) * sizeof(float), hipMemcpyHostToDevice));
  if ((rc = maps_ensure(e, cx, 1))) return rc;
  if ((rc = maps_launch(e, cx, 0))) return rc;
  HIPCHK(e, hipStreamSynchronize(sl.stream));
  memcpy(maps_host, sl.maps.host, g.bytes);
  return RTP_OK;
}

}  // extern "C"

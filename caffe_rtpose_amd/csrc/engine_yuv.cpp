// engine_yuv.cpp — the engine's side of the YUV output (yuv_export.hip): the conversion of a device frame into a caller's planes, the YUV
// mode of the renderer (planar 4:2:0 planes in place of the raw frame) and the export of a rendered frame into a caller's planes.
// Every byte written is what codecs.cpp's rtp_convert_bgr_to_yuv writes.
#include "engine_internal.h"

namespace rtp {
namespace eng __attribute__((visibility("hidden"))) {

// Y, U, V of a w x h 4:2:0 frame one after the other in `planes`, pitches = plane widths: the payload of a Y4M FRAME
YuvView yuv_out_view(unsigned char* planes, int w, int h) {
  const long cw = (w + 1) / 2, ch = (h + 1) / 2;
  YuvView v;
  v.y = planes;
  v.u = planes + (size_t)w * h;
  v.v = v.u + (size_t)cw * ch;
  v.w = w; v.h = h; v.sx = 1; v.sy = 1;
  v.ys = w; v.uvs = cw; v.uvp = 1;
  return v;
}

// rtp_set_render_yuv: frame sj's rendered image -> its planes -> the slot's pinned buffer, on the frame's own stream behind the render
// kernel (the buffers: frame_outputs_ensure)
int yuv_out_launch(rtp_engine* e, Ctx& cx, int sj) {
  Slot& sl = cx.slot[sj];
  const int w = e->cfg.disp_w, h = e->cfg.disp_h;
  const FrameView src = packed_bgr_view(sl.render.dev, w, h);
  const YuvView dst = yuv_out_view(sl.render.yuv_dev, w, h);
  HIPCHK(e, launch_yuv_export(frame_stamp(e, cx, sj, STAMP_YUV_OUT), src, dst, yuv_export_layout(src, dst), sl.stream));
  HIPCHK(e, hipMemcpyAsync(sl.render.yuv_host, sl.render.yuv_dev, rtp_yuv_bytes(w, h, 420), hipMemcpyDeviceToHost, sl.stream));
  return RTP_OK;
}

}  // namespace eng
}  // namespace rtp

extern "C" {

// Which kernel rtp_convert_to_yuv_device would launch for (src, dst): a YuvLayout value, or RTP_EINVAL.  Host only (field checks and
// yuv_export_layout, no HIP call, pointers are never dereferenced); not part of the public header — the tests use it to see that
// aligned 4:2:0 planes really take the 4 x 2 kernel and everything else the generic one.
extern "C" int rtp_internal_yuv_export_layout(const rtp_frame_view* src, const rtp_yuv_view* dst) {
  static const char* fn = "rtp_internal_yuv_export_layout";
  YuvView yv;
  FrameView fv;
  long hi[3], shi = 0;
  int rc;
  if ((rc = check_yuv_fields(nullptr, dst, fn, &yv, hi))) return rc;
  if ((rc = check_view_fields(nullptr, src, fn, &fv, &shi))) return rc;
  return yuv_export_layout(fv, yv);
}

// The conversion kernel alone, on the caller's stream: no frame slot, no engine buffer.
int rtp_convert_to_yuv_device(rtp_engine* e, const rtp_frame_view* src, const rtp_yuv_view* dst, void* stream) {
  static const char* fn = "rtp_convert_to_yuv_device";
  YuvView yv;
  FrameView fv;
  long hi[3], shi = 0;
  int rc, layout = LAYOUT_GENERIC;
  if ((rc = check_yuv_fields(e, dst, fn, &yv, hi))) return rc;
  if ((rc = check_view_fields(e, src, fn, &fv, &shi))) return rc;
  if (fv.w != yv.w || fv.h != yv.h) return fail(e, RTP_EINVAL, "%s: the planes are %d x %d, the frame %d x %d", fn, yv.w, yv.h, fv.w, fv.h);
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if ((rc = check_caller_stream(e, stream, fn))) return rc;
  if ((rc = check_view_memory(e, fn, fv, shi, &layout))) return rc;
  if ((rc = check_yuv_memory(e, fn, yv, hi))) return rc;
  if ((rc = use_device(e))) return rc;
  HIPCHK(e, launch_yuv_export(nullptr, fv, yv, yuv_export_layout(fv, yv), (hipStream_t)stream));
  if (!stream) HIPCHK(e, hipStreamSynchronize(nullptr));
  return RTP_OK;
}

// YUV mode of the renderer.  Like rtp_set_render_jpeg the switch needs an idle engine, and there is no captured graph to drop: batches
// of an engine that renders are launched eagerly (launch_batch).
int rtp_set_render_yuv(rtp_engine* e, int chroma) {
  if (!e) return fail(nullptr, RTP_EINVAL, "rtp_set_render_yuv: NULL engine");
  if (chroma != 0 && chroma != 420) return fail(e, RTP_EINVAL, "rtp_set_render_yuv: chroma %d (0 = off, 420)", chroma);
  if (chroma && !e->cfg.render) return fail(e, RTP_EINVAL, "rtp_set_render_yuv needs rtp_config.render >= 1");
  if (chroma && e->jpeg_quality)
    return fail(e, RTP_EINVAL, "rtp_set_render_yuv: JPEG mode is on (rtp_set_render_jpeg %d): one renderer mode at a time", e->jpeg_quality);
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "rtp_set_render_yuv: %zu frames in flight (collect them first)", e->fifo.size());
  int rc;
  if (chroma && (rc = render_host_release(e))) return rc;
  e->yuv_mode = chroma;
  return RTP_OK;
}

// rtp_collect_rendered with the planes of the rendered frame.  Every refusal happens before the frame is taken off the FIFO.
int rtp_collect_rendered_yuv(rtp_engine* e, uint64_t* tag, float* joints, int* num_people, unsigned char* planes_host, size_t capacity) {
  static const char* fn = "rtp_collect_rendered_yuv";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->yuv_mode) return fail(e, RTP_EINVAL, "%s: YUV mode is off (rtp_set_render_yuv)", fn);
  const size_t need = rtp_yuv_bytes(e->cfg.disp_w, e->cfg.disp_h, 420);
  if (!planes_host || capacity < need)
    return fail(e, RTP_EINVAL, "%s: capacity %zu, need rtp_yuv_bytes(%d, %d, 420) = %zu", fn, planes_host ? capacity : (size_t)0, e->cfg.disp_w,
                e->cfg.disp_h, need);
  int rc, ci = 0, sj = 0;
  if ((rc = oldest_frame(e, fn, &ci, &sj))) return rc;
  if ((rc = collect_impl(e, tag, joints, num_people, nullptr, true))) return rc;
  memcpy(planes_host, e->ctx[ci].slot[sj].render.yuv_host, need);
  return RTP_OK;
}

// rtp_collect_rendered_device with the image converted into the caller's planes.  Every refusal happens before the frame is taken off
// the FIFO.  The conversion runs on the caller's stream (NULL: on the frame's own stream, waited for here); the host has already waited
// for the frame's last event in collect_impl, so the rendered image is complete when the conversion is enqueued.
int rtp_collect_rendered_yuv_device(rtp_engine* e, uint64_t* tag, float* joints, int* num_people, const rtp_yuv_view* out, void* stream) {
  static const char* fn = "rtp_collect_rendered_yuv_device";
  YuvView yv;
  long hi[3];
  int rc;
  if ((rc = check_yuv_fields(e, out, fn, &yv, hi))) return rc;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if ((rc = check_caller_stream(e, stream, fn))) return rc;
  if (!e->cfg.render) return fail(e, RTP_EINVAL, "%s needs rtp_config.render >= 1", fn);
  if (yv.w != e->cfg.disp_w || yv.h != e->cfg.disp_h)
    return fail(e, RTP_EINVAL, "%s: the output view is %d x %d, the display image %d x %d", fn, yv.w, yv.h, e->cfg.disp_w, e->cfg.disp_h);
  if ((rc = check_yuv_memory(e, fn, yv, hi))) return rc;
  int ci = 0, sj = 0;
  if ((rc = oldest_frame(e, fn, &ci, &sj))) return rc;
  if ((rc = collect_impl(e, tag, joints, num_people, nullptr, true))) return rc;
  Ctx& cx = e->ctx[ci];
  Slot& sl = cx.slot[sj];
  hipStream_t st = stream ? (hipStream_t)stream : sl.stream;
  const FrameView src = packed_bgr_view(sl.render.dev, e->cfg.disp_w, e->cfg.disp_h);
  HIPCHK(e, launch_yuv_export(frame_stamp(e, cx, sj, STAMP_YUV_OUT), src, yv, yuv_export_layout(src, yv), st));
  return fence_arm(e, sl.render.fence, st, !stream);
}

}  // extern "C"

// engine_jpeg.cpp — the engine's side of both GPU codecs: the encoder's buffers and tables (jpeg_enc.hip), the decoder's buffers, plan
// and launches (jpeg_dec.hip, jpeg_plan.h), and the entry points that encode rendered frames or decode submitted files.
#include "engine_internal.h"

namespace rtp {
namespace eng __attribute__((visibility("hidden"))) {

// ---- the GPU JPEG encoder (jpeg_enc.hip) ----------------------------------------------------------------------------------------
// A w x h encoder: one device allocation of scratch (with the Huffman code tables, filled here) and one pinned buffer that the last
// kernel writes: the file after its header, padded to 16 bytes, then the length.  Called under SYNC_GUARD (hipMalloc, hipMemcpy).
void jpeg_free(JpegBufs* b, unsigned char** host, size_t* cap) {
  if (b->base) (void)hipFree(b->base);
  if (*host) (void)hipHostFree(*host);
  *b = JpegBufs();
  *host = nullptr;
  *cap = 0;
}

namespace {
bool jpeg_size_ok(int w, int h) {  // every bit offset of the entropy-coded segment fits 31 bits
  return w >= 1 && h >= 1 && w <= 65535 && h <= 65535 && (double)((w + 15) / 16) * ((h + 15) / 16) * 6 * kJpegMaxBlockBits < 2147483648.0;
}
}  // namespace

int jpeg_alloc(rtp_engine* e, int w, int h, JpegBufs* b, unsigned char** host, unsigned char** host_dev, size_t* cap) {
  jpeg_free(b, host, cap);
  *host_dev = nullptr;
  JpegBufs nb;
  unsigned char* hb = nullptr;
  unsigned char* hd = nullptr;
  unsigned char qt[2][64], hdr[1024];
  JpegHuffTab huff[4];
  unsigned short code[4][256];
  unsigned char size[4][256];
  rtp_internal_jpeg_setup(w, h, 75, qt, hdr, sizeof hdr, code, size);
  for (int t = 0; t < 4; ++t) { memcpy(huff[t].code, code[t], sizeof code[t]); memcpy(huff[t].size, size[t], sizeof size[t]); }
  const size_t c = (rtp_jpeg_max_bytes(w, h) + 15) / 16 * 16;   // >= the stuffed data + EOI rounded up to 16 bytes
  const char* what = "hipMalloc";
  hipError_t st = hipMalloc(&nb.base, jpeg_bufs_bytes(w, h, nullptr));
  if (st == hipSuccess) {
    jpeg_bufs_bytes(w, h, &nb);
    what = "hipMemcpy";
    st = hipMemcpy(nb.huff, huff, sizeof huff, hipMemcpyHostToDevice);
  }
  if (st == hipSuccess) { what = "hipHostMalloc"; st = hipHostMalloc((void**)&hb, c + 16, hipHostMallocMapped | hipHostMallocCoherent); }
  if (st == hipSuccess) { what = "hipHostGetDevicePointer"; st = hipHostGetDevicePointer((void**)&hd, hb, 0); }
  if (st != hipSuccess) {   // nothing half-made stays behind
    if (nb.base) (void)hipFree(nb.base);
    if (hb) (void)hipHostFree(hb);
    return fail(e, RTP_EHIP, "JPEG encoder buffers for %d x %d: %s failed: %s", w, h, what, hipGetErrorString(st));
  }
  *b = nb;
  *host = hb;
  *host_dev = hd;
  *cap = c;
  return RTP_OK;
}

namespace {
// the quantisers of `quality` (jcdctmgr.c divides by 8 Q) and the header of a w x h file
void jpeg_tables(int w, int h, int quality, JpegQuant* q, std::vector<unsigned char>* hdr) {
  unsigned char qt[2][64], hb[1024];
  unsigned short code[4][256];
  unsigned char size[4][256];
  const size_t hl = rtp_internal_jpeg_setup(w, h, quality, qt, hb, sizeof hb, code, size);
  hdr->assign(hb, hb + hl);
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const uint64_t dv = (uint64_t)qt[t][i] << 3;
      q->recip[t][i] = (unsigned)(((1ull << 32) + dv - 1) / dv);
      q->half[t][i] = (unsigned short)(dv >> 1);
    }
}
}  // namespace

// ---- the GPU JPEG decoder (jpeg_dec.hip) -------------------------------------------------------------------------------------------
void jd_free(JdBufs* b) {
  if (b->dev) (void)hipFree(b->dev);
  if (b->host) (void)hipHostFree(b->host);
  if (b->status_host) (void)hipHostFree(b->status_host);
  *b = JdBufs();
}

namespace {
// Room in the decoder's buffers; the first `keep` bytes of the pinned buffer survive its growth.  Rare (the first file of a slot, or a
// larger one): under the creation lock, and hipFree synchronises the device.
int jd_ensure(rtp_engine* e, JdBufs* b, size_t host_bytes, size_t dev_bytes, size_t keep) {
  if (host_bytes <= b->host_cap && dev_bytes <= b->dev_cap && b->status_host) return RTP_OK;
  SYNC_GUARD;
  if (!b->status_host) {
    HIPCHK(e, hipHostMalloc((void**)&b->status_host, 64, hipHostMallocDefault));
    HIPCHK(e, hipHostGetDevicePointer((void**)&b->status_host_dev, b->status_host, 0));
    *b->status_host = 0xffffffffu;
  }
  if (host_bytes > b->host_cap) {
    const size_t cap = round_up_sz(host_bytes + host_bytes / 4, 4096);
    unsigned char* nh = nullptr;
    HIPCHK(e, hipHostMalloc((void**)&nh, cap, hipHostMallocDefault));
    if (keep && b->host) memcpy(nh, b->host, std::min(keep, b->host_cap));
    if (b->host) (void)hipHostFree(b->host);
    b->host = nh; b->host_cap = cap;
  }
  if (dev_bytes > b->dev_cap) {
    const size_t cap = round_up_sz(dev_bytes + dev_bytes / 4, 4096);
    if (b->dev) (void)hipFree(b->dev);
    b->dev = nullptr; b->dev_cap = 0;
    HIPCHK(e, hipMalloc((void**)&b->dev, cap));
    b->dev_cap = cap;
  }
  return RTP_OK;
}

void jd_fill_recon(const JpegGeom& g, JdRecon* r, long* plane_bytes) {
  memset(r, 0, sizeof *r);
  r->W = g.W; r->H = g.H; r->ncomp = g.ncomp; r->rgb = g.rgb; r->hmax = g.hmax; r->vmax = g.vmax;
  long off = 0;
  int blocks = 0;
  for (int c = 0; c < g.ncomp; ++c) {
    r->h[c] = g.h[c]; r->v[c] = g.v[c]; r->bw[c] = g.bw[c]; r->bh[c] = g.bh[c]; r->dw[c] = g.dw[c]; r->dh[c] = g.dh[c];
    r->coef_off[c] = blocks;
    blocks += g.bw[c] * g.bh[c];
    r->plane_off[c] = off;
    off += (long)round_up_sz((size_t)g.bw[c] * 8 * g.bh[c] * 8, 256);
    memcpy(r->qn[c], g.qn[c], sizeof r->qn[c]);
  }
  r->blocks = blocks;
  *plane_bytes = off;
}

// Parse the file, stage what the device needs in b's pinned buffer and describe the launches in *job.  No HIP work is enqueued.
// Failures carry the code and the message of rtp_decode_image.
int jd_plan(rtp_engine* e, const char* fn, const unsigned char* bytes, size_t n, int sub_bits, int group, bool force_host, JdBufs* b, JdJob* job) {
  int rc;
  const size_t wcap = std::min(kJdStageCap, round_up_sz(n + n / 2 + 64, 4));
  if ((rc = jd_ensure(e, b, wcap, 0, 0))) return rc;
  JpegPlan P;
  try {
    rc = jpeg_plan(bytes, n, sub_bits, reinterpret_cast<uint32_t*>(b->host), wcap / 4, force_host, &P);
  } catch (const std::exception& ex) {
    return fail(e, RTP_ENOMEM, "%s: %s", fn, ex.what());
  }
  if (rc) return fail(e, rc, "%s: %s", fn, rtp_codec_last_error());
  // one synchronisation launch is enqueued per workgroup of subsequences: a scan that would need more than kJdMaxGroups of them (a
  // huge file, or tiny S / group from a test or a sweep) takes the host's entropy decoder instead of flooding the stream
  if (P.path == RTP_JPEG_ENTROPY_DEVICE && (P.subs.size() + group - 1) / group > (size_t)kJdMaxGroups) {
    try {
      rc = jpeg_plan(bytes, n, sub_bits, nullptr, 0, true, &P);
    } catch (const std::exception& ex) {
      return fail(e, RTP_ENOMEM, "%s: %s", fn, ex.what());
    }
    if (rc) return fail(e, rc, "%s: %s", fn, rtp_codec_last_error());
  }
  long plane_bytes = 0;
  jd_fill_recon(P.g, &job->g, &plane_bytes);
  const bool dev = P.path == RTP_JPEG_ENTROPY_DEVICE;
  job->path = P.path;
  job->group = group;
  job->mcus = P.g.mcux * P.g.mcuy;
  job->L = jd_layout(job->g.blocks, plane_bytes, dev ? P.nwords : 0, dev ? P.segs.size() : 0, dev ? P.subs.size() : 0, group);
  const JdLayout& L = job->L;
  const size_t coef_bytes = (size_t)job->g.blocks * 64 * sizeof(short);
  if ((rc = jd_ensure(e, b, dev ? L.staged : coef_bytes, L.total, dev ? P.nwords * 4 : 0))) return rc;
  job->coef = reinterpret_cast<short*>(b->dev + L.coef);
  job->planes = b->dev + L.planes;
  if (!dev) {
    memcpy(b->host, P.coef.data(), coef_bytes);
    job->copy_bytes = coef_bytes; job->copy_dst = L.coef;
    return RTP_OK;
  }
  JdTables* tab = reinterpret_cast<JdTables*>(b->host + L.tab);
  tab->scan = P.scan;
  memcpy(tab->dc, P.dc, sizeof tab->dc);
  memcpy(tab->ac, P.ac, sizeof tab->ac);
  memcpy(b->host + L.segs, P.segs.data(), P.segs.size() * sizeof(JdSeg));
  memcpy(b->host + L.subs, P.subs.data(), P.subs.size() * sizeof(JdSub));
  job->copy_bytes = L.staged; job->copy_dst = 0;
  JdDev& d = job->d;
  d.tab = reinterpret_cast<const JdTables*>(b->dev + L.tab);
  d.segs = reinterpret_cast<const JdSeg*>(b->dev + L.segs);
  d.subs = reinterpret_cast<const JdSub*>(b->dev + L.subs);
  d.words = reinterpret_cast<const uint32_t*>(b->dev + L.words);
  d.nsub = (int)P.subs.size(); d.nwords = (int)P.nwords; d.ngroups = L.ngroups;
  d.entry = reinterpret_cast<JdState*>(b->dev + L.entry);
  d.exit_ = reinterpret_cast<JdState*>(b->dev + L.exit_);
  d.count = reinterpret_cast<int*>(b->dev + L.count);
  d.excl = reinterpret_cast<int*>(b->dev + L.excl);
  d.gexit = reinterpret_cast<JdState*>(b->dev + L.gexit);
  d.flags = reinterpret_cast<int*>(b->dev + L.flags);
  d.status = reinterpret_cast<unsigned*>(b->dev + L.status);
  d.status_out = b->status_host_dev;
  d.coef = job->coef;
  d.dcsum = reinterpret_cast<int*>(b->dev + L.dcsum);
  return RTP_OK;
}
}  // namespace

// The kernels of a planned decode on `stream` (behind the copy of its staged bytes): entropy decoding where the device does it,
// then the reconstruction into the three named channels of dst
int jd_launch(rtp_engine* e, unsigned long long* stamp, const JdJob& job, const FrameView& dst, hipStream_t stream) {
  if (job.path == RTP_JPEG_ENTROPY_DEVICE)
    HIPCHK(e, launch_jpeg_entropy(stamp, job.d, job.group, job.mcus, job.g.ncomp, job.g.blocks, stream));
  HIPCHK(e, launch_jpeg_reconstruct(stamp, job.g, job.coef, job.planes, dst, stream));
  return RTP_OK;
}

}  // namespace eng
}  // namespace rtp

extern "C" {

// ---- JPEG files decoded on the GPU ---------------------------------------------------------------------------------------------------
// rtp_decode_jpeg_device with the test knobs: sub_bits = S (0: the engine's), group = subsequences per workgroup (0: the engine's),
// force_host = 1: the host's entropy decoder whatever the file.  rounds (may be NULL): [0] launches of the synchronisation kernel that
// did work, [1] launches enqueued.  Not part of the public header.
extern "C" int rtp_internal_jpeg_decode_device(rtp_engine* e, const unsigned char* jpeg_host, size_t n, const rtp_frame_view* dst, void* stream,
                                               int sub_bits, int group, int force_host, int* entropy_path, int* rounds) {
  static const char* fn = "rtp_decode_jpeg_device";
  FrameView fv;
  long hi = 0;
  int rc, layout = LAYOUT_GENERIC;
  if ((rc = check_view_fields(e, dst, fn, &fv, &hi))) return rc;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!jpeg_host) return fail(e, RTP_EINVAL, "%s: NULL file", fn);
  if (n >= 8 && jpeg_host[0] == 0x89 && jpeg_host[1] == 'P') return fail(e, RTP_EINVAL, "%s: a PNG file (only JPEG is decoded on the GPU: rtp_decode_image)", fn);
  if (sub_bits <= 0) sub_bits = e->jd_sub_bits;
  if (group <= 0) group = e->jd_group;
  if (sub_bits < 32 || sub_bits % 32 || group < 1 || group > 1024) return fail(e, RTP_EINVAL, "%s: S = %d bits (a multiple of 32), %d subsequences per workgroup (1..1024)", fn, sub_bits, group);
  if ((rc = check_caller_stream(e, stream, fn))) return rc;
  if ((rc = check_view_memory(e, fn, fv, hi, &layout))) return rc;
  if ((rc = use_device(e))) return rc;
  if (e->jdec_ev) HIPCHK(e, hipEventSynchronize(e->jdec_ev));
  else HIPCHK(e, hipEventCreateWithFlags(&e->jdec_ev, hipEventDisableTiming));
  JdJob job;
  if ((rc = jd_plan(e, fn, jpeg_host, n, sub_bits, group, force_host != 0, &e->jdec, &job))) return rc;
  if (job.g.W != fv.w || job.g.H != fv.h) return fail(e, RTP_EINVAL, "%s: the destination is %d x %d, the file %d x %d", fn, fv.w, fv.h, job.g.W, job.g.H);
  if (entropy_path) *entropy_path = job.path;
  const hipStream_t st = (hipStream_t)stream;
  *e->jdec.status_host = 0xffffffffu;
  HIPCHK(e, hipMemcpyAsync(e->jdec.dev + job.copy_dst, e->jdec.host, job.copy_bytes, hipMemcpyHostToDevice, st));
  if ((rc = jd_launch(e, nullptr, job, fv, st))) return rc;
  HIPCHK(e, hipEventRecord(e->jdec_ev, st));
  HIPCHK(e, hipEventSynchronize(e->jdec_ev));
  if (rounds) {
    rounds[0] = rounds[1] = 0;
    if (job.path == RTP_JPEG_ENTROPY_DEVICE) {
      std::vector<int> flags((size_t)job.d.ngroups);
      HIPCHK(e, hipMemcpy(flags.data(), job.d.flags, flags.size() * sizeof(int), hipMemcpyDeviceToHost));
      rounds[1] = job.d.ngroups;
      for (int r = 0; r < job.d.ngroups; ++r) if (r == 0 || flags[r - 1]) rounds[0] = r + 1;
    }
  }
  const unsigned s = *e->jdec.status_host;
  if (s != 0xffffffffu) return fail(e, RTP_EIO, "%s: %s", fn, jpeg_entropy_message((int)(s & 3u)));
  return RTP_OK;
}

int rtp_decode_jpeg_device(rtp_engine* e, const unsigned char* jpeg_host, size_t n, const rtp_frame_view* dst, void* stream, int* entropy_path) {
  return rtp_internal_jpeg_decode_device(e, jpeg_host, n, dst, stream, 0, 0, 0, entropy_path, nullptr);
}

// S and subsequences per workgroup of every later decode of this engine (0: back to the defaults)
extern "C" int rtp_internal_jpeg_knobs(rtp_engine* e, int sub_bits, int group) {
  if (!e) return RTP_EINVAL;
  if (sub_bits < 0 || sub_bits % 32 || group < 0 || group > 1024) return fail(e, RTP_EINVAL, "rtp_internal_jpeg_knobs: S = %d, group = %d", sub_bits, group);
  e->jd_sub_bits = sub_bits ? sub_bits : kJdSubBits;
  e->jd_group = group ? group : kJdGroup;
  return RTP_OK;
}

// The reconstruction kernels alone: coefficient blocks (host, component after component, natural order) and natural-order 16-bit
// quantisers -> the view.  The device counterpart of codecs.cpp's rtp_internal_jpeg_reconstruct_host.
extern "C" int rtp_internal_jpeg_reconstruct_device(rtp_engine* e, int W, int H, int ncomp, const int* hv, const unsigned short* qn, int rgb,
                                                    const short* coef_host, const rtp_frame_view* dst, void* stream) {
  static const char* fn = "rtp_internal_jpeg_reconstruct_device";
  FrameView fv;
  long hi = 0;
  int rc, layout = LAYOUT_GENERIC;
  if ((rc = check_view_fields(e, dst, fn, &fv, &hi))) return rc;
  if (!e || !coef_host) return fail(e, RTP_EINVAL, "%s: NULL argument", fn);
  JpegGeom g;
  if ((rc = rtp_internal_jpeg_geom(W, H, ncomp, hv, qn, rgb, &g))) return fail(e, rc, "%s: %s", fn, rtp_codec_last_error());
  if (fv.w != W || fv.h != H) return fail(e, RTP_EINVAL, "%s: the destination is %d x %d, the image %d x %d", fn, fv.w, fv.h, W, H);
  if ((rc = check_caller_stream(e, stream, fn))) return rc;
  if ((rc = check_view_memory(e, fn, fv, hi, &layout))) return rc;
  if ((rc = use_device(e))) return rc;
  if (e->jdec_ev) HIPCHK(e, hipEventSynchronize(e->jdec_ev));
  else HIPCHK(e, hipEventCreateWithFlags(&e->jdec_ev, hipEventDisableTiming));
  JdJob job;
  long plane_bytes = 0;
  jd_fill_recon(g, &job.g, &plane_bytes);
  job.L = jd_layout(job.g.blocks, plane_bytes, 0, 0, 0, 1);
  const size_t coef_bytes = (size_t)job.g.blocks * 64 * sizeof(short);
  if ((rc = jd_ensure(e, &e->jdec, coef_bytes, job.L.total, 0))) return rc;
  memcpy(e->jdec.host, coef_host, coef_bytes);
  job.coef = reinterpret_cast<short*>(e->jdec.dev + job.L.coef);
  job.planes = e->jdec.dev + job.L.planes;
  const hipStream_t st = (hipStream_t)stream;
  HIPCHK(e, hipMemcpyAsync(job.coef, e->jdec.host, coef_bytes, hipMemcpyHostToDevice, st));
  if ((rc = jd_launch(e, nullptr, job, fv, st))) return rc;
  HIPCHK(e, hipEventRecord(e->jdec_ev, st));
  HIPCHK(e, hipEventSynchronize(e->jdec_ev));
  return RTP_OK;
}

// rtp_submit_frame on the pixels rtp_decode_image makes of the file: the scan (or the host decoder's coefficients) crosses PCIe, the
// decode kernels run in front of the warp.
int rtp_submit_frame_jpeg(rtp_engine* e, const unsigned char* jpeg_host, size_t n, uint64_t tag, float* frame_scale, int* w, int* h) {
  static const char* fn = "rtp_submit_frame_jpeg";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!jpeg_host) return fail(e, RTP_EINVAL, "%s: NULL file", fn);
  int rc, ci, sj;
  const bool png = n >= 8 && jpeg_host[0] == 0x89 && jpeg_host[1] == 'P';
  if (!e->gpu_prep_ok || png) {   // the host fallback of rtp_submit_frame, on the decoded pixels (a PNG file always is decoded there)
    try {   // (nothing may unwind through the C boundary)
      int iw = 0, ih = 0;
      if ((rc = rtp_decode_image(jpeg_host, n, nullptr, 0, &iw, &ih))) return fail(e, rc, "%s: %s", fn, rtp_codec_last_error());
      std::vector<unsigned char> bgr((size_t)iw * ih * 3);
      if ((rc = rtp_decode_image(jpeg_host, n, bgr.data(), bgr.size(), &iw, &ih))) return fail(e, rc, "%s: %s", fn, rtp_codec_last_error());
      if (w) *w = iw;
      if (h) *h = ih;
      return rtp_submit_frame(e, bgr.data(), iw, ih, tag, frame_scale);
    } catch (const std::exception& ex) {
      return fail(e, RTP_ENOMEM, "%s: host decoding: %s", fn, ex.what());
    }
  }
  if ((rc = use_device(e))) return rc;
  if ((rc = need_weights(e))) return rc;
  if (e->prep_defer && (rc = pump(e, PUMP_POLL))) return rc;
  if ((rc = open_slot(e, &ci, &sj))) return rc;
  Ctx& cx = e->ctx[ci];
  Slot& sl = cx.slot[sj];
  // everything that can refuse the file happens before the slot is committed: a failed call leaves the open batch as it was
  if ((rc = jd_plan(e, fn, jpeg_host, n, e->jd_sub_bits, e->jd_group, false, &sl.jd, &sl.jd_job))) return rc;
  if (w) *w = sl.jd_job.g.W;
  if (h) *h = sl.jd_job.g.H;
  if (e->busy_probe && sj == 0 && (rc = busy_mark_stage0(e, cx))) return rc;
  if (e->prep_defer && (rc = flush_prep(e, cx, false))) return rc;   // an earlier frame of this batch whose copy is done by now
  sl.has_disp = true;
  *sl.jd.status_host = 0xffffffffu;
  if ((rc = enqueue_preprocess(e, cx, sj, nullptr, sl.jd_job.g.W, sl.jd_job.g.H, frame_scale, nullptr, true))) return rc;
  sl.jpeg_status = sl.jd_job.path == RTP_JPEG_ENTROPY_DEVICE;
  return commit_slot(e, ci, sj, tag);
}

// ---- JPEG files encoded on the GPU (jpeg_enc.hip: the bytes of rtp_encode_jpeg) ------------------------------------------------
int rtp_set_render_jpeg(rtp_engine* e, int quality) {
  if (!e) return fail(nullptr, RTP_EINVAL, "rtp_set_render_jpeg: NULL engine");
  if (quality < 0 || quality > 100) return fail(e, RTP_EINVAL, "rtp_set_render_jpeg: quality %d (0 = off, 1..100)", quality);
  if (quality && !e->cfg.render) return fail(e, RTP_EINVAL, "rtp_set_render_jpeg needs rtp_config.render >= 1");
  if (quality && e->yuv_mode) return fail(e, RTP_EINVAL, "rtp_set_render_jpeg: YUV mode is on (rtp_set_render_yuv %d): one renderer mode at a time", e->yuv_mode);
  if (quality && !jpeg_size_ok(e->cfg.disp_w, e->cfg.disp_h))
    return fail(e, RTP_EINVAL, "rtp_set_render_jpeg: a %d x %d display image is too large for the GPU encoder", e->cfg.disp_w, e->cfg.disp_h);
  if (!e->fifo.empty()) return fail(e, RTP_EAGAIN, "rtp_set_render_jpeg: %zu frames in flight (collect them first)", e->fifo.size());
  if (quality) {
    jpeg_tables(e->cfg.disp_w, e->cfg.disp_h, quality, &e->jpeg_q, &e->jpeg_hdr);
    int rc;
    if ((rc = render_host_release(e))) return rc;
  }
  e->jpeg_quality = quality;
  return RTP_OK;
}

// rtp_collect_rendered with the JPEG file of the rendered frame.  Every refusal happens before the frame is taken off the FIFO.
int rtp_collect_rendered_jpeg(rtp_engine* e, uint64_t* tag, float* joints, int* num_people, unsigned char* jpeg_host, size_t capacity,
                              size_t* jpeg_bytes) {
  static const char* fn = "rtp_collect_rendered_jpeg";
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if (!e->jpeg_quality) return fail(e, RTP_EINVAL, "%s: JPEG mode is off (rtp_set_render_jpeg)", fn);
  const size_t need = rtp_jpeg_max_bytes(e->cfg.disp_w, e->cfg.disp_h);
  if (!jpeg_host || capacity < need)
    return fail(e, RTP_EINVAL, "%s: capacity %zu, need rtp_jpeg_max_bytes(%d, %d) = %zu", fn, jpeg_host ? capacity : (size_t)0, e->cfg.disp_w,
                e->cfg.disp_h, need);
  int rc, ci = 0, sj = 0;
  if ((rc = oldest_frame(e, fn, &ci, &sj))) return rc;
  if ((rc = collect_impl(e, tag, joints, num_people, nullptr, true))) return rc;
  const RenderOut& r = e->ctx[ci].slot[sj].render;
  unsigned n = 0;
  memcpy(&n, r.jpeg_host + r.jpeg_cap, sizeof n);
  const size_t hl = e->jpeg_hdr.size();
  if (hl + n > capacity) return fail(e, RTP_EHIP, "%s: the encoder reported %u bytes, more than its bound", fn, n);
  memcpy(jpeg_host, e->jpeg_hdr.data(), hl);
  memcpy(jpeg_host + hl, r.jpeg_host, n);
  if (jpeg_bytes) *jpeg_bytes = hl + n;
  return RTP_OK;
}

// rtp_encode_jpeg on the pixels of a view of device memory, ordered after the work queued on `stream`; returns with the file on the host.
// The engine's own scratch: frames in flight are not touched.
int rtp_encode_jpeg_device(rtp_engine* e, const rtp_frame_view* src, int quality, void* stream, unsigned char* jpeg_host, size_t capacity,
                           size_t* jpeg_bytes) {
  static const char* fn = "rtp_encode_jpeg_device";
  FrameView fv;
  long hi = 0;
  int rc, layout = LAYOUT_GENERIC;
  if ((rc = check_view_fields(e, src, fn, &fv, &hi))) return rc;
  if (!e) return fail(nullptr, RTP_EINVAL, "%s: NULL engine", fn);
  if ((rc = check_caller_stream(e, stream, fn))) return rc;
  if ((rc = check_view_memory(e, fn, fv, hi, &layout))) return rc;
  if (!jpeg_size_ok(fv.w, fv.h)) return fail(e, RTP_EINVAL, "%s: a %d x %d frame is too large for the GPU encoder", fn, fv.w, fv.h);
  if ((rc = use_device(e))) return rc;
  if (quality < 1) quality = 1;
  if (quality > 100) quality = 100;
  if (e->jenc.w != fv.w || e->jenc.h != fv.h) {
    SYNC_GUARD;
    if (e->jenc_ev) HIPCHK(e, hipEventSynchronize(e->jenc_ev));
    if ((rc = jpeg_alloc(e, fv.w, fv.h, &e->jenc, &e->jenc_host, &e->jenc_host_dev, &e->jenc_cap))) return rc;
  }
  if (!e->jenc_ev) HIPCHK(e, hipEventCreateWithFlags(&e->jenc_ev, hipEventDisableTiming));
  JpegQuant q;
  std::vector<unsigned char> hdr;
  jpeg_tables(fv.w, fv.h, quality, &q, &hdr);
  const hipStream_t st = (hipStream_t)stream;
  HIPCHK(e, launch_jpeg_encode(nullptr, fv, q, e->jenc, e->jenc_host_dev, reinterpret_cast<unsigned*>(e->jenc_host_dev + e->jenc_cap), st));
  HIPCHK(e, hipEventRecord(e->jenc_ev, st));
  HIPCHK(e, hipEventSynchronize(e->jenc_ev));
  unsigned n = 0;
  memcpy(&n, e->jenc_host + e->jenc_cap, sizeof n);
  const size_t total = hdr.size() + n;
  if (jpeg_bytes) *jpeg_bytes = total;
  if (jpeg_host) {
    if (capacity < total) return fail(e, RTP_EINVAL, "%s: output buffer too small (%zu bytes, the file has %zu)", fn, capacity, total);
    memcpy(jpeg_host, hdr.data(), hdr.size());
    memcpy(jpeg_host + hdr.size(), e->jenc_host, n);
  }
  return RTP_OK;
}

}  // extern "C"

// host_util.cpp — the host-only pieces of the path behind the C-ABI: model descriptor tables,
// default thresholds, process_and_pad_image, the JSON body, the narrow formats of maps mode and the boxes and pixels of
// crops mode (rtp_crop_people), tracking mode (rtp_track_update), its appearance term (rtp_appearance_describe,
// rtp_track_update_appearance), smoothing mode (rtp_smooth_update), overlay mode
// (rtp_overlay_update, rtp_overlay_draw) and redaction mode (rtp_redact_regions, rtp_redact_apply).  No GPU needed.
#include <algorithm>
#include <vector>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>

#include "../../include/rtpose_mi355x.h"

namespace {
// ModelDescriptorFactory::createModelDescriptor (src/rtpose/modelDescriptorFactory.cpp:25-26, 52-53)
const int kCocoLimb[38] = {1, 2, 1, 5, 2, 3, 3, 4, 5, 6, 6, 7, 1, 8, 8, 9, 9, 10, 1, 11, 11, 12, 12, 13, 1, 0, 0, 14, 14, 16, 0, 15, 15, 17, 2, 16, 5, 17};
const int kCocoMap[38] = {31, 32, 39, 40, 33, 34, 35, 36, 41, 42, 43, 44, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 47, 48, 49, 50, 53, 54, 51, 52, 55, 56, 37, 38, 45, 46};
const int kMpiLimb[28] = {0, 1, 1, 2, 2, 3, 3, 4, 1, 5, 5, 6, 6, 7, 1, 14, 14, 11, 11, 12, 12, 13, 14, 8, 8, 9, 9, 10};
const int kMpiMap[28] = {16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 38, 39, 40, 41, 42, 43, 32, 33, 34, 35, 36, 37};
}  // namespace

extern "C" {

int rtp_model_tables(int model, int* num_parts, int* num_limbs, int* limb_seq, int* map_idx) {
  if (model == RTP_MODEL_COCO_18) {
    if (num_parts) *num_parts = 18;
    if (num_limbs) *num_limbs = 19;
    if (limb_seq) memcpy(limb_seq, kCocoLimb, sizeof kCocoLimb);
    if (map_idx) memcpy(map_idx, kCocoMap, sizeof kCocoMap);
    return RTP_OK;
  }
  if (model == RTP_MODEL_MPI_15) {
    if (num_parts) *num_parts = 15;
    if (num_limbs) *num_limbs = 14;
    if (limb_seq) memcpy(limb_seq, kMpiLimb, sizeof kMpiLimb);
    if (map_idx) memcpy(map_idx, kMpiMap, sizeof kMpiMap);
    return RTP_OK;
  }
  return RTP_EINVAL;  // "Undefined ModelDescriptor selected." (modelDescriptorFactory.cpp:59)
}

// warmup(), rtpose.cpp:212-226
int rtp_default_thresholds(int model, float* nms_threshold, float* connect_inter_threshold, int* connect_inter_min_above_threshold,
                           int* connect_min_subset_cnt, float* connect_min_subset_score) {
  if (model != RTP_MODEL_COCO_18 && model != RTP_MODEL_MPI_15) return RTP_EINVAL;
  const bool mpi = model == RTP_MODEL_MPI_15;
  if (nms_threshold) *nms_threshold = mpi ? 0.2f : 0.05f;
  if (connect_inter_threshold) *connect_inter_threshold = mpi ? 0.01f : 0.050f;
  if (connect_inter_min_above_threshold) *connect_inter_min_above_threshold = mpi ? 8 : 9;
  if (connect_min_subset_cnt) *connect_min_subset_cnt = 3;
  if (connect_min_subset_score) *connect_min_subset_score = 0.4f;
  return RTP_OK;
}

// process_and_pad_image, rtpose.cpp:239-269
int rtp_process_and_pad_image(float* target, const unsigned char* bgr, int ow, int oh, int tw, int th, int normalize) {
  if (!target || !bgr || ow < 0 || oh < 0 || tw <= 0 || th <= 0) return RTP_EINVAL;
  const int plane = tw * th;
  const int padw = (tw - ow) / 2, padh = (th - oh) / 2;
  if (padw < 0 || padh < 0) return RTP_EINVAL;  // "Image too big for target size."
  for (int c = 0; c < 3; ++c) {
    float* t = target + (size_t)c * plane;
    for (int y = 0; y < th; ++y) {
      const int oy = y - padh;
      const bool row_in = oy >= 0 && oy < oh;
      for (int x = 0; x < tw; ++x) {
        const int ox = x - padw;
        float v = 0.f;
        if (row_in && ox >= 0 && ox < ow) {
          const float p = (float)bgr[((size_t)oy * ow + ox) * 3 + c];
          v = normalize ? p / 256.0f - 0.5f : p;
        }
        t[(size_t)y * tw + x] = v;
      }
    }
  }
  return RTP_OK;
}

// displayFrame's JSON body, rtpose.cpp:1394-1415: std::ofstream at default precision, i.e. every number as printf("%g")
// (floatfield unset, precision 6).  std::to_chars(general, 6) is specified to produce exactly that text and costs a quarter of
// an ostream insertion: 76 people x 54 numbers (the noise-map worst case) took 1.2 ms per frame through std::ostringstream —
// one writer thread would have capped an 8-GPU node at ~800 frames/s.  tests/test_ref_golden.py: byte-identical to the
// reference's own block, edge values included.
// (recs != nullptr: rtp_format_json_tracked's "id" member in front of every body's "joints")
static long format_json(char* buf, size_t buflen, const float* joints, int num_people, int num_parts, float frame_scale, const int* recs) {
  if (!buf || (num_people > 0 && !joints) || num_people < 0 || num_parts <= 0) return RTP_EINVAL;
  const double scale = 1.0 / frame_scale;
  char* p = buf;
  char* const end = buf + buflen;
  auto lit = [&](const char* s) { const size_t n = strlen(s); if ((size_t)(end - p) < n + 1) return false; memcpy(p, s, n); p += n; return true; };
  auto num = [&](double v) {
    if (end - p < 40) return false;
    const std::to_chars_result r = std::to_chars(p, end - 1, v, std::chars_format::general, 6);
    if (r.ec != std::errc()) return false;
    p = r.ptr;
    return true;
  };
  bool ok = lit("{\n\"version\":0.1,\n\"bodies\":[\n");
  for (int ip = 0; ok && ip < num_people; ip++) {
    ok = lit("{\n");
    if (recs) {
      char id[32];
      snprintf(id, sizeof id, "\"id\":%d,", recs[(size_t)ip * RTP_TRACK_REC_INTS]);
      ok = ok && lit(id);
    }
    ok = ok && lit("\"joints\":[");
    for (int ij = 0; ok && ij < num_parts; ij++) {
      const float* j = joints + ((size_t)ip * num_parts + ij) * 3;
      ok = num(scale * j[0]) && lit(",") && num(scale * j[1]) && lit(",") && num((double)j[2]) && (ij == num_parts - 1 || lit(","));
    }
    ok = ok && lit("]\n}") && (ip == num_people - 1 || lit(",\n"));
  }
  ok = ok && lit("]\n}\n");
  if (!ok) return RTP_ERANGE;
  *p = 0;
  return (long)(p - buf);
}
long rtp_format_json(char* buf, size_t buflen, const float* joints, int num_people, int num_parts, float frame_scale) {
  return format_json(buf, buflen, joints, num_people, num_parts, frame_scale, nullptr);
}
long rtp_format_json_tracked(char* buf, size_t buflen, const float* joints, int num_people, int num_parts, float frame_scale, const int* recs) {
  return format_json(buf, buflen, joints, num_people, num_parts, frame_scale, recs);
}

// The two narrow formats of maps mode (maps_export.hip computes the same bits on the device).  Each float operation is spelled as
// one statement: a multiply never feeds an add here, so no build of this file can contract one into an FMA.
int rtp_maps_quantize_u8(const float* v, size_t n, int is_paf, unsigned char* out) {
  if ((!v || !out) && n) return RTP_EINVAL;
  for (size_t i = 0; i < n; ++i) {
    float s;
    if (is_paf) {
      const float t = v[i] + 1.f;
      s = t * 127.5f;
    } else {
      s = v[i] * 255.f;
    }
    const float lo = fmaxf(s, 0.f);   // NaN -> 0
    const float hi = fminf(lo, 255.f);
    out[i] = (unsigned char)rintf(hi);  // round half to even (the default rounding mode)
  }
  return RTP_OK;
}

// float -> IEEE binary16, round to nearest even, in integer arithmetic on the bits
int rtp_maps_to_f16(const float* v, size_t n, uint16_t* out) {
  if ((!v || !out) && n) return RTP_EINVAL;
  for (size_t i = 0; i < n; ++i) {
    uint32_t b;
    memcpy(&b, &v[i], 4);
    const uint32_t sign = (b >> 16) & 0x8000u, a = b & 0x7fffffffu;
    uint32_t h;
    if (a > 0x7f800000u) h = 0x7e00u | ((a >> 13) & 0x1ffu);          // NaN (quiet, some payload kept)
    else if (a >= 0x47800000u) h = 0x7c00u;                            // >= 65536 (65520 .. 65536 round up through the carry below), inf
    else if (a >= 0x38800000u) {                                       // normal in binary16: drop 13 mantissa bits, carry may reach the exponent / inf
      const uint32_t m = a - 0x38000000u;                              // re-biased exponent (127 -> 15)
      h = (m + 0xfffu + ((m >> 13) & 1u)) >> 13;
    } else if (a >= 0x33000000u) {                                     // denormal in binary16: 2^-25 <= |v| < 2^-14
      const int shift = 126 - (int)(a >> 23);                          // mantissa with its hidden bit, shifted to units of 2^-24: 14 .. 24 bits dropped
      const uint32_t m = (a & 0x7fffffu) | 0x800000u;
      const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
      h = q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u);
    } else h = 0;                                                      // below half of the smallest denormal
    out[i] = (uint16_t)(sign | h);
  }
  return RTP_OK;
}

}  // extern "C"

// ---- crops mode: the one definition of its arithmetic (crops.hip computes the same bits on the device) ------------------------------

// What is wrong with the configuration for a model of model_parts parts, or nullptr.  The engine's switch reports the same text.
extern "C" const char* rtp_internal_crops_check(const rtp_crops_config* c, int model_parts) {
  if (!c) return "NULL rtp_crops_config";
  if (c->struct_size != sizeof(rtp_crops_config)) return "rtp_crops_config.struct_size is not this library's sizeof(rtp_crops_config)";
  if (model_parts < 1 || model_parts > RTP_MAX_NUM_PARTS) return "num_parts outside 1 .. RTP_MAX_NUM_PARTS";
  if (c->crop_w < RTP_CROP_MIN_SIZE || c->crop_w > RTP_CROP_MAX_SIZE) return "crop_w outside 8 .. 512";
  if (c->crop_h < RTP_CROP_MIN_SIZE || c->crop_h > RTP_CROP_MAX_SIZE) return "crop_h outside 8 .. 512";
  if (c->max_crops < 1 || c->max_crops > RTP_MAX_PEOPLE) return "max_crops outside 1 .. RTP_MAX_PEOPLE";
  if (!(c->min_score >= 0.f) || std::isinf(c->min_score)) return "min_score must be a finite number >= 0";
  if (c->min_parts < 1) return "min_parts must be >= 1";
  if (!(c->margin >= 0.f && c->margin <= 16.f)) return "margin outside 0 .. 16";
  if (c->layout != RTP_CROPS_HWC_BGR && c->layout != RTP_CROPS_CHW_RGB) return "layout is neither RTP_CROPS_HWC_BGR nor RTP_CROPS_CHW_RGB";
  if (c->parts) {
    if (c->num_parts < 1 || c->num_parts > RTP_MAX_NUM_PARTS) return "the part list's num_parts outside 1 .. RTP_MAX_NUM_PARTS";
    for (int i = 0; i < c->num_parts; ++i)
      if (c->parts[i] < 0 || c->parts[i] >= model_parts) return "a listed part is outside the model's parts";
  }
  return nullptr;
}

// rtp_crops_head_parts: nose, eyes and ears (COCO), head and neck (MPI)
extern "C" int rtp_crops_head_parts(int model, int parts[8]) {
  static const int coco[5] = {0, 14, 15, 16, 17}, mpi[2] = {0, 1};
  const bool c = model == RTP_MODEL_COCO_18;
  if (!c && model != RTP_MODEL_MPI_15) return RTP_EINVAL;
  const int n = c ? 5 : 2;
  memcpy(parts, c ? coco : mpi, n * sizeof(int));
  return n;
}

extern "C" {

int rtp_crop_people(const unsigned char* display_bgr, int w, int h, const float* joints, int num_people, int num_parts,
                    const rtp_crops_config* cfg, float* boxes, unsigned char* crops) {
#pragma clang fp contract(off)
  if (rtp_internal_crops_check(cfg, num_parts) || !boxes || w < 1 || h < 1 || w > 32768 || h > 32768 || num_people < 0) return RTP_EINVAL;
  if ((num_people > 0 && !joints) || (crops && !display_bgr)) return RTP_EINVAL;
  const int n = num_people < cfg->max_crops ? num_people : cfg->max_crops;
  const int nlist = cfg->parts ? cfg->num_parts : num_parts;
  const int cw = cfg->crop_w, ch = cfg->crop_h;
  const size_t crop_bytes = (size_t)cw * ch * 3;
  const float fcw = (float)cw, fch = (float)ch;
  for (int k = 0; k < n; ++k) {
    const float* jp = joints + (size_t)k * num_parts * 3;
    float* rec = boxes + (size_t)k * RTP_CROP_BOX_FLOATS;
    unsigned char* out = crops ? crops + (size_t)k * crop_bytes : nullptr;
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    int count = 0;
    for (int i = 0; i < nlist; ++i) {
      const int p = cfg->parts ? cfg->parts[i] : i;
      const float s = jp[3 * p + 2];
      if (!(s > cfg->min_score) || !std::isfinite(jp[3 * p]) || !std::isfinite(jp[3 * p + 1])) continue;
      const float x = jp[3 * p] + 0.0f, y = jp[3 * p + 1] + 0.0f;
      x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
      ++count;
    }
    bool valid = count >= cfg->min_parts;
    float left = 0.f, top = 0.f, bw = 0.f, bh = 0.f;
    if (valid) {
      const float sx = x0 + x1, sy = y0 + y1;
      const float cx = sx * 0.5f, cy = sy * 0.5f;
      bw = x1 - x0; bh = y1 - y0;
      const bool finite = std::isfinite(bw) && std::isfinite(bh);
      const float gm = cfg->margin * fmaxf(bw, bh);
      const float g = gm * 2.0f;
      const float wg = bw + g, hg = bh + g;
      bw = fmaxf(wg, 1.0f); bh = fmaxf(hg, 1.0f);
      const float wn = bh * fcw;
      const float wa = wn / fch;
      if (wa > bw) bw = wa;
      else { const float hn = bw * fch; bh = hn / fcw; }
      const float hw = bw * 0.5f, hh = bh * 0.5f;
      left = cx - hw; top = cy - hh;
      const float right = left + bw, bottom = top + bh;
      const float lim = 1048576.0f;
      valid = finite && fabsf(left) <= lim && fabsf(top) <= lim && fabsf(right) <= lim && fabsf(bottom) <= lim;
    }
    if (!valid) {
      rec[0] = rec[1] = rec[2] = rec[3] = 0.f; rec[4] = (float)count; rec[5] = 0.f;
      if (out) memset(out, 0, crop_bytes);
      continue;
    }
    rec[0] = left; rec[1] = top; rec[2] = bw; rec[3] = bh; rec[4] = (float)count; rec[5] = 1.f;
    if (!out) continue;
    const float lq = left * 65536.0f, tq = top * 65536.0f;
    const float stx = bw / fcw, sty = bh / fch;
    const float dxq = stx * 65536.0f, dyq = sty * 65536.0f;
    const long long ox = (long long)rintf(lq), oy = (long long)rintf(tq);
    const long long dx = (long long)rintf(dxq), dy = (long long)rintf(dyq);
    const int Sx = dx <= 98304 ? 1 : dx <= 196608 ? 2 : 4, Sy = dy <= 98304 ? 1 : dy <= 196608 ? 2 : 4;
    const long long half = (long long)Sx * Sy * 2097152, den = (long long)Sx * Sy * 4194304;
    for (int j = 0; j < ch; ++j)
      for (int i = 0; i < cw; ++i) {
        long long T[3] = {0, 0, 0};
        for (int b = 0; b < Sy; ++b) {
          const long long py = oy + j * dy + ((2 * b + 1) * dy) / (2 * Sy) - 32768;
          const long long Y = py >> 16, fy = ((py & 65535) + 16) >> 5;
          for (int a = 0; a < Sx; ++a) {
            const long long px = ox + i * dx + ((2 * a + 1) * dx) / (2 * Sx) - 32768;
            const long long X = px >> 16, fx = ((px & 65535) + 16) >> 5;
            for (int c = 0; c < 3; ++c) {
              long long p[2][2];
              for (int r = 0; r < 2; ++r)
                for (int q = 0; q < 2; ++q) {
                  const long long yy = Y + r, xx = X + q;
                  p[r][q] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? display_bgr[((size_t)yy * w + xx) * 3 + c] : 0;
                }
              T[c] += (2048 - fy) * ((2048 - fx) * p[0][0] + fx * p[0][1]) + fy * ((2048 - fx) * p[1][0] + fx * p[1][1]);
            }
          }
        }
        for (int c = 0; c < 3; ++c) {
          const unsigned char v = (unsigned char)((T[c] + half) / den);
          if (cfg->layout == RTP_CROPS_HWC_BGR) out[((size_t)j * cw + i) * 3 + c] = v;
          else out[((size_t)(2 - c) * ch + j) * cw + i] = v;
        }
      }
  }
  return n;
}

}  // extern "C"

// ---- tracking mode: the one definition of its arithmetic (track.hip computes the same integers and float bits on the device) --------

// What is wrong with the configuration, or nullptr.  The engine's switch reports the same text.
extern "C" const char* rtp_internal_track_check(const rtp_track_config* c) {
  if (!c) return "NULL rtp_track_config";
  if (c->struct_size != sizeof(rtp_track_config)) return "rtp_track_config.struct_size is not this library's sizeof(rtp_track_config)";
  if (!(c->min_score >= 0.f) || std::isinf(c->min_score)) return "min_score must be a finite number >= 0";
  if (c->min_parts < 1) return "min_parts must be >= 1";
  if (c->min_common < 1) return "min_common must be >= 1";
  if (!(c->max_cost > 0.f) || std::isinf(c->max_cost)) return "max_cost must be a finite number > 0";
  if (c->max_misses < 0) return "max_misses must be >= 0";
  return nullptr;
}

extern "C" {

int rtp_track_config_default(rtp_track_config* cfg) {
  if (!cfg) return RTP_EINVAL;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = (unsigned)sizeof *cfg;
  cfg->min_score = 0.f;
  cfg->min_parts = 3;
  cfg->min_common = 2;
  cfg->max_cost = 0.0625f;
  cfg->max_misses = 15;
  return RTP_OK;
}

int rtp_track_state_init(rtp_track_state* state, int num_parts) {
  if (!state || num_parts < 1 || num_parts > RTP_MAX_NUM_PARTS) return RTP_EINVAL;
  memset(state, 0, sizeof *state);
  state->struct_size = (unsigned)sizeof *state;
  state->num_parts = num_parts;
  state->next_id = 1;
  return RTP_OK;
}

int rtp_track_update(rtp_track_state* st, const rtp_track_config* cfg, const float* joints, int num_people, int* recs) {
#pragma clang fp contract(off)
  if (!st || !recs || rtp_internal_track_check(cfg)) return RTP_EINVAL;
  if (st->struct_size != sizeof(rtp_track_state) || st->num_parts < 1 || st->num_parts > RTP_MAX_NUM_PARTS) return RTP_EINVAL;
  const int n = num_people < 0 ? 0 : num_people > RTP_MAX_PEOPLE ? RTP_MAX_PEOPLE : num_people;
  if (n > 0 && !joints) return RTP_EINVAL;
  const int P = st->num_parts;
  auto counts = [&](const float* j) { return j[2] > cfg->min_score && std::isfinite(j[0]) && std::isfinite(j[1]); };
  // 1. trackable people
  bool trackable[RTP_MAX_PEOPLE];
  for (int k = 0; k < n; ++k) {
    int c = 0;
    for (int p = 0; p < P; ++p) c += counts(joints + ((size_t)k * P + p) * 3) ? 1 : 0;
    trackable[k] = c >= cfg->min_parts;
  }
  // 2. the candidates, as keys (cost bits, slot, person)
  struct Cand { uint32_t bits; int t, k; };
  std::vector<Cand> cand;
  for (int t = 0; t < RTP_MAX_TRACKS; ++t) {
    if (!st->id[t]) continue;
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int p = 0; p < P; ++p) {
      const float* tj = st->joints[t][p];
      if (!counts(tj)) continue;
      const float x = tj[0] + 0.0f, y = tj[1] + 0.0f;
      x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
    }
    const float w = x1 - x0, h = y1 - y0;
    const float ww = w * w, hh = h * h;
    const float wh = ww + hh;
    const float d = fmaxf(wh, 1.0f);
    for (int k = 0; k < n; ++k) {
      if (!trackable[k]) continue;
      float s = 0.0f;
      int m = 0;
      for (int p = 0; p < P; ++p) {
        const float* pj = joints + ((size_t)k * P + p) * 3;
        const float* tj = st->joints[t][p];
        if (!counts(pj) || !counts(tj)) continue;
        const float dx = pj[0] - tj[0], dy = pj[1] - tj[1];
        const float a = dx * dx, b = dy * dy;
        const float c = a + b;
        s = s + c;
        ++m;
      }
      if (m < cfg->min_common) continue;
      const float q = s / (float)m;
      const float cost = q / d;
      if (!std::isfinite(cost) || !(cost <= cfg->max_cost)) continue;
      const float cz = cost + 0.0f;
      Cand c;
      memcpy(&c.bits, &cz, 4);
      c.t = t; c.k = k;
      cand.push_back(c);
    }
  }
  // 3. greedy assignment in key order
  std::sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) { return a.bits != b.bits ? a.bits < b.bits : a.t != b.t ? a.t < b.t : a.k < b.k; });
  int slot_of[RTP_MAX_PEOPLE], person_of[RTP_MAX_TRACKS];
  uint32_t cost_of[RTP_MAX_PEOPLE];
  for (int k = 0; k < RTP_MAX_PEOPLE; ++k) { slot_of[k] = -1; cost_of[k] = 0; }
  for (int t = 0; t < RTP_MAX_TRACKS; ++t) person_of[t] = -1;
  for (const Cand& c : cand) {
    if (person_of[c.t] >= 0 || slot_of[c.k] >= 0) continue;
    person_of[c.t] = c.k; slot_of[c.k] = c.t; cost_of[c.k] = c.bits;
  }
  // 4. matched slots, 5. unmatched live slots
  for (int t = 0; t < RTP_MAX_TRACKS; ++t) {
    if (!st->id[t]) continue;
    if (person_of[t] >= 0) {
      memcpy(st->joints[t], joints + (size_t)person_of[t] * P * 3, (size_t)P * 3 * sizeof(float));
      st->hits[t]++;
      st->misses[t] = 0;
    } else if (++st->misses[t] > cfg->max_misses) {
      st->id[t] = st->hits[t] = st->misses[t] = 0;
      memset(st->joints[t], 0, sizeof st->joints[t]);
    }
  }
  // 6. births: the lowest free slot for each unmatched trackable person, in person order
  bool born[RTP_MAX_PEOPLE] = {};
  int free_t = 0;
  for (int k = 0; k < n; ++k) {
    if (!trackable[k] || slot_of[k] >= 0) continue;
    while (free_t < RTP_MAX_TRACKS && st->id[free_t]) ++free_t;
    if (free_t == RTP_MAX_TRACKS) break;
    if (st->next_id == 0) st->next_id = 1;
    st->id[free_t] = (int)st->next_id++;
    if (st->next_id == 0) st->next_id = 1;
    st->hits[free_t] = 1;
    st->misses[free_t] = 0;
    memcpy(st->joints[free_t], joints + (size_t)k * P * 3, (size_t)P * 3 * sizeof(float));
    slot_of[k] = free_t;
    born[k] = true;
  }
  st->frames++;   // 7.
  for (int k = 0; k < n; ++k) {
    int* r = recs + (size_t)k * RTP_TRACK_REC_INTS;
    const int t = slot_of[k];
    if (t < 0) { r[0] = 0; r[1] = -1; r[2] = 0; r[3] = 0; continue; }
    r[0] = st->id[t]; r[1] = t; r[2] = st->hits[t];
    r[3] = born[k] ? 0 : (int)cost_of[k];
  }
  return n;
}

}  // extern "C"

// ---- appearance-aided tracking: the one definition of its arithmetic (appearance.hip and track.hip's appearance form compute the same
// integers and float bits on the device) ------------------------------------------------------------------------------------------

// What is wrong with the fields the cost and the table update read, or nullptr
static const char* appearance_check_fields(const rtp_appearance_config* c) {
  if (!c) return "NULL rtp_appearance_config";
  if (c->struct_size != sizeof(rtp_appearance_config)) return "rtp_appearance_config.struct_size is not this library's sizeof(rtp_appearance_config)";
  if (!(c->min_score >= 0.f) || std::isinf(c->min_score)) return "min_score must be a finite number >= 0";
  if (c->min_parts < 1) return "min_parts must be >= 1";
  if (!(c->margin >= 0.f && c->margin <= 16.f)) return "margin outside 0 .. 16";
  if (!(c->weight >= 0.f) || std::isinf(c->weight)) return "weight must be a finite number >= 0";
  if (!(c->max_dist > 0.f && c->max_dist <= 1.f)) return "max_dist outside (0, 1]";
  if (!(c->unknown >= 0.f && c->unknown <= 1.f)) return "unknown outside 0 .. 1";
  if (c->rate < 1 || c->rate > 256) return "rate outside 1 .. 256";
  return nullptr;
}

// What is wrong with the configuration for a model of model_parts parts, or nullptr.  The engine's switch reports the same text.
extern "C" const char* rtp_internal_appearance_check(const rtp_appearance_config* c, int model_parts) {
  if (const char* bad = appearance_check_fields(c)) return bad;
  if (model_parts < 1 || model_parts > RTP_MAX_NUM_PARTS) return "num_parts outside 1 .. RTP_MAX_NUM_PARTS";
  if (c->parts) {
    if (c->num_parts < 1 || c->num_parts > RTP_MAX_NUM_PARTS) return "the part list's num_parts outside 1 .. RTP_MAX_NUM_PARTS";
    for (int i = 0; i < c->num_parts; ++i)
      if (c->parts[i] < 0 || c->parts[i] >= model_parts) return "a listed part is outside the model's parts";
  }
  return nullptr;
}

// rtp_appearance_torso_parts: neck, shoulders and hips (COCO), and the chest (MPI)
extern "C" int rtp_appearance_torso_parts(int model, int parts[8]) {
  static const int coco[5] = {1, 2, 5, 8, 11}, mpi[6] = {1, 2, 5, 8, 11, 14};
  const bool c = model == RTP_MODEL_COCO_18;
  if (!parts || (!c && model != RTP_MODEL_MPI_15)) return RTP_EINVAL;
  const int n = c ? 5 : 6;
  memcpy(parts, c ? coco : mpi, n * sizeof(int));
  return n;
}

// The configuration's list for a model of model_parts parts (checked): its own, the torso parts of a model of 18 or 15 parts, or all parts
extern "C" int rtp_internal_appearance_list(const rtp_appearance_config* c, int model_parts, int list[RTP_MAX_NUM_PARTS]) {
  if (c->parts) {
    memcpy(list, c->parts, (size_t)c->num_parts * sizeof(int));
    return c->num_parts;
  }
  if (model_parts == 18 || model_parts == 15) return rtp_appearance_torso_parts(model_parts == 18 ? RTP_MODEL_COCO_18 : RTP_MODEL_MPI_15, list);
  for (int p = 0; p < model_parts; ++p) list[p] = p;
  return model_parts;
}

extern "C" {

int rtp_appearance_config_default(rtp_appearance_config* cfg) {
  if (!cfg) return RTP_EINVAL;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = (unsigned)sizeof *cfg;
  cfg->min_score = 0.f;
  cfg->min_parts = 3;
  cfg->margin = 0.f;
  cfg->weight = 0.125f;
  cfg->max_dist = 1.f;
  cfg->unknown = 0.25f;
  cfg->rate = 32;
  return RTP_OK;
}

int rtp_appearance_state_init(rtp_appearance_state* state) {
  if (!state) return RTP_EINVAL;
  memset(state, 0, sizeof *state);
  state->struct_size = (unsigned)sizeof *state;
  return RTP_OK;
}

int rtp_appearance_describe(const unsigned char* display_bgr, int w, int h, const float* joints, int num_people, int num_parts,
                            const rtp_appearance_config* cfg, uint16_t* bins_out, unsigned char* valid_out) {
#pragma clang fp contract(off)
  if (rtp_internal_appearance_check(cfg, num_parts) || !bins_out || !valid_out || w < 1 || h < 1 || w > 32768 || h > 32768 || num_people < 0) return RTP_EINVAL;
  if (num_people > 0 && (!joints || !display_bgr)) return RTP_EINVAL;
  const int n = num_people < RTP_MAX_PEOPLE ? num_people : RTP_MAX_PEOPLE;
  int list[RTP_MAX_NUM_PARTS];
  const int nlist = rtp_internal_appearance_list(cfg, num_parts, list);
  for (int k = 0; k < n; ++k) {
    const float* jp = joints + (size_t)k * num_parts * 3;
    uint16_t* bins = bins_out + (size_t)k * RTP_APPEARANCE_BINS;
    memset(bins, 0, RTP_APPEARANCE_BINS * sizeof(uint16_t));
    valid_out[k] = 0;
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    int count = 0;
    for (int i = 0; i < nlist; ++i) {
      const int p = list[i];
      const float s = jp[3 * p + 2];
      if (!(s > cfg->min_score) || !std::isfinite(jp[3 * p]) || !std::isfinite(jp[3 * p + 1])) continue;
      const float x = jp[3 * p] + 0.0f, y = jp[3 * p + 1] + 0.0f;
      x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
      ++count;
    }
    if (count < cfg->min_parts) continue;
    const float sx = x0 + x1, sy = y0 + y1;
    const float cx = sx * 0.5f, cy = sy * 0.5f;
    float bw = x1 - x0, bh = y1 - y0;
    if (!std::isfinite(bw) || !std::isfinite(bh)) continue;
    const float gm = cfg->margin * fmaxf(bw, bh);
    const float g = gm * 2.0f;
    const float wg = bw + g, hg = bh + g;
    bw = fmaxf(wg, 1.0f); bh = fmaxf(hg, 1.0f);
    const float hw = bw * 0.5f, hh = bh * 0.5f;
    const float left = cx - hw, top = cy - hh;
    const float right = left + bw, bottom = top + bh;
    const float lim = 1048576.0f;
    if (!(fabsf(left) <= lim && fabsf(top) <= lim && fabsf(right) <= lim && fabsf(bottom) <= lim)) continue;
    const float lq = left * 65536.0f, tq = top * 65536.0f;
    const float stx = bw / 32.0f, sty = bh / 32.0f;
    const float dxq = stx * 65536.0f, dyq = sty * 65536.0f;
    const long long ox = (long long)rintf(lq), oy = (long long)rintf(tq);
    const long long dx = (long long)rintf(dxq), dy = (long long)rintf(dyq);
    for (int j = 0; j < RTP_APPEARANCE_GRID; ++j) {
      long long row = (oy + j * dy + dy / 2) >> 16;
      row = row < 0 ? 0 : row > h - 1 ? h - 1 : row;
      for (int i = 0; i < RTP_APPEARANCE_GRID; ++i) {
        long long col = (ox + i * dx + dx / 2) >> 16;
        col = col < 0 ? 0 : col > w - 1 ? w - 1 : col;
        const unsigned char* px = display_bgr + ((size_t)row * w + (size_t)col) * 3;
        bins[(j >= 16 ? 64 : 0) + (px[2] >> 6) * 16 + (px[1] >> 6) * 4 + (px[0] >> 6)]++;
      }
    }
    valid_out[k] = 1;
  }
  return n;
}

int rtp_track_update_appearance(rtp_track_state* st, rtp_appearance_state* ap, const rtp_track_config* cfg, const rtp_appearance_config* acfg,
                                const float* joints, int num_people, const uint16_t* bins, const unsigned char* valid, int* recs) {
#pragma clang fp contract(off)
  if (!st || !ap || !recs || rtp_internal_track_check(cfg) || appearance_check_fields(acfg)) return RTP_EINVAL;
  if (st->struct_size != sizeof(rtp_track_state) || st->num_parts < 1 || st->num_parts > RTP_MAX_NUM_PARTS) return RTP_EINVAL;
  if (ap->struct_size != sizeof(rtp_appearance_state) || (bins && !valid)) return RTP_EINVAL;
  const int n = num_people < 0 ? 0 : num_people > RTP_MAX_PEOPLE ? RTP_MAX_PEOPLE : num_people;
  if (n > 0 && !joints) return RTP_EINVAL;
  const int P = st->num_parts;
  auto counts = [&](const float* j) { return j[2] > cfg->min_score && std::isfinite(j[0]) && std::isfinite(j[1]); };
  auto described = [&](int k) { return bins && valid[k] != 0; };
  // 1. trackable people
  bool trackable[RTP_MAX_PEOPLE];
  for (int k = 0; k < n; ++k) {
    int c = 0;
    for (int p = 0; p < P; ++p) c += counts(joints + ((size_t)k * P + p) * 3) ? 1 : 0;
    trackable[k] = c >= cfg->min_parts;
  }
  // 2. the candidates, as keys (total bits, slot, person): the motion cost and its gate, then THE COST
  struct Cand { uint32_t bits; int t, k; };
  std::vector<Cand> cand;
  for (int t = 0; t < RTP_MAX_TRACKS; ++t) {
    if (!st->id[t]) continue;
    const bool has = ap->owner[t] == st->id[t];
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int p = 0; p < P; ++p) {
      const float* tj = st->joints[t][p];
      if (!counts(tj)) continue;
      const float x = tj[0] + 0.0f, y = tj[1] + 0.0f;
      x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
    }
    const float w = x1 - x0, h = y1 - y0;
    const float ww = w * w, hh = h * h;
    const float wh = ww + hh;
    const float d = fmaxf(wh, 1.0f);
    for (int k = 0; k < n; ++k) {
      if (!trackable[k]) continue;
      float s = 0.0f;
      int m = 0;
      for (int p = 0; p < P; ++p) {
        const float* pj = joints + ((size_t)k * P + p) * 3;
        const float* tj = st->joints[t][p];
        if (!counts(pj) || !counts(tj)) continue;
        const float dx = pj[0] - tj[0], dy = pj[1] - tj[1];
        const float a = dx * dx, b = dy * dy;
        const float c = a + b;
        s = s + c;
        ++m;
      }
      if (m < cfg->min_common) continue;
      const float q = s / (float)m;
      const float cost = q / d;
      if (!std::isfinite(cost) || !(cost <= cfg->max_cost)) continue;
      float a = acfg->unknown;
      if (has && described(k)) {
        const uint16_t* bk = bins + (size_t)k * RTP_APPEARANCE_BINS;
        int L = 0;
        for (int b = 0; b < RTP_APPEARANCE_BINS; ++b) {
          const int v = (int)ap->desc[t][b] - 16 * (int)bk[b];
          L += v < 0 ? -v : v;
        }
        a = (float)L / 32768.0f;
        if (!(a <= acfg->max_dist)) continue;
      }
      const float wa = acfg->weight * a;
      const float total = cost + wa;
      if (!std::isfinite(total)) continue;
      const float tz = total + 0.0f;
      Cand c;
      memcpy(&c.bits, &tz, 4);
      c.t = t; c.k = k;
      cand.push_back(c);
    }
  }
  // 3. greedy assignment in key order
  std::sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) { return a.bits != b.bits ? a.bits < b.bits : a.t != b.t ? a.t < b.t : a.k < b.k; });
  int slot_of[RTP_MAX_PEOPLE], person_of[RTP_MAX_TRACKS];
  uint32_t cost_of[RTP_MAX_PEOPLE];
  for (int k = 0; k < RTP_MAX_PEOPLE; ++k) { slot_of[k] = -1; cost_of[k] = 0; }
  for (int t = 0; t < RTP_MAX_TRACKS; ++t) person_of[t] = -1;
  for (const Cand& c : cand) {
    if (person_of[c.t] >= 0 || slot_of[c.k] >= 0) continue;
    person_of[c.t] = c.k; slot_of[c.k] = c.t; cost_of[c.k] = c.bits;
  }
  // 4. matched slots, 5. unmatched live slots
  for (int t = 0; t < RTP_MAX_TRACKS; ++t) {
    if (!st->id[t]) continue;
    if (person_of[t] >= 0) {
      memcpy(st->joints[t], joints + (size_t)person_of[t] * P * 3, (size_t)P * 3 * sizeof(float));
      st->hits[t]++;
      st->misses[t] = 0;
    } else if (++st->misses[t] > cfg->max_misses) {
      st->id[t] = st->hits[t] = st->misses[t] = 0;
      memset(st->joints[t], 0, sizeof st->joints[t]);
    }
  }
  // 6. births: the lowest free slot for each unmatched trackable person, in person order
  bool born[RTP_MAX_PEOPLE] = {};
  int free_t = 0;
  for (int k = 0; k < n; ++k) {
    if (!trackable[k] || slot_of[k] >= 0) continue;
    while (free_t < RTP_MAX_TRACKS && st->id[free_t]) ++free_t;
    if (free_t == RTP_MAX_TRACKS) break;
    if (st->next_id == 0) st->next_id = 1;
    st->id[free_t] = (int)st->next_id++;
    if (st->next_id == 0) st->next_id = 1;
    st->hits[free_t] = 1;
    st->misses[free_t] = 0;
    memcpy(st->joints[free_t], joints + (size_t)k * P * 3, (size_t)P * 3 * sizeof(float));
    slot_of[k] = free_t;
    born[k] = true;
  }
  // THE TABLE UPDATE
  for (int k = 0; k < n; ++k) {
    const int t = slot_of[k];
    if (t < 0 || !described(k)) continue;
    const uint16_t* bk = bins + (size_t)k * RTP_APPEARANCE_BINS;
    if (ap->owner[t] == st->id[t]) {
      for (int b = 0; b < RTP_APPEARANCE_BINS; ++b)
        ap->desc[t][b] = (uint16_t)(((int)ap->desc[t][b] * (256 - acfg->rate) + 16 * (int)bk[b] * acfg->rate + 128) >> 8);
    } else {
      for (int b = 0; b < RTP_APPEARANCE_BINS; ++b) ap->desc[t][b] = (uint16_t)(16 * (int)bk[b]);
      ap->owner[t] = st->id[t];
    }
  }
  st->frames++;   // 7.
  for (int k = 0; k < n; ++k) {
    int* r = recs + (size_t)k * RTP_TRACK_REC_INTS;
    const int t = slot_of[k];
    if (t < 0) { r[0] = 0; r[1] = -1; r[2] = 0; r[3] = 0; continue; }
    r[0] = st->id[t]; r[1] = t; r[2] = st->hits[t];
    r[3] = born[k] ? 0 : (int)cost_of[k];
  }
  return n;
}

}  // extern "C"

// ---- smoothing mode: the one definition of its arithmetic (smooth.hip computes the same float bits and bytes on the device) ---------

// What is wrong with the configuration, or nullptr.  The engine's switch reports the same text.
extern "C" const char* rtp_internal_smooth_check(const rtp_smooth_config* c) {
  if (!c) return "NULL rtp_smooth_config";
  if (c->struct_size != sizeof(rtp_smooth_config)) return "rtp_smooth_config.struct_size is not this library's sizeof(rtp_smooth_config)";
  if (!(c->min_score >= 0.f) || std::isinf(c->min_score)) return "min_score must be a finite number >= 0";
  if (!(c->min_cutoff > 0.f) || std::isinf(c->min_cutoff)) return "min_cutoff must be a finite number > 0";
  if (!(c->beta >= 0.f) || std::isinf(c->beta)) return "beta must be a finite number >= 0";
  if (!(c->d_cutoff > 0.f) || std::isinf(c->d_cutoff)) return "d_cutoff must be a finite number > 0";
  if (c->max_hold < 0 || c->max_hold > RTP_SMOOTH_MAX_HOLD) return "max_hold must be 0 .. 1000";
  if (c->apply & ~(unsigned)(RTP_SMOOTH_RENDER | RTP_SMOOTH_CROPS)) return "apply must be a mask of RTP_SMOOTH_RENDER and RTP_SMOOTH_CROPS";
  return nullptr;
}

extern "C" {

int rtp_smooth_config_default(rtp_smooth_config* cfg) {
  if (!cfg) return RTP_EINVAL;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = (unsigned)sizeof *cfg;
  cfg->min_score = 0.f;
  cfg->min_cutoff = 1.0f / 30.0f;
  cfg->beta = 0.01f;
  cfg->d_cutoff = 1.0f / 30.0f;
  cfg->max_hold = 5;
  cfg->apply = 0;
  return RTP_OK;
}

int rtp_smooth_state_init(rtp_smooth_state* state, int num_parts) {
  if (!state || num_parts < 1 || num_parts > RTP_MAX_NUM_PARTS) return RTP_EINVAL;
  memset(state, 0, sizeof *state);
  state->struct_size = (unsigned)sizeof *state;
  state->num_parts = num_parts;
  return RTP_OK;
}

int rtp_smooth_update(rtp_smooth_state* st, const rtp_smooth_config* cfg, const float* joints, int num_people, const int* recs, float* joints_s,
                      float* vel, unsigned char* flags) {
#pragma clang fp contract(off)
  if (!st || !joints_s || rtp_internal_smooth_check(cfg)) return RTP_EINVAL;
  if (st->struct_size != sizeof(rtp_smooth_state) || st->num_parts < 1 || st->num_parts > RTP_MAX_NUM_PARTS) return RTP_EINVAL;
  const int n = num_people < 0 ? 0 : num_people > RTP_MAX_PEOPLE ? RTP_MAX_PEOPLE : num_people;
  if (n > 0 && (!joints || !recs)) return RTP_EINVAL;
  bool taken[RTP_MAX_TRACKS] = {};
  for (int k = 0; k < n; ++k) {
    const int* r = recs + (size_t)k * RTP_TRACK_REC_INTS;
    if (r[0] == 0) continue;
    if (r[1] < 0 || r[1] >= RTP_MAX_TRACKS || taken[r[1]]) return RTP_EINVAL;
    taken[r[1]] = true;
  }
  const int P = st->num_parts;
  const float TWO_PI = 6.2831855f;
  const unsigned max_hold = (unsigned)cfg->max_hold;
  // 1.
  st->frames++;
  if (st->frames == 0) st->frames = 1;
  const unsigned now = st->frames;
  for (int k = 0; k < n; ++k) {
    const int id = recs[(size_t)k * RTP_TRACK_REC_INTS], t = recs[(size_t)k * RTP_TRACK_REC_INTS + 1];
    for (int p = 0; p < P; ++p) {
      const size_t i = (size_t)k * P + p;
      const float* j = joints + i * 3;
      const float x = j[0], y = j[1], score = j[2];
      const bool counts = score > cfg->min_score && std::isfinite(x) && std::isfinite(y);
      float o[3], ov[2] = {0.0f, 0.0f};
      unsigned char flag = RTP_SMOOTH_FLAG_NONE;
      memcpy(o, j, sizeof o);
      if (id == 0) {   // 2.
        flag = counts ? RTP_SMOOTH_FLAG_START : RTP_SMOOTH_FLAG_NONE;
      } else {         // 3.
        rtp_smooth_cell& c = st->cell[t][p];
        const bool live = c.owner == id && c.last != 0;
        const unsigned g = now - c.last;
        bool start = counts && (!live || g - 1u > max_hold);
        if (counts && !start) {
          const float dt = (float)g;
          const float v2[2] = {x, y};
          float nh[2], ne[2];
          for (int a2 = 0; a2 < 2; ++a2) {
            const float v = v2[a2], vh = c.pos[a2], dvh = c.vel[a2];
            const float d = v - vh;
            const float dv = d / dt;
            float rd = TWO_PI * cfg->d_cutoff;
            rd = rd * dt;
            const float rd1 = rd + 1.0f;
            const float ad = rd / rd1;
            const float t1 = ad * dv;
            const float ad1 = 1.0f - ad;
            const float t2 = ad1 * dvh;
            const float e = t1 + t2;
            float fc = cfg->beta * fabsf(e);
            fc = cfg->min_cutoff + fc;
            float r = TWO_PI * fc;
            r = r * dt;
            const float r1 = r + 1.0f;
            const float a = r / r1;
            const float u1 = a * v;
            const float a1 = 1.0f - a;
            const float u2 = a1 * vh;
            nh[a2] = u1 + u2;
            ne[a2] = e;
          }
          if (std::isfinite(nh[0]) && std::isfinite(nh[1]) && std::isfinite(ne[0]) && std::isfinite(ne[1])) {
            c.pos[0] = nh[0]; c.pos[1] = nh[1]; c.vel[0] = ne[0]; c.vel[1] = ne[1]; c.score = score; c.last = now;
            o[0] = nh[0]; o[1] = nh[1];
            ov[0] = ne[0]; ov[1] = ne[1];
            flag = RTP_SMOOTH_FLAG_FILTER;
          } else {
            start = true;
          }
        }
        if (start) {
          c.owner = id; c.last = now; c.pos[0] = x; c.pos[1] = y; c.vel[0] = 0.0f; c.vel[1] = 0.0f; c.score = score;
          flag = RTP_SMOOTH_FLAG_START;
        } else if (!counts) {
          if (live && g <= max_hold) {
            memcpy(o, c.pos, 2 * sizeof(float));
            memcpy(o + 2, &c.score, sizeof(float));
            memcpy(ov, c.vel, sizeof ov);
            flag = RTP_SMOOTH_FLAG_HELD;
          } else {
            flag = RTP_SMOOTH_FLAG_NONE;
          }
        }
      }
      memcpy(joints_s + i * 3, o, sizeof o);
      if (vel) memcpy(vel + i * 2, ov, sizeof ov);
      if (flags) flags[i] = flag;
    }
  }
  return n;
}

}  // extern "C"

// ---- overlay mode: the one definition of its draw list and its pixels (overlay.hip computes the same integers and bytes on the device)

// What is wrong with the configuration, or nullptr.  The engine's switch reports the same text.
extern "C" const char* rtp_internal_overlay_check(const rtp_overlay_config* c) {
  if (!c) return "NULL rtp_overlay_config";
  if (c->struct_size != sizeof(rtp_overlay_config)) return "rtp_overlay_config.struct_size is not this library's sizeof(rtp_overlay_config)";
  if (c->what == 0 || (c->what & ~(unsigned)(RTP_OVERLAY_BOX | RTP_OVERLAY_LABEL | RTP_OVERLAY_TRAIL))) return "what must be a non-empty mask of RTP_OVERLAY_BOX, RTP_OVERLAY_LABEL and RTP_OVERLAY_TRAIL";
  if (!(c->min_score >= 0.f) || std::isinf(c->min_score)) return "min_score must be a finite number >= 0";
  if (c->box_margin < 0 || c->box_margin > RTP_OVERLAY_MAX_MARGIN) return "box_margin must be 0 .. 1024";
  if (c->line_width < 1 || c->line_width > 16) return "line_width must be 1 .. 16";
  if (c->label_scale < 1 || c->label_scale > 8) return "label_scale must be 1 .. 8";
  if (c->trail_len < 0 || c->trail_len > RTP_TRAIL_MAX) return "trail_len must be 0 .. 32";
  if (c->trail_radius < 0 || c->trail_radius > 16) return "trail_radius must be 0 .. 16";
  if (c->alpha < 0 || c->alpha > 256) return "alpha must be 0 .. 256";
  return nullptr;
}

// What is wrong with the trail table (but its num_parts), or nullptr
extern "C" const char* rtp_internal_trail_check(const rtp_trail_state* st) {
  if (!st) return "NULL rtp_trail_state";
  if (st->struct_size != sizeof(rtp_trail_state)) return "rtp_trail_state.struct_size is not this library's sizeof(rtp_trail_state)";
  for (int t = 0; t < RTP_MAX_TRACKS; ++t)
    if (st->slot[t].count < 0 || st->slot[t].count > RTP_TRAIL_MAX || st->slot[t].head < 0 || st->slot[t].head >= RTP_TRAIL_MAX) return "a ring's count must be 0 .. 32 and its head 0 .. 31";
  return nullptr;
}

namespace {

const int kOverlayPalette[16] = RTP_OVERLAY_PALETTE;
const unsigned char kOverlayFont[10][7] = RTP_OVERLAY_FONT;

int overlay_round(float v) {
#pragma clang fp contract(off)
  v = v < -32767.0f ? -32767.0f : v > 32767.0f ? 32767.0f : v;
  return (int)floorf(v + 0.5f);
}

// steps 1 and 2 for one person: false = no counting part; box = {x0, y0, x1, y1} with the margin
bool overlay_box(const float* j, int P, float min_score, int margin, int box[4]) {
  float fx0 = 0.f, fx1 = 0.f, fy0 = 0.f, fy1 = 0.f;
  bool any = false;
  for (int p = 0; p < P; ++p) {
    const float x = j[3 * p], y = j[3 * p + 1], s = j[3 * p + 2];
    if (!(s > min_score) || !std::isfinite(x) || !std::isfinite(y)) continue;
    if (!any) { fx0 = fx1 = x; fy0 = fy1 = y; any = true; continue; }
    if (x < fx0) fx0 = x;
    if (x > fx1) fx1 = x;
    if (y < fy0) fy0 = y;
    if (y > fy1) fy1 = y;
  }
  if (!any) return false;
  box[0] = overlay_round(fx0) - margin; box[1] = overlay_round(fy0) - margin;
  box[2] = overlay_round(fx1) + margin; box[3] = overlay_round(fy1) + margin;
  return true;
}

int overlay_digits(unsigned v) {
  int d = 1;
  while (v >= 10u) { v /= 10u; ++d; }
  return d;
}

int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// 0: the item does not cover (px, py); 1: with its colour; 2: with the text colour.  `it` has been clamped (rtp_overlay_draw).
int overlay_covers(const int* it, const int* digit, int ndig, int px, int py) {
  const int x0 = it[1], y0 = it[2], x1 = it[3], y1 = it[4], size = it[5];
  switch (it[0]) {
    case RTP_OVERLAY_KIND_RECT:
      if (px < x0 || px > x1 || py < y0 || py > y1) return 0;
      return px - x0 < size || x1 - px < size || py - y0 < size || y1 - py < size;
    case RTP_OVERLAY_KIND_CAPSULE: {
      const long long dx = (long long)x1 - x0, dy = (long long)y1 - y0, ux = (long long)px - x0, uy = (long long)py - y0, r2 = (long long)size * size;
      const long long L = dx * dx + dy * dy, t = ux * dx + uy * dy;
      if (L == 0 || t < 0) return ux * ux + uy * uy <= r2;
      if (t > L) { const long long vx = (long long)px - x1, vy = (long long)py - y1; return vx * vx + vy * vy <= r2; }
      long long cross = ux * dy - uy * dx;
      if (cross < 0) cross = -cross;
      if (cross > (1LL << 31)) cross = 1LL << 31;
      return cross * cross <= r2 * L;
    }
    case RTP_OVERLAY_KIND_LABEL: {
      if (px < x0 || px > x1 || py < y0 || py > y1) return 0;
      const int u = (px - x0) / size, v = (py - y0) / size;
      if (v < 1 || v > 7 || u < 1) return 1;
      const int c = (u - 1) % 6, i = (u - 1) / 6;
      if (c >= 5 || i >= ndig) return 1;
      return (kOverlayFont[digit[i]][v - 1] >> (4 - c)) & 1 ? 2 : 1;
    }
    default: return 0;
  }
}

}  // namespace

extern "C" {

int rtp_overlay_config_default(rtp_overlay_config* cfg) {
  if (!cfg) return RTP_EINVAL;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = (unsigned)sizeof *cfg;
  cfg->what = RTP_OVERLAY_BOX | RTP_OVERLAY_LABEL | RTP_OVERLAY_TRAIL;
  cfg->min_score = 0.f;
  cfg->box_margin = 4;
  cfg->line_width = 2;
  cfg->label_scale = 1;
  cfg->trail_len = 16;
  cfg->trail_radius = 1;
  cfg->alpha = 192;
  return RTP_OK;
}

int rtp_trail_state_init(rtp_trail_state* state, int num_parts) {
  if (!state || num_parts < 1 || num_parts > RTP_MAX_NUM_PARTS) return RTP_EINVAL;
  memset(state, 0, sizeof *state);
  state->struct_size = (unsigned)sizeof *state;
  state->num_parts = num_parts;
  return RTP_OK;
}

int rtp_overlay_update(rtp_trail_state* st, const rtp_overlay_config* cfg, const float* joints, int num_people, const int* recs, int* items, int* num_items,
                       int capacity) {
  if (!items || !num_items || capacity < 0 || rtp_internal_overlay_check(cfg) || rtp_internal_trail_check(st)) return RTP_EINVAL;
  if (st->num_parts < 1 || st->num_parts > RTP_MAX_NUM_PARTS) return RTP_EINVAL;
  const int n = num_people < 0 ? 0 : num_people > RTP_MAX_PEOPLE ? RTP_MAX_PEOPLE : num_people;
  if (n > 0 && (!joints || !recs)) return RTP_EINVAL;
  const int P = st->num_parts, L = cfg->trail_len;
  bool taken[RTP_MAX_TRACKS] = {};
  int box[RTP_MAX_PEOPLE][4];
  bool draws[RTP_MAX_PEOPLE];
  int total = 0;
  // the frame's count first: a refused call leaves the state untouched
  for (int k = 0; k < n; ++k) {
    const int id = recs[(size_t)k * RTP_TRACK_REC_INTS], t = recs[(size_t)k * RTP_TRACK_REC_INTS + 1];
    draws[k] = false;
    if (id == 0) continue;
    if (t < 0 || t >= RTP_MAX_TRACKS || taken[t]) return RTP_EINVAL;
    taken[t] = true;
    draws[k] = overlay_box(joints + (size_t)k * P * 3, P, cfg->min_score, cfg->box_margin, box[k]);
    if (!draws[k]) continue;
    const int count = std::min((st->slot[t].owner == id ? st->slot[t].count : 0) + 1, L);
    total += ((cfg->what & RTP_OVERLAY_TRAIL) ? std::max(count - 1, 0) : 0) + ((cfg->what & RTP_OVERLAY_BOX) ? 1 : 0) + ((cfg->what & RTP_OVERLAY_LABEL) ? 1 : 0);
  }
  *num_items = total;
  if (total > capacity) return RTP_ERANGE;
  st->frames++;
  if (st->frames == 0) st->frames = 1;
  int* it = items;
  for (int k = 0; k < n; ++k) {
    if (!draws[k]) continue;
    const int id = recs[(size_t)k * RTP_TRACK_REC_INTS];
    rtp_trail_slot& S = st->slot[recs[(size_t)k * RTP_TRACK_REC_INTS + 1]];
    const int* b = box[k];
    if (S.owner != id) { S.owner = id; S.count = 0; S.head = 0; }
    S.pts[S.head][0] = (b[0] + b[2]) >> 1;
    S.pts[S.head][1] = (b[1] + b[3]) >> 1;
    S.head = (S.head + 1) % RTP_TRAIL_MAX;
    S.count = std::min(S.count + 1, L);
    const int colour = kOverlayPalette[id & 15];
    if (cfg->what & RTP_OVERLAY_TRAIL) {
      const int m = std::max(S.count - 1, 0);
      for (int j = 0; j < m; ++j, it += RTP_OVERLAY_ITEM_INTS) {
        const int* a = S.pts[(S.head - S.count + j + RTP_TRAIL_MAX) % RTP_TRAIL_MAX];
        const int* c = S.pts[(S.head - S.count + j + 1 + RTP_TRAIL_MAX) % RTP_TRAIL_MAX];
        const int item[RTP_OVERLAY_ITEM_INTS] = {RTP_OVERLAY_KIND_CAPSULE, a[0], a[1], c[0], c[1], cfg->trail_radius, colour, cfg->alpha * (j + 1) / m, 0};
        memcpy(it, item, sizeof item);
      }
    }
    if (cfg->what & RTP_OVERLAY_BOX) {
      const int item[RTP_OVERLAY_ITEM_INTS] = {RTP_OVERLAY_KIND_RECT, b[0], b[1], b[2], b[3], cfg->line_width, colour, cfg->alpha, 0};
      memcpy(it, item, sizeof item);
      it += RTP_OVERLAY_ITEM_INTS;
    }
    if (cfg->what & RTP_OVERLAY_LABEL) {
      const int lw = (6 * overlay_digits((unsigned)id) + 1) * cfg->label_scale, lh = 9 * cfg->label_scale;
      const int ly = b[1] - lh < 0 ? b[1] : b[1] - lh;
      const int item[RTP_OVERLAY_ITEM_INTS] = {RTP_OVERLAY_KIND_LABEL, b[0], ly, b[0] + lw - 1, ly + lh - 1, cfg->label_scale, colour, cfg->alpha, id};
      memcpy(it, item, sizeof item);
      it += RTP_OVERLAY_ITEM_INTS;
    }
  }
  return RTP_OK;
}

int rtp_overlay_draw(const int* items, int num_items, unsigned char* image_bgr, int w, int h, long stride) {
  if (!image_bgr || num_items < 0 || (num_items > 0 && !items) || w < 1 || h < 1 || stride < 3L * w) return RTP_EINVAL;
  for (int i = 0; i < num_items; ++i) {
    int it[RTP_OVERLAY_ITEM_INTS];
    memcpy(it, items + (size_t)i * RTP_OVERLAY_ITEM_INTS, sizeof it);
    const int kind = it[0];
    if (kind != RTP_OVERLAY_KIND_CAPSULE && kind != RTP_OVERLAY_KIND_RECT && kind != RTP_OVERLAY_KIND_LABEL) continue;
    for (int q = 1; q <= 4; ++q) it[q] = clampi(it[q], -65535, 65535);
    it[5] = kind == RTP_OVERLAY_KIND_LABEL ? clampi(it[5], 1, 8) : clampi(it[5], 0, 16);
    const int a = clampi(it[7], 0, 256);
    // the item's bounding box, clipped to the image
    const int grow = kind == RTP_OVERLAY_KIND_CAPSULE ? it[5] : 0;
    const int bx0 = std::max(std::min(it[1], it[3]) - grow, 0), bx1 = std::min(std::max(it[1], it[3]) + grow, w - 1);
    const int by0 = std::max(std::min(it[2], it[4]) - grow, 0), by1 = std::min(std::max(it[2], it[4]) + grow, h - 1);
    int digit[10] = {}, ndig = 0;
    if (kind == RTP_OVERLAY_KIND_LABEL) {
      unsigned v = (unsigned)it[8];
      ndig = overlay_digits(v);
      for (int d = ndig - 1; d >= 0; --d, v /= 10u) digit[d] = (int)(v % 10u);
    }
    const int cb = it[6] & 255, cg = (it[6] >> 8) & 255, cr = (it[6] >> 16) & 255;
    const int text = ((29 * cb + 150 * cg + 77 * cr) >> 8) >= 128 ? 0 : 255;
    for (int py = by0; py <= by1; ++py)
      for (int px = bx0; px <= bx1; ++px) {
        const int c = overlay_covers(it, digit, ndig, px, py);
        if (!c) continue;
        unsigned char* p = image_bgr + (size_t)py * stride + (size_t)px * 3;
        const int col[3] = {c == 2 ? text : cb, c == 2 ? text : cg, c == 2 ? text : cr};
        for (int ch = 0; ch < 3; ++ch) p[ch] = (unsigned char)((p[ch] * (256 - a) + col[ch] * a + 128) >> 8);
      }
  }
  return RTP_OK;
}

}  // extern "C"

// ---- redaction mode: the one definition of its regions and its pixels (redact.hip computes the same integers and bytes on the device)

// What is wrong with the configuration for a model of model_parts parts, or nullptr.  The engine's switch reports the same text.
extern "C" const char* rtp_internal_redact_check(const rtp_redact_config* c, int model_parts) {
  if (!c) return "NULL rtp_redact_config";
  if (c->struct_size != sizeof(rtp_redact_config)) return "rtp_redact_config.struct_size is not this library's sizeof(rtp_redact_config)";
  if (model_parts < 1 || model_parts > RTP_MAX_NUM_PARTS) return "num_parts outside 1 .. RTP_MAX_NUM_PARTS";
  if (c->effect != RTP_REDACT_MOSAIC && c->effect != RTP_REDACT_BLUR && c->effect != RTP_REDACT_FILL) return "effect is none of RTP_REDACT_MOSAIC, RTP_REDACT_BLUR and RTP_REDACT_FILL";
  if (c->shape != RTP_REDACT_ELLIPSE && c->shape != RTP_REDACT_RECT) return "shape is neither RTP_REDACT_ELLIPSE nor RTP_REDACT_RECT";
  if (!(c->min_score >= 0.f) || std::isinf(c->min_score)) return "min_score must be a finite number >= 0";
  if (c->min_parts < 1) return "min_parts must be >= 1";
  if (c->scale_q8 < 64 || c->scale_q8 > 4096) return "scale_q8 must be 64 .. 4096";
  if (c->aspect_q8 < 64 || c->aspect_q8 > 1024) return "aspect_q8 must be 64 .. 1024";
  if (c->pad < 0 || c->pad > 256) return "pad must be 0 .. 256";
  if (c->min_radius < 0 || c->min_radius > 256) return "min_radius must be 0 .. 256";
  if (c->cell != 2 && c->cell != 4 && c->cell != 8 && c->cell != 16 && c->cell != 32) return "cell must be 2, 4, 8, 16 or 32";
  if (c->radius < 1 || c->radius > 16) return "radius must be 1 .. 16";
  if (c->parts) {
    if (c->num_parts < 1 || c->num_parts > RTP_MAX_NUM_PARTS) return "the part list's num_parts outside 1 .. RTP_MAX_NUM_PARTS";
    bool seen[RTP_MAX_NUM_PARTS] = {};
    for (int i = 0; i < c->num_parts; ++i) {
      if (c->parts[i] < 0 || c->parts[i] >= model_parts) return "a listed part is outside the model's parts";
      if (seen[c->parts[i]]) return "a part is listed twice";
      seen[c->parts[i]] = true;
    }
  }
  return nullptr;
}

// The list the configuration names for a model of model_parts parts (checked): its own, or the model's head parts; 0 = NULL parts and
// neither 18 nor 15 parts
extern "C" int rtp_internal_redact_list(const rtp_redact_config* c, int model_parts, int list[RTP_MAX_NUM_PARTS]) {
  if (c->parts) {
    memcpy(list, c->parts, (size_t)c->num_parts * sizeof(int));
    return c->num_parts;
  }
  int head[8];
  const int n = model_parts == 18 ? rtp_crops_head_parts(RTP_MODEL_COCO_18, head) : model_parts == 15 ? rtp_crops_head_parts(RTP_MODEL_MPI_15, head) : 0;
  if (n > 0) memcpy(list, head, (size_t)n * sizeof(int));
  return n > 0 ? n : 0;
}

extern "C" {

int rtp_redact_config_default(rtp_redact_config* cfg) {
  if (!cfg) return RTP_EINVAL;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = (unsigned)sizeof *cfg;
  cfg->effect = RTP_REDACT_MOSAIC;
  cfg->shape = RTP_REDACT_ELLIPSE;
  cfg->parts = nullptr;
  cfg->num_parts = 0;
  cfg->min_score = 0.f;
  cfg->min_parts = 1;
  cfg->scale_q8 = 384;
  cfg->aspect_q8 = 320;
  cfg->pad = 2;
  cfg->min_radius = 4;
  cfg->cell = 8;
  cfg->radius = 8;
  cfg->colour = 0;
  return RTP_OK;
}

int rtp_redact_regions(const float* joints, int num_people, int num_parts, const rtp_redact_config* cfg, int* regions) {
  if (rtp_internal_redact_check(cfg, num_parts) || !regions) return RTP_EINVAL;
  int list[RTP_MAX_NUM_PARTS];
  const int nlist = rtp_internal_redact_list(cfg, num_parts, list);
  if (nlist < 1) return RTP_EINVAL;
  const int n = num_people < 0 ? 0 : num_people > RTP_MAX_PEOPLE ? RTP_MAX_PEOPLE : num_people;
  if (n > 0 && !joints) return RTP_EINVAL;
  for (int k = 0; k < n; ++k) {
    const float* j = joints + (size_t)k * num_parts * 3;
    int* rec = regions + (size_t)k * RTP_REDACT_REGION_INTS;
    float fx0 = 0.f, fx1 = 0.f, fy0 = 0.f, fy1 = 0.f;
    int c = 0;
    for (int i = 0; i < nlist; ++i) {
      const float x = j[3 * list[i]], y = j[3 * list[i] + 1], s = j[3 * list[i] + 2];
      if (!(s > cfg->min_score) || !std::isfinite(x) || !std::isfinite(y)) continue;
      if (c++ == 0) { fx0 = fx1 = x; fy0 = fy1 = y; continue; }
      if (x < fx0) fx0 = x;
      if (x > fx1) fx1 = x;
      if (y < fy0) fy0 = y;
      if (y > fy1) fy1 = y;
    }
    if (c < cfg->min_parts) {
      const int none[RTP_REDACT_REGION_INTS] = {0, 0, 0, 0, c, 0};
      memcpy(rec, none, sizeof none);
      continue;
    }
    const int x0 = overlay_round(fx0), x1 = overlay_round(fx1), y0 = overlay_round(fy0), y1 = overlay_round(fy1);
    const int s = std::max(x1 - x0, y1 - y0) + 1;   // 1 .. 65535: s * scale_q8 < 2^28
    const int rx = clampi(((s * cfg->scale_q8) >> 9) + cfg->pad, cfg->min_radius, RTP_REDACT_MAX_RADIUS);
    const int ry = std::min((rx * cfg->aspect_q8) >> 8, RTP_REDACT_MAX_RADIUS);
    const int rec_k[RTP_REDACT_REGION_INTS] = {(x0 + x1) >> 1, (y0 + y1) >> 1, rx, ry, c, 1};   // (>> of a negative sum: floor)
    memcpy(rec, rec_k, sizeof rec_k);
  }
  return n;
}

int rtp_redact_apply(const int* regions, int num_regions, const rtp_redact_config* cfg, unsigned char* image_bgr, int w, int h, long stride) {
  if (rtp_internal_redact_check(cfg, RTP_MAX_NUM_PARTS) || !image_bgr || num_regions < 0 || num_regions > RTP_MAX_PEOPLE || (num_regions > 0 && !regions) || w < 1 || h < 1 ||
      w > 32768 || h > 32768 || stride < 3L * w)
    return RTP_EINVAL;
  // the valid regions, clamped, and the box [bx0, bx1] x [by0, by1] of the image that holds every covered pixel
  struct Reg { int cx, cy, rx, ry; };
  std::vector<Reg> regs;
  int bx0 = w, bx1 = -1, by0 = h, by1 = -1;
  for (int i = 0; i < num_regions; ++i) {
    const int* r = regions + (size_t)i * RTP_REDACT_REGION_INTS;
    if (!r[5]) continue;
    const Reg g = {clampi(r[0], -65535, 65535), clampi(r[1], -65535, 65535), clampi(r[2], 0, RTP_REDACT_MAX_RADIUS), clampi(r[3], 0, RTP_REDACT_MAX_RADIUS)};
    if (g.cx + g.rx < 0 || g.cx - g.rx >= w || g.cy + g.ry < 0 || g.cy - g.ry >= h) continue;
    regs.push_back(g);
    bx0 = std::min(bx0, std::max(g.cx - g.rx, 0)); bx1 = std::max(bx1, std::min(g.cx + g.rx, w - 1));
    by0 = std::min(by0, std::max(g.cy - g.ry, 0)); by1 = std::max(by1, std::min(g.cy + g.ry, h - 1));
  }
  if (regs.empty()) return RTP_OK;
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
  std::vector<unsigned char> covered((size_t)bw * bh, 0);
  const bool ellipse = cfg->shape == RTP_REDACT_ELLIPSE;
  for (const Reg& g : regs) {
    const long long rx = g.rx, ry = g.ry, lim = rx * ry * rx * ry;
    for (int py = std::max(g.cy - g.ry, 0); py <= std::min(g.cy + g.ry, h - 1); ++py)
      for (int px = std::max(g.cx - g.rx, 0); px <= std::min(g.cx + g.rx, w - 1); ++px) {
        const long long dx = (long long)(px - g.cx) * ry, dy = (long long)(py - g.cy) * rx;
        if (!ellipse || dx * dx + dy * dy <= lim) covered[(size_t)(py - by0) * bw + (px - bx0)] = 1;
      }
  }
  if (cfg->effect == RTP_REDACT_FILL) {
    const unsigned char col[3] = {(unsigned char)(cfg->colour & 255), (unsigned char)((cfg->colour >> 8) & 255), (unsigned char)((cfg->colour >> 16) & 255)};
    for (int py = by0; py <= by1; ++py)
      for (int px = bx0; px <= bx1; ++px)
        if (covered[(size_t)(py - by0) * bw + (px - bx0)]) memcpy(image_bgr + (size_t)py * stride + (size_t)px * 3, col, 3);
    return RTP_OK;
  }
  // The image as it was, as a summed-area table over the box grown by what a covered pixel's value reads (the blur's radius, or out
  // to its cell's borders): S[y][x][c] = the sum over rows < y and columns < x, in uint32 arithmetic modulo 2^32 — a window's
  // sum, at most 33 * 33 * 255 (blur) or 32 * 32 * 255 (mosaic), comes out of the four corners exactly whatever has wrapped.
  const bool mosaic = cfg->effect == RTP_REDACT_MOSAIC;
  const int cell = cfg->cell, rad = cfg->radius;
  const int sx0 = mosaic ? bx0 / cell * cell : std::max(bx0 - rad, 0), sy0 = mosaic ? by0 / cell * cell : std::max(by0 - rad, 0);
  const int sx1 = mosaic ? std::min((bx1 / cell + 1) * cell, w) : std::min(bx1 + rad + 1, w);   // exclusive
  const int sy1 = mosaic ? std::min((by1 / cell + 1) * cell, h) : std::min(by1 + rad + 1, h);
  const int sw = sx1 - sx0, sh = sy1 - sy0;
  std::vector<unsigned> S((size_t)(sw + 1) * (sh + 1) * 3, 0u);
  for (int y = 0; y < sh; ++y) {
    const unsigned char* row = image_bgr + (size_t)(sy0 + y) * stride + (size_t)sx0 * 3;
    unsigned run[3] = {0u, 0u, 0u};
    for (int x = 0; x < sw; ++x)
      for (int c = 0; c < 3; ++c) {
        run[c] += row[3 * x + c];
        S[((size_t)(y + 1) * (sw + 1) + x + 1) * 3 + c] = S[((size_t)y * (sw + 1) + x + 1) * 3 + c] + run[c];
      }
  }
  for (int py = by0; py <= by1; ++py)
    for (int px = bx0; px <= bx1; ++px) {
      if (!covered[(size_t)(py - by0) * bw + (px - bx0)]) continue;
      int x0, x1, y0, y1;   // the window inside the image, x1 and y1 exclusive
      if (mosaic) {
        x0 = px / cell * cell; x1 = std::min(x0 + cell, w); y0 = py / cell * cell; y1 = std::min(y0 + cell, h);
      } else {
        x0 = std::max(px - rad, 0); x1 = std::min(px + rad + 1, w); y0 = std::max(py - rad, 0); y1 = std::min(py + rad + 1, h);
      }
      const unsigned cnt = (unsigned)(x1 - x0) * (unsigned)(y1 - y0);
      unsigned char* p = image_bgr + (size_t)py * stride + (size_t)px * 3;
      for (int c = 0; c < 3; ++c) {
        auto at = [&](int y, int x) { return S[((size_t)(y - sy0) * (sw + 1) + (x - sx0)) * 3 + c]; };
        const unsigned sum = at(y1, x1) - at(y0, x1) - at(y1, x0) + at(y0, x0);
        p[c] = (unsigned char)((sum + (cnt >> 1)) / cnt);
      }
    }
  return RTP_OK;
}

}  // extern "C"

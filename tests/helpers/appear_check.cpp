// Stand-alone replay of tests/_appearcases.py through rtp_appearance_describe and rtp_track_update_appearance for
// tests/test_appearance_cpu.py, built with g++ -fsanitize=address,undefined together with the host-only sources of the library.  Image,
// joints, descriptors, valid bytes and records of every call are heap blocks of exactly the bytes the call may touch, so a load or
// store one element past them is an AddressSanitizer report.
// Input (argv[1], written by the test): int32 cases; per case: int32 P, the appearance configuration (int32 nlist (-1 = NULL), nlist
// int32, float min_score, int32 min_parts, float margin, float weight, float max_dist, float unknown, int32 rate), the tracking
// configuration (float min_score, int32 min_parts, int32 min_common, float max_cost, int32 max_misses), int32 frames; per frame:
// int32 num_people (as given to the update), int32 rows, rows * P * 3 floats, int32 w, int32 h (0 0 = no image), w * h * 3 bytes,
// int32 nd (descriptors expected of the describe call, when there is an image), nd * 128 uint16, nd bytes, int32 n, n * 4 int32
// expected records (n = -1: the frame of a describe case, no update is run).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rtpose_mi355x.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int cases = 0, frames_total = 0;
  if (!rd(f, &cases, 4)) return 2;
  rtp_track_state* st = (rtp_track_state*)malloc(sizeof(rtp_track_state));
  rtp_track_state* st_before = (rtp_track_state*)malloc(sizeof(rtp_track_state));
  rtp_appearance_state* ap = (rtp_appearance_state*)malloc(sizeof(rtp_appearance_state));
  rtp_appearance_state* ap_before = (rtp_appearance_state*)malloc(sizeof(rtp_appearance_state));
  for (int c = 0; c < cases; ++c) {
    rtp_appearance_config acfg;
    rtp_track_config tcfg;
    rtp_appearance_config_default(&acfg);
    rtp_track_config_default(&tcfg);
    int P = 0, frames = 0, nlist = 0;
    if (!rd(f, &P, 4) || !rd(f, &nlist, 4)) return 2;
    int* list = nlist > 0 ? (int*)malloc((size_t)nlist * sizeof(int)) : nullptr;
    if (nlist > 0 && !rd(f, list, (size_t)nlist * sizeof(int))) return 2;
    acfg.parts = list;
    acfg.num_parts = nlist > 0 ? nlist : 0;
    if (!rd(f, &acfg.min_score, 4) || !rd(f, &acfg.min_parts, 4) || !rd(f, &acfg.margin, 4) || !rd(f, &acfg.weight, 4) || !rd(f, &acfg.max_dist, 4) ||
        !rd(f, &acfg.unknown, 4) || !rd(f, &acfg.rate, 4) || !rd(f, &tcfg.min_score, 4) || !rd(f, &tcfg.min_parts, 4) || !rd(f, &tcfg.min_common, 4) ||
        !rd(f, &tcfg.max_cost, 4) || !rd(f, &tcfg.max_misses, 4) || !rd(f, &frames, 4))
      return 2;
    if (rtp_track_state_init(st, P) != RTP_OK || rtp_appearance_state_init(ap) != RTP_OK) { printf("case %d: state_init refused\n", c); return 1; }
    for (int i = 0; i < frames; ++i, ++frames_total) {
      int num_people = 0, rows = 0, w = 0, h = 0, nd = 0, n = 0;
      if (!rd(f, &num_people, 4) || !rd(f, &rows, 4)) return 2;
      float* joints = rows ? (float*)malloc((size_t)rows * P * 3 * sizeof(float)) : nullptr;
      if (!rd(f, joints, (size_t)rows * P * 3 * sizeof(float)) || !rd(f, &w, 4) || !rd(f, &h, 4)) return 2;
      unsigned char* image = w ? (unsigned char*)malloc((size_t)w * h * 3) : nullptr;
      if (!rd(f, image, (size_t)w * h * 3) || !rd(f, &nd, 4)) return 2;
      std::vector<uint16_t> want_bins((size_t)nd * RTP_APPEARANCE_BINS);
      std::vector<unsigned char> want_valid((size_t)nd);
      if (!rd(f, want_bins.data(), want_bins.size() * 2) || !rd(f, want_valid.data(), want_valid.size()) || !rd(f, &n, 4)) return 2;
      std::vector<int> want(n > 0 ? (size_t)n * 4 : 0);
      if (!rd(f, want.data(), want.size() * sizeof(int))) return 2;
      uint16_t* bins = nullptr;
      unsigned char* valid = nullptr;
      if (image) {
        bins = (uint16_t*)malloc(nd ? (size_t)nd * RTP_APPEARANCE_BINS * 2 : 1);
        valid = (unsigned char*)malloc(nd ? (size_t)nd : 1);
        const int got = rtp_appearance_describe(image, w, h, joints, rows, P, &acfg, bins, valid);
        if (got != nd || (nd && (memcmp(bins, want_bins.data(), want_bins.size() * 2) != 0 || memcmp(valid, want_valid.data(), (size_t)nd) != 0))) {
          printf("case %d frame %d: %d descriptors (expected %d), or their values differ\n", c, i, got, nd);
          return 1;
        }
        // refusals: nothing is written (the blocks hold what the good call left)
        rtp_appearance_config bad = acfg;
        bad.rate = 0;
        int far_part = P;
        rtp_appearance_config bad_list = acfg;
        bad_list.parts = &far_part;
        bad_list.num_parts = 1;
        if (rtp_appearance_describe(image, w, h, joints, rows, P, &bad, bins, valid) != RTP_EINVAL || rtp_appearance_describe(image, 0, h, joints, rows, P, &acfg, bins, valid) != RTP_EINVAL ||
            rtp_appearance_describe(image, w, h, joints, rows, P, &bad_list, bins, valid) != RTP_EINVAL || rtp_appearance_describe(image, w, h, joints, -1, P, &acfg, bins, valid) != RTP_EINVAL ||
            rtp_appearance_describe(image, w, h, joints, rows, P, &acfg, nullptr, valid) != RTP_EINVAL || rtp_appearance_describe(image, w, h, joints, rows, P, &acfg, bins, nullptr) != RTP_EINVAL ||
            (rows && rtp_appearance_describe(nullptr, w, h, joints, rows, P, &acfg, bins, valid) != RTP_EINVAL) ||
            (nd && (memcmp(bins, want_bins.data(), want_bins.size() * 2) != 0 || memcmp(valid, want_valid.data(), (size_t)nd) != 0))) {
          printf("case %d frame %d: a refused describe call\n", c, i);
          return 1;
        }
      }
      if (n >= 0) {
        int* recs = (int*)malloc(n ? (size_t)n * 4 * sizeof(int) : 1);
        // a refused call leaves both states untouched
        memcpy(st_before, st, sizeof *st);
        memcpy(ap_before, ap, sizeof *ap);
        rtp_appearance_config bad = acfg;
        bad.max_dist = 0.f;
        rtp_track_config tbad = tcfg;
        tbad.max_cost = 0.f;
        if (rtp_track_update_appearance(st, ap, &tcfg, &bad, joints, num_people, bins, valid, recs) != RTP_EINVAL ||
            rtp_track_update_appearance(st, ap, &tbad, &acfg, joints, num_people, bins, valid, recs) != RTP_EINVAL ||
            rtp_track_update_appearance(st, ap, &tcfg, &acfg, joints, num_people, bins, valid, nullptr) != RTP_EINVAL ||
            rtp_track_update_appearance(st, nullptr, &tcfg, &acfg, joints, num_people, bins, valid, recs) != RTP_EINVAL ||
            rtp_track_update_appearance(nullptr, ap, &tcfg, &acfg, joints, num_people, bins, valid, recs) != RTP_EINVAL ||
            (bins && rtp_track_update_appearance(st, ap, &tcfg, &acfg, joints, num_people, bins, nullptr, recs) != RTP_EINVAL) ||
            memcmp(st_before, st, sizeof *st) != 0 || memcmp(ap_before, ap, sizeof *ap) != 0) {
          printf("case %d frame %d: a refused update call\n", c, i);
          return 1;
        }
        const int got = rtp_track_update_appearance(st, ap, &tcfg, &acfg, joints, num_people, bins, valid, recs);
        if (got != n || (n && memcmp(recs, want.data(), want.size() * sizeof(int)) != 0)) { printf("case %d frame %d: %d records (expected %d), or their values differ\n", c, i, got, n); return 1; }
        free(recs);
      }
      free(bins);
      free(valid);
      free(image);
      free(joints);
    }
    free(list);
  }
  fclose(f);
  free(st); free(st_before); free(ap); free(ap_before);
  printf("appear_check OK: %d cases, %d frames\n", cases, frames_total);
  return 0;
}

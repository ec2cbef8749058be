// Stand-alone replay of tests/_trackcases.py through rtp_track_update for tests/test_track_cpu.py, built with
// g++ -fsanitize=address,undefined together with the host-only sources of the library.  The joints and the records of every frame are
// heap blocks of exactly the bytes the call may touch, so a load or store one element past them is an AddressSanitizer report.
// Input (argv[1], written by the test): int32 cases; per case: int32 P, float min_score, int32 min_parts, int32 min_common,
// float max_cost, int32 max_misses, int32 frames; per frame: int32 num_people (as given to the call), int32 rows, rows * P * 3 floats,
// int32 n, n * 4 int32 expected records.
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
  rtp_track_state* before = (rtp_track_state*)malloc(sizeof(rtp_track_state));
  for (int c = 0; c < cases; ++c) {
    rtp_track_config cfg;
    rtp_track_config_default(&cfg);
    int P = 0, frames = 0;
    if (!rd(f, &P, 4) || !rd(f, &cfg.min_score, 4) || !rd(f, &cfg.min_parts, 4) || !rd(f, &cfg.min_common, 4) || !rd(f, &cfg.max_cost, 4) || !rd(f, &cfg.max_misses, 4) ||
        !rd(f, &frames, 4))
      return 2;
    if (rtp_track_state_init(st, P) != RTP_OK) { printf("case %d: state_init(%d) refused\n", c, P); return 1; }
    for (int i = 0; i < frames; ++i, ++frames_total) {
      int num_people = 0, rows = 0, n = 0;
      if (!rd(f, &num_people, 4) || !rd(f, &rows, 4)) return 2;
      float* joints = rows ? (float*)malloc((size_t)rows * P * 3 * sizeof(float)) : nullptr;
      if (!rd(f, joints, (size_t)rows * P * 3 * sizeof(float)) || !rd(f, &n, 4)) return 2;
      std::vector<int> want((size_t)n * 4);
      if (!rd(f, want.data(), want.size() * sizeof(int))) return 2;
      int* recs = (int*)malloc(n ? (size_t)n * 4 * sizeof(int) : 1);
      const int got = rtp_track_update(st, &cfg, joints, num_people, recs);
      if (got != n || (n && memcmp(recs, want.data(), want.size() * sizeof(int)) != 0)) { printf("case %d frame %d: %d records (expected %d), or their values differ\n", c, i, got, n); return 1; }
      // a refused call leaves the state untouched
      memcpy(before, st, sizeof *st);
      rtp_track_config bad = cfg;
      bad.max_cost = 0.f;
      if (rtp_track_update(st, &bad, joints, num_people, recs) != RTP_EINVAL || rtp_track_update(st, &cfg, joints, num_people, nullptr) != RTP_EINVAL ||
          memcmp(before, st, sizeof *st) != 0) { printf("case %d frame %d: a refused call\n", c, i); return 1; }
      free(recs);
      free(joints);
    }
  }
  fclose(f);
  free(st);
  free(before);
  printf("track_check OK: %d cases, %d frames\n", cases, frames_total);
  return 0;
}

// Stand-alone check of rtp_convert_yuv for tests/test_yuv_frames_cpu.py, built with g++ -fsanitize=address,undefined together with the
// host-only sources of the library.  Every plane is a heap block of exactly the bytes its view describes, so a load one element past
// a plane (the odd widths and heights are the cases that invite one) is an AddressSanitizer report; the output is compared with the
// formula written out once more.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rtpose_mi355x.h"

namespace {

int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

unsigned g_state = 12345u;
unsigned char next_byte() { g_state = g_state * 1664525u + 1013904223u; return (unsigned char)(g_state >> 24); }

// mode 0 = planar, 1 = NV12, 2 = NV21; sx = sy = -1: luma only
int check(int w, int h, int sx, int sy, int mode, long ypad, long cpad) {
  const bool mono = sx < 0;
  const int cw = mono ? 0 : (w + sx) >> sx, ch = mono ? 0 : (h + sy) >> sy;
  const long ys = w + ypad, ps = mode ? 2 : 1, cs = cw * ps + cpad;
  // exactly the bytes the view addresses: the last row has no padding
  unsigned char* Y = (unsigned char*)malloc((size_t)((h - 1) * ys + w));
  for (long i = 0; i < (h - 1) * ys + w; ++i) Y[i] = next_byte();
  unsigned char *U = nullptr, *V = nullptr, *UV = nullptr;
  if (!mono) {
    if (mode == 0) {
      const size_t n = (size_t)((ch - 1) * cs + cw);
      U = (unsigned char*)malloc(n);
      V = (unsigned char*)malloc(n);
      for (size_t i = 0; i < n; ++i) { U[i] = next_byte(); V[i] = next_byte(); }
    } else {
      const size_t n = (size_t)((ch - 1) * cs + 2 * cw);
      UV = (unsigned char*)malloc(n);
      for (size_t i = 0; i < n; ++i) UV[i] = next_byte();
      U = mode == 1 ? UV : UV + 1;
      V = mode == 1 ? UV + 1 : UV;
    }
  }
  rtp_yuv_view v;
  memset(&v, 0, sizeof v);
  v.struct_size = sizeof v;
  v.matrix = RTP_YUV_BT601_LIMITED;
  v.y = Y; v.u = U; v.v = V;
  v.width = w; v.height = h;
  v.chroma_shift_x = mono ? 0 : sx; v.chroma_shift_y = mono ? 0 : sy;
  v.y_stride = ys; v.uv_stride = mono ? 0 : cs; v.uv_pixel_stride = ps;
  unsigned char* out = (unsigned char*)malloc((size_t)w * h * 3);
  int bad = 0;
  const int rc = rtp_convert_yuv(&v, out, (size_t)w * h * 3);
  if (rc != RTP_OK) { printf("rtp_convert_yuv(%d x %d, shifts %d %d, mode %d) = %d: %s\n", w, h, sx, sy, mode, rc, rtp_codec_last_error()); bad = 1; }
  for (int y = 0; y < h && !bad; ++y)
    for (int x = 0; x < w; ++x) {
      const int c = 298 * (Y[y * ys + x] - 16);
      const int d = mono ? 0 : U[(y >> sy) * cs + (x >> sx) * ps] - 128, e = mono ? 0 : V[(y >> sy) * cs + (x >> sx) * ps] - 128;
      const int want[3] = {clamp255((c + 516 * d + 128) >> 8), clamp255((c - 100 * d - 208 * e + 128) >> 8), clamp255((c + 409 * e + 128) >> 8)};
      const unsigned char* o = out + ((size_t)y * w + x) * 3;
      if (o[0] != want[0] || o[1] != want[1] || o[2] != want[2]) {
        printf("%d x %d shifts %d %d mode %d: pixel (%d, %d) is %d %d %d, want %d %d %d\n", w, h, sx, sy, mode, x, y, o[0], o[1], o[2], want[0], want[1], want[2]);
        bad = 1;
        break;
      }
    }
  free(out);
  free(Y);
  if (mode == 0) { free(U); free(V); } else free(UV);
  return bad;
}

}  // namespace

int main() {
  const int sizes[][2] = {{1, 1}, {2, 2}, {3, 3}, {5, 4}, {16, 8}, {67, 45}};
  const int shifts[][2] = {{1, 1}, {1, 0}, {0, 0}, {-1, -1}};
  int bad = 0, n = 0;
  for (const auto& s : sizes)
    for (const auto& sh : shifts)
      for (int mode = 0; mode < (sh[0] < 0 ? 1 : 3); ++mode)
        for (int pad = 0; pad < 2; ++pad) {
          bad |= check(s[0], s[1], sh[0], sh[1], mode, pad ? 5 : 0, pad ? 3 : 0);
          ++n;
        }
  if (bad) return 1;
  printf("yuv_check OK: %d views\n", n);
  return 0;
}

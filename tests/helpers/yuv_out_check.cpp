// Stand-alone check of rtp_convert_bgr_to_yuv and the stream writers for tests/test_yuv_out_cpu.py, built with g++
// -fsanitize=address,undefined together with the host-only sources of the library.  The source image and every plane are heap blocks of
// exactly the bytes their views describe, so a load past the image's last pixel or a store past a plane's last sample (the odd widths and
// heights are the cases that invite one) is an AddressSanitizer report; the output is compared with the formula written out once more.
// argv[1]: a directory for the two streams the writers produce (read back through rtp_video_open).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtpose_mi355x.h"

namespace {

unsigned g_state = 2463534242u;
unsigned char next_byte() { g_state = g_state * 1664525u + 1013904223u; return (unsigned char)(g_state >> 24); }

struct Planes {
  unsigned char *Y = nullptr, *U = nullptr, *V = nullptr, *UV = nullptr;
  rtp_yuv_view v;
  int mode = 0;
  void release() { free(Y); if (mode == 0) { free(U); free(V); } else free(UV); }
};

// mode 0 = planar, 1 = NV12, 2 = NV21; sx = sy = -1: luma only.  Exactly the bytes the view addresses: the last row has no padding.
Planes make_planes(int w, int h, int sx, int sy, int mode, long ypad, long cpad) {
  Planes p;
  p.mode = mode;
  const bool mono = sx < 0;
  const int cw = mono ? 0 : (w + sx) >> sx, ch = mono ? 0 : (h + sy) >> sy;
  const long ys = w + ypad, ps = mode ? 2 : 1, cs = cw * ps + cpad;
  p.Y = (unsigned char*)malloc((size_t)((h - 1) * ys + w));
  if (!mono) {
    if (mode == 0) {
      const size_t n = (size_t)((ch - 1) * cs + cw);
      p.U = (unsigned char*)malloc(n);
      p.V = (unsigned char*)malloc(n);
    } else {
      p.UV = (unsigned char*)malloc((size_t)((ch - 1) * cs + 2 * cw));
      p.U = mode == 1 ? p.UV : p.UV + 1;
      p.V = mode == 1 ? p.UV + 1 : p.UV;
    }
  }
  memset(&p.v, 0, sizeof p.v);
  p.v.struct_size = sizeof p.v;
  p.v.matrix = RTP_YUV_BT601_LIMITED;
  p.v.y = p.Y; p.v.u = p.U; p.v.v = p.V;
  p.v.width = w; p.v.height = h;
  p.v.chroma_shift_x = mono ? 0 : sx; p.v.chroma_shift_y = mono ? 0 : sy;
  p.v.y_stride = ys; p.v.uv_stride = mono ? 0 : cs; p.v.uv_pixel_stride = ps;
  return p;
}

int check(int w, int h, int sx, int sy, int mode, long ypad, long cpad, long spad) {
  const bool mono = sx < 0;
  const long row = 3L * w + spad;
  const size_t nsrc = (size_t)((h - 1) * row + 3L * w);
  unsigned char* src = (unsigned char*)malloc(nsrc);
  for (size_t i = 0; i < nsrc; ++i) src[i] = next_byte();
  Planes p = make_planes(w, h, sx, sy, mode, ypad, cpad);
  int bad = 0;
  const int rc = rtp_convert_bgr_to_yuv(src, w, h, row, &p.v);
  if (rc != RTP_OK) { printf("rtp_convert_bgr_to_yuv(%d x %d, shifts %d %d, mode %d) = %d: %s\n", w, h, sx, sy, mode, rc, rtp_codec_last_error()); bad = 1; }
  for (int y = 0; y < h && !bad; ++y)
    for (int x = 0; x < w; ++x) {
      const unsigned char* q = src + y * row + 3 * x;
      const int want = ((66 * q[2] + 129 * q[1] + 25 * q[0] + 128) >> 8) + 16;
      if (p.Y[y * p.v.y_stride + x] != want) { printf("%d x %d: luma (%d, %d) is %d, want %d\n", w, h, x, y, p.Y[y * p.v.y_stride + x], want); bad = 1; break; }
    }
  if (!mono && !bad) {
    const int cw = (w + sx) >> sx, ch = (h + sy) >> sy, n = (1 << sx) * (1 << sy);
    for (int cy = 0; cy < ch && !bad; ++cy)
      for (int cx = 0; cx < cw; ++cx) {
        int s[3] = {0, 0, 0};
        for (int dy = 0; dy < (1 << sy); ++dy)
          for (int dx = 0; dx < (1 << sx); ++dx) {
            int yy = (cy << sy) + dy, xx = (cx << sx) + dx;
            if (yy > h - 1) yy = h - 1;
            if (xx > w - 1) xx = w - 1;
            for (int c = 0; c < 3; ++c) s[c] += src[yy * row + 3 * xx + c];
          }
        int m[3];
        for (int c = 0; c < 3; ++c) m[c] = n == 4 ? (s[c] + 2) >> 2 : (n == 2 ? (s[c] + 1) >> 1 : s[c]);
        const int wu = ((-38 * m[2] - 74 * m[1] + 112 * m[0] + 128) >> 8) + 128, wv = ((112 * m[2] - 94 * m[1] - 18 * m[0] + 128) >> 8) + 128;
        const long at = cy * p.v.uv_stride + cx * p.v.uv_pixel_stride;
        if (p.U[at] != wu || p.V[at] != wv) {
          printf("%d x %d shifts %d %d mode %d: chroma (%d, %d) is %d %d, want %d %d\n", w, h, sx, sy, mode, cx, cy, p.U[at], p.V[at], wu, wv);
          bad = 1;
          break;
        }
      }
  }
  p.release();
  free(src);
  return bad;
}

// three 4:2:0 frames of an odd chroma width through the Y4M writer (from pitched NV12 planes) and back through the project's reader;
// three JPEG files through the MJPEG writer and back
int check_writers(const std::string& dir) {
  const int w = 18, h = 10, cw = 9, ch = 5;
  const std::string y4m = dir + "/out.y4m", mj = dir + "/out.mjpeg";
  rtp_video_out* o = nullptr;
  if (rtp_video_create(y4m.c_str(), w, h, RTP_VIDEO_Y4M, 25, 1, &o) != RTP_OK) { printf("create: %s\n", rtp_codec_last_error()); return 1; }
  std::vector<std::vector<unsigned char>> want;
  unsigned char jpeg1[4] = {0xFF, 0xD8, 0xFF, 0xD9};
  if (rtp_video_write_jpeg(o, jpeg1, 4) != RTP_EINVAL) { printf("a JPEG file was accepted by the Y4M writer\n"); return 1; }
  for (int f = 0; f < 3; ++f) {
    Planes p = make_planes(w, h, 1, 1, 1, 5, 3);
    std::vector<unsigned char> flat;
    for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) { p.Y[y * p.v.y_stride + x] = next_byte(); }
    for (int y = 0; y < ch; ++y) for (int x = 0; x < cw; ++x) { p.U[y * p.v.uv_stride + 2 * x] = next_byte(); p.V[y * p.v.uv_stride + 2 * x] = next_byte(); }
    for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) flat.push_back(p.Y[y * p.v.y_stride + x]);
    for (int y = 0; y < ch; ++y) for (int x = 0; x < cw; ++x) flat.push_back(p.U[y * p.v.uv_stride + 2 * x]);
    for (int y = 0; y < ch; ++y) for (int x = 0; x < cw; ++x) flat.push_back(p.V[y * p.v.uv_stride + 2 * x]);
    want.push_back(flat);
    const int rc = rtp_video_write_yuv(o, &p.v);
    p.release();
    if (rc != RTP_OK) { printf("write_yuv: %s\n", rtp_codec_last_error()); return 1; }
  }
  if (rtp_video_finish(o) != RTP_OK) { printf("finish: %s\n", rtp_codec_last_error()); return 1; }
  rtp_video* v = nullptr;
  int rw = 0, rh = 0, rn = 0;
  if (rtp_video_open(y4m.c_str(), &v, &rw, &rh, &rn) != RTP_OK || rw != w || rh != h || rn != 3 || rtp_video_chroma(v) != 420) { printf("reading back %s: %d x %d, %d frames\n", y4m.c_str(), rw, rh, rn); return 1; }
  for (int f = 0; f < 3; ++f) {
    rtp_yuv_view yv;
    if (rtp_video_read_yuv(v, &yv) != RTP_OK || memcmp(yv.y, want[f].data(), want[f].size()) != 0) { printf("frame %d of %s differs\n", f, y4m.c_str()); return 1; }
  }
  rtp_video_close(v);

  std::vector<std::vector<unsigned char>> files;
  if (rtp_video_create(mj.c_str(), w, h, RTP_VIDEO_MJPEG, 30, 1, &o) != RTP_OK) { printf("create: %s\n", rtp_codec_last_error()); return 1; }
  for (int f = 0; f < 3; ++f) {
    std::vector<unsigned char> img((size_t)w * h * 3), jpg(rtp_jpeg_max_bytes(w, h));
    for (unsigned char& b : img) b = next_byte();
    const long n = rtp_encode_jpeg(img.data(), w, h, 90, jpg.data(), jpg.size());
    if (n <= 0) { printf("encode: %s\n", rtp_codec_last_error()); return 1; }
    jpg.resize((size_t)n);
    if (rtp_video_write_jpeg(o, jpg.data(), jpg.size()) != RTP_OK) { printf("write_jpeg: %s\n", rtp_codec_last_error()); return 1; }
    files.push_back(jpg);
  }
  if (rtp_video_finish(o) != RTP_OK) { printf("finish: %s\n", rtp_codec_last_error()); return 1; }
  if (rtp_video_open(mj.c_str(), &v, &rw, &rh, &rn) != RTP_OK || rw != w || rh != h) { printf("reading back %s\n", mj.c_str()); return 1; }
  for (int f = 0; f < 3; ++f) {
    const unsigned char* b = nullptr;
    size_t n = 0;
    if (rtp_video_read_jpeg(v, &b, &n) != RTP_OK || n != files[f].size() || memcmp(b, files[f].data(), n) != 0) { printf("file %d of %s differs\n", f, mj.c_str()); return 1; }
  }
  rtp_video_close(v);
  if (rtp_video_create((dir + "/missing/out.y4m").c_str(), w, h, RTP_VIDEO_Y4M, 25, 1, &o) != RTP_EIO) { printf("a path in a missing directory was not refused with RTP_EIO\n"); return 1; }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const int sizes[][2] = {{1, 1}, {2, 2}, {3, 5}, {5, 4}, {17, 9}, {64, 48}};
  const int shifts[][2] = {{1, 1}, {1, 0}, {0, 0}, {-1, -1}};
  int bad = 0, n = 0;
  for (const auto& s : sizes)
    for (const auto& sh : shifts)
      for (int mode = 0; mode < (sh[0] < 0 ? 1 : 3); ++mode)
        for (int pad = 0; pad < 2; ++pad) {
          bad |= check(s[0], s[1], sh[0], sh[1], mode, pad ? 5 : 0, pad ? 3 : 0, pad ? 7 : 0);
          ++n;
        }
  if (bad) return 1;
  if (argc > 1 && check_writers(argv[1])) return 1;
  printf("yuv_out_check OK: %d views\n", n);
  return 0;
}

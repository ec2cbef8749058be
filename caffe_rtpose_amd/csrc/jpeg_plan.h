// jpeg_plan.h — what codecs.cpp's JPEG parser hands to the GPU decoder (engine_jpeg.cpp, jpeg_dec.hip): geometry, quantisers, colour
// model, and either the staged scan with its subsequence tables (entropy decoding on the device) or the coefficients the host's own
// entropy decoder produced (progressive, multi-scan and every irregular file).  Host only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "jpeg_dec.h"

namespace rtp {

struct JpegGeom {
  int W = 0, H = 0, ncomp = 0, hmax = 1, vmax = 1, mcux = 0, mcuy = 0;
  int h[3] = {1, 1, 1}, v[3] = {1, 1, 1}, bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0}, dw[3] = {0, 0, 0}, dh[3] = {0, 0, 0};
  int rgb = 0;                 // three components that already are R, G, B (Adobe transform 0 / component ids "RGB")
  uint16_t qn[3][64];          // per component: the quantiser in NATURAL order
  long blocks() const { long n = 0; for (int c = 0; c < ncomp; ++c) n += (long)bw[c] * bh[c]; return n; }
};

struct JpegPlan {
  int path = 1;                // RTP_JPEG_ENTROPY_DEVICE (0) or RTP_JPEG_ENTROPY_HOST (1)
  JpegGeom g;
  // ---- HOST path: the coefficients, component after component, blocks in raster order, 64 shorts each in natural order
  std::vector<short> coef;
  // ---- DEVICE path
  JdScan scan;
  JdHuff dc[3], ac[3];         // by component
  std::vector<JdSeg> segs;
  std::vector<JdSub> subs;
  size_t nwords = 0;           // staged words (the caller's buffer)
};

// Parses the file and plans its decoding.  sub_bits = S (a multiple of 32).  stage / stage_words: where the scan is staged (the
// planner falls back to the HOST path when it does not fit).  force_host: never plan the DEVICE path.  Returns RTP_OK or the code
// rtp_decode_image returns for the file, with the same message in rtp_codec_last_error().
int jpeg_plan(const unsigned char* bytes, size_t n, int sub_bits, uint32_t* stage, size_t stage_words, bool force_host, JpegPlan* out);

// Host counterpart of the reconstruction kernels: coefficients -> BGR HWC (W x H x 3)
int jpeg_reconstruct_host(const JpegGeom& g, const short* coef, unsigned char* out_bgr, size_t capacity);

// The message codecs.cpp's decoder gives for an entropy failure code (JD_ERR_*)
const char* jpeg_entropy_message(int jd_err);

}  // namespace rtp

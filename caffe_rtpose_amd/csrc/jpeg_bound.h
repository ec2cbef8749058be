// jpeg_bound.h — the worst-case code length of one 8x8 block of a baseline JPEG file with the standard Huffman tables (8-bit samples):
// DC <= 11-bit code + 11 value bits, each of the 63 AC coefficients <= 16-bit code + 10 value bits.  rtp_jpeg_max_bytes (codecs.cpp)
// and the GPU encoder's buffers (jpeg_enc.hip) are both sized from it.
#pragma once

constexpr int kJpegMaxBlockBits = 22 + 63 * 26;

// jpeg_dec.h — what the host (codecs.cpp: planner, serial emulation) and the device (jpeg_dec.hip) share of the GPU JPEG decoder:
// the tables the host uploads, and the ONE per-symbol step of the entropy decoder (Huffman lookup, extend, state update), compiled
// for both, so that the subsequence / round algorithm can be run and tested serially on a CPU.
//
// The entropy-coded segment is staged without stuffing bytes and RSTn markers as big-endian 32-bit words; every restart segment
// starts on a word.  A decoder state at a symbol boundary is (bit position, block within the MCU, zig-zag index: 0 = the DC symbol
// is next).  Bits at or past `limit` (the end of the state's restart segment) read as zero, which is what codecs.cpp's BitReader
// feeds after a marker or the end of the data; no read touches a word past `nwords`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define JD_HD inline
#endif

enum { JD_MAX_MCU_BLOCKS = 10 };
enum { JD_OK = 0, JD_ERR_DC = 1, JD_ERR_AC = 2, JD_ERR_RUN = 3 };   // the three ways decode_block of codecs.cpp fails

// build_huff of codecs.cpp in a fixed layout
struct JdHuff {
  unsigned short fast[512];   // 9-bit lookahead: (length << 8) | symbol, 0 = longer code
  int maxcode[18], mincode[17], valptr[17];
  unsigned char vals[256];
};

struct JdState { int pos, blk, k; };
JD_HD bool jd_same(const JdState& a, const JdState& b) { return a.pos == b.pos && a.blk == b.blk && a.k == b.k; }

// One restart segment (a file without DRI has one): its first subsequence, the scan-order index of its first block, the blocks it
// holds, the bit range of its data in the staged words
struct JdSeg { int first_sub, blk0, nblocks, start, limit; };
// One subsequence: bits [start, end) of the staged words, all inside segment `seg`; the first one of a segment starts at the
// segment's start with a known state (anchored), the last one ends at or past the segment's limit
struct JdSub { int start, end, seg, flags; };
enum { JD_SUB_ANCHORED = 1, JD_SUB_LAST = 2 };

// What a block of the scan is: component, and the block's place inside the MCU
struct JdScan {
  int nblk;                                   // blocks per MCU
  int ncomp, mcux;
  int restart_blocks;                         // blocks per restart segment (0: no restart interval)
  int comp[JD_MAX_MCU_BLOCKS], bx[JD_MAX_MCU_BLOCKS], by[JD_MAX_MCU_BLOCKS];
  int h[3], v[3], bw[3];                      // per component: sampling factors, blocks per row
  int coef_off[3];                            // first block of the component in the coefficient buffer
};

JD_HD int jd_zigzag(int k) {
  // natural index of zig-zag position k, 4 entries per word would save nothing: a constant table the compiler places itself
  const unsigned char z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k & 63];
}

// The bit reader: 32 bits starting at bit `pos`, zeros at and past `limit`
struct JdBits {
  const uint32_t* w;
  int nwords;
  JD_HD uint32_t word(int i) const { return (i >= 0 && i < nwords) ? w[i] : 0u; }
  JD_HD uint32_t peek32(int pos, int limit) const {
    if (pos >= limit) return 0u;
    const int i = pos >> 5, sh = pos & 31;
    const uint64_t v = ((uint64_t)word(i) << 32) | word(i + 1);
    uint32_t r = (uint32_t)(v >> (32 - sh));
    const int left = limit - pos;            // > 0
    if (left < 32) r &= ~(0xffffffffu >> left);
    return r;
  }
};

JD_HD int jd_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// huff_decode of codecs.cpp on the top bits of `bits`: the symbol (or -1 after 16 bits without a code), *len = bits consumed (1..16)
JD_HD int jd_huff(const JdHuff& h, uint32_t bits, int* len) {
  const int look = (int)(bits >> 23);
  const unsigned short f = h.fast[look];
  if (f) { *len = f >> 8; return f & 255; }
  int code = look;
  for (int l = 10; l <= 16; ++l) {
    code = (code << 1) | (int)((bits >> (32 - l)) & 1u);
    if (h.maxcode[l] >= 0 && code <= h.maxcode[l]) { *len = l; return h.vals[(h.valptr[l] + code - h.mincode[l]) & 255]; }
  }
  *len = 16;
  return -1;
}

// What one step produced
struct JdStep {
  int err;        // JD_OK or the failure of the true decoder at this symbol
  int coef_k;     // >= 0: zig-zag index of the coefficient `value` (0: the DC difference); -1: none
  int value;
  int block_done; // the symbol completed its block
};

// One symbol: decode_block of codecs.cpp (sequential branch), one Huffman code and its extra bits at a time.  A step moves the
// position forward by at least one bit, except that a position more than 64 bits past `limit` is first pulled back to limit + 64
// (all bits there are zero, so nothing changes but the number).  Termination of the loops around it therefore does NOT rest on the
// position alone: every loop counts its steps against a bound fixed before it starts (jd_run_sub, jd_write_sub), and a subsequence's
// end is at most 32 bits past its segment's limit, so the clamp never holds a position in front of an end.  After a failure the state moves on deterministically (speculative decoding starts in the middle of symbols: failures are
// normal there and only the fixed point's are reported).
JD_HD JdStep jd_step(const JdBits& br, int limit, const JdHuff* dc, const JdHuff* ac, const JdScan& sc, JdState* st) {
  JdStep r = {JD_OK, -1, 0, 0};
  int pos = st->pos;
  if (pos > limit + 64) pos = limit + 64;   // every bit from `limit` on is zero: the position need not grow without bound
  const int comp = sc.comp[st->blk];
  int len;
  if (st->k == 0) {
    const int s0 = jd_huff(dc[comp], br.peek32(pos, limit), &len);
    pos += len;
    r.coef_k = 0;
    if (s0 < 0 || s0 > 15) r.err = JD_ERR_DC;
    else if (s0) { r.value = jd_extend((int)(br.peek32(pos, limit) >> (32 - s0)), s0); pos += s0; }
    st->k = 1;
  } else {
    const int rs = jd_huff(ac[comp], br.peek32(pos, limit), &len);
    pos += len;
    if (rs < 0) { r.err = JD_ERR_AC; r.block_done = 1; }
    else {
      const int run = rs >> 4, sz = rs & 15;
      if (sz == 0) {
        if (run == 15) { st->k += 16; if (st->k > 63) r.block_done = 1; }
        else r.block_done = 1;   // EOB
      } else {
        const int k = st->k + run;
        if (k > 63) { r.err = JD_ERR_RUN; r.block_done = 1; }
        else {
          r.coef_k = k;
          r.value = jd_extend((int)(br.peek32(pos, limit) >> (32 - sz)), sz);
          pos += sz;
          st->k = k + 1;
          if (st->k > 63) r.block_done = 1;
        }
      }
    }
  }
  if (r.block_done) { st->k = 0; st->blk = st->blk + 1 == sc.nblk ? 0 : st->blk + 1; }
  st->pos = pos;
  return r;
}

// Where scan-order block g lives: its index in the coefficient buffer (blocks of 64 shorts)
JD_HD int jd_block_index(const JdScan& sc, int g) {
  const int mcu = g / sc.nblk, b = g - mcu * sc.nblk;
  const int my = mcu / sc.mcux, mx = mcu - my * sc.mcux;
  const int c = sc.comp[b];
  return sc.coef_off[c] + (my * sc.v[c] + sc.by[b]) * sc.bw[c] + mx * sc.h[c] + sc.bx[b];
}

// A subsequence from `entry` to the first symbol boundary at or after its end: the exit state, and the blocks completed on the way.
// max_steps bounds the loop whatever the bits are (below the clamp of jd_step every step consumes a bit, so end - start + 64 steps reach the end).
JD_HD JdState jd_run_sub(const JdBits& br, const JdSub& sub, int limit, const JdHuff* dc, const JdHuff* ac, const JdScan& sc, JdState entry,
                         int* blocks) {
  JdState st = entry;
  int n = 0;
  const int max_steps = sub.end - sub.start + 64;
  for (int it = 0; it < max_steps && st.pos < sub.end; ++it) n += jd_step(br, limit, dc, ac, sc, &st).block_done;
  *blocks = n;
  return st;
}

// The final pass over one subsequence from its true entry state: coefficients (natural order, (short) wrap) and raw DC differences
// into `coef`, the first failure in scan order into *status as (scan-order block << 2 | code) through `report`.  base = blocks of the
// segment completed in front of this subsequence.  The last subsequence of a segment goes on (over zero bits) until the segment has
// all its blocks; blocks past the segment's count (padding bits read as symbols) are dropped.
template <typename Report>
JD_HD void jd_write_sub(const JdBits& br, const JdSub& sub, const JdSeg& seg, const JdHuff* dc, const JdHuff* ac, const JdScan& sc,
                        JdState entry, int base, short* coef, Report report) {
  JdState st = entry;
  int local = base;
  const bool last = (sub.flags & JD_SUB_LAST) != 0;
  // steps: the subsequence's bits, or for the last one every symbol the missing blocks can hold
  long max_steps = (long)(sub.end - sub.start) + 64;
  if (last) max_steps += (long)(seg.nblocks > base ? seg.nblocks - base : 0) * 64;
  for (long it = 0; it < max_steps; ++it) {
    if (local >= seg.nblocks) break;
    if (st.pos >= sub.end && !last) break;
    const JdStep r = jd_step(br, seg.limit, dc, ac, sc, &st);
    const int g = seg.blk0 + local;
    if (r.err) { report((unsigned)g << 2 | (unsigned)r.err); }
    else if (r.coef_k >= 0) coef[(long)jd_block_index(sc, g) * 64 + jd_zigzag(r.coef_k)] = (short)r.value;
    local += r.block_done;
  }
}

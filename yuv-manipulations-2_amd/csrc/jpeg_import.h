// jpeg_import.h — the arithmetic of the JPEG import (include/myyuv_hip.h,
// "Import from JPEG"): the marker parser that turns a baseline 4:2:0 file into
// a plan and a table of restart intervals, the decode tables of ITU-T T.81
// F.2.2.3, the bit source that un-stuffs FF 00, the baseline block decoder
// written against it, and the map from a scan's MCUs to the stream's blocks.
// Shared, operation for operation, by the gfx950 kernel (k_jpeg_import.hip),
// the library's host decode of files below the segment threshold
// (myyuv_hip.cpp) and the host program tools/jpeg_import_host.cpp
// (tests/test_jpeg_import_host.py), so the arithmetic exists once.  Plain C++,
// no HIP types; inspect and decode_scans are host-only.
//
// One block's code (T.81 F.2.2): the DC table's symbol c (0..11), c bits of
// the difference (EXTEND), DC = predictor + difference; then AC symbols
// (run << 4 | size): size 0 with run 15 skips 16 positions, size 0 with run 0
// ends the block, any other symbol skips `run` positions and reads `size`
// (1..10) bits of the coefficient at the zig-zag position reached.
#pragma once
#include <stdint.h>

#include "jpeg_export.h"  // kZigzag, the MYYUV_JP_* function attributes

#include <string.h>

namespace myyuv_jpegin {

// the codes of include/myyuv_hip.h (MYYUV_E_JPEG_*), as inspect and decode_scans return them
constexpr int kUnsupported = 21, kSyntax = 22, kData = 23, kTables = 24;
// Files with fewer restart intervals than this in all their scans, or with a
// scan that has none, are decoded on the host (part of the contract).
constexpr uint32_t kSegThreshold = 64;

// A Huffman table in decode form.  Codes of length l are the values
// [first_l, first_l + BITS[l]) of the next l bits; with the next 16 bits w,
// limit[l - 1] = (first_l + BITS[l]) << (16 - l) is non-decreasing in l, so the
// code's length is the smallest l with w < limit[l - 1], and its symbol is
// val[off[l - 1] + (w >> (16 - l))], off = VALPTR - first (F.2.2.3's MAXCODE,
// VALPTR and MINCODE folded into two words per length).
struct DecTab {
  uint32_t limit[16];
  int32_t off[16];
  uint8_t val[256];
};

// false: BITS oversubscribes the code space or names more than 256 symbols.
MYYUV_JP_HD bool build_dectab(const uint8_t bits[16], const uint8_t* vals, uint32_t nvals, DecTab& t) {
  uint32_t code = 0, k = 0;
  for (uint32_t l = 1; l <= 16; l++) {
    t.off[l - 1] = (int32_t)k - (int32_t)code;
    k += bits[l - 1];
    code += bits[l - 1];
    if (code > (1u << l)) return false;
    t.limit[l - 1] = code << (16 - l);
    code <<= 1;
  }
  if (k > 256 || k != nvals) return false;
  for (uint32_t i = 0; i < 256; i++) t.val[i] = i < nvals ? vals[i] : 0;
  return true;
}

// One restart interval of one scan: entropy bytes [off, off + len) of the file
// (to the byte before the RSTm or the next marker), MCUs [mcu0, mcu0 + nmcu).
struct Seg {
  uint32_t off, len, mcu0, nmcu, scan;
};

// Where a scan's MCUs land.  The stream's frame is the file's MCU-padded grid:
// plane p has bw[p] blocks per row, and owns the stream's blocks
// [cum[p], cum[p + 1]).  An interleaved scan (ns 3) has mcux MCUs per row; a
// non-interleaved one (ns 1) covers plane[s]'s own cw[p] x ch[p] blocks,
// ceil(W / 8) x ceil(H / 8) for luma: fewer than the padded grid's when the
// picture's last MCU column or row is half empty.
struct Plan {
  uint32_t mcux, mcuy;
  uint32_t cum[4], bw[3];
  uint32_t cw[3], ch[3];
  uint32_t nscan;
  uint32_t ns[3], plane[3], ri[3];
};

// Block j (0..5: Y00 Y01 Y10 Y11 Cb Cr; 0 in a non-interleaved scan) of MCU
// `mcu` of scan s: the plane, and the block's index in the stream's order.
MYYUV_JP_HD uint32_t block_of_mcu(const Plan& P, uint32_t s, uint32_t mcu, uint32_t j, uint32_t& plane) {
  if (P.ns[s] == 3) {
    const uint32_t my = mcu / P.mcux, mx = mcu - my * P.mcux;
    if (j < 4) {
      plane = 0;
      return (2 * my + (j >> 1)) * P.bw[0] + 2 * mx + (j & 1u);
    }
    plane = j - 3;
    return P.cum[plane] + my * P.bw[plane] + mx;
  }
  plane = P.plane[s];
  const uint32_t by = mcu / P.cw[plane], bx = mcu - by * P.cw[plane];
  return P.cum[plane] + by * P.bw[plane] + bx;
}

// The bit source: bytes [off, off + len) of the file, read through W(i), the
// little-endian 32-bit word at byte 4 i (so a device reads aligned words; the
// first and last word may reach up to 3 bytes beyond the interval, never
// beyond the file's buffer rounded up to 4).  FF 00 is un-stuffed per byte; an
// FF followed by anything else ends the data.  Bits sit left-justified in a
// 64-bit buffer.  skip / get return false / -1 when the interval has fewer
// bits left than asked for (and set `under`).
template <class Words>
struct BitSrc {
  Words W;
  uint32_t pos, end, cw, n;
  uint64_t buf;
  bool under;
  MYYUV_JP_MEMBER BitSrc(Words w, uint32_t off, uint32_t len)
      : W(w), pos(off), end(off + len), cw(0), n(0), buf(0), under(false) {
    if (pos < end) cw = W(pos >> 2);
  }
  MYYUV_JP_MEMBER int next_byte() {
    if (pos >= end) return -1;
    const int b = (int)((cw >> (8 * (pos & 3u))) & 0xFFu);
    pos++;
    if ((pos & 3u) == 0 && pos < end) cw = W(pos >> 2);
    return b;
  }
  MYYUV_JP_MEMBER void fill() {
    while (n <= 56) {
      const int b = next_byte();
      if (b < 0) break;
      if (b == 0xFF && next_byte() != 0) {
        pos = end;
        break;
      }
      buf |= (uint64_t)(uint32_t)b << (56 - n);
      n += 8;
    }
  }
  // the next 16 bits, zeros past the interval's end
  MYYUV_JP_MEMBER uint32_t peek16() {
    if (n < 16) fill();
    return (uint32_t)(buf >> 48);
  }
  MYYUV_JP_MEMBER bool skip(uint32_t k) {  // k <= 16
    if (n < k) fill();
    if (n < k) {
      under = true;
      return false;
    }
    buf <<= k;
    n -= k;
    return true;
  }
  MYYUV_JP_MEMBER int get(uint32_t k) {  // 1 <= k <= 16
    if (n < k) fill();
    if (n < k) {
      under = true;
      return -1;
    }
    const int v = (int)(buf >> (64 - k));
    buf <<= k;
    n -= k;
    return v;
  }
};

// The symbol of the next code, or -1: no code of the table, or the code ends
// beyond the interval.
template <class Src>
MYYUV_JP_HD int decode_symbol(Src& s, const DecTab& t) {
  const uint32_t w = s.peek16();
  // the limits do not decrease: the smallest l with w < limit[l - 1] is one more
  // than the count of limits at or below w (16 independent loads, no branch)
  uint32_t l = 1;
  MYYUV_JP_UNROLL
  for (uint32_t i = 0; i < 16; i++) l += w >= t.limit[i] ? 1u : 0u;
  if (l > 16 || !s.skip(l)) return -1;
  return t.val[(uint32_t)(t.off[l - 1] + (int32_t)(w >> (16 - l))) & 255u];
}

// T.81 F.2.2.1 EXTEND: the value of c >= 1 bits v.
MYYUV_JP_HD int extend(int v, uint32_t c) { return v < (1 << (c - 1)) ? v - (1 << c) + 1 : v; }

// Decodes one block: put(natural index, value) for every nonzero coefficient,
// pred is the component's DC predictor (updated).  Returns nonzero on any of
// the data errors of the definition; what was put before it is to be dropped.
// zz(k): the natural index of zig-zag position k (the kernel reads its LDS
// copy of kZigzag: a constant-memory load per coefficient costs a trip to L2).
template <class Src, class Put, class Zz>
MYYUV_JP_HD int decode_block(Src& s, const DecTab& dc, const DecTab& ac, int& pred, Put put, Zz zz) {
  const int c = decode_symbol(s, dc);
  if (c < 0 || c > 11) return 1;
  int diff = 0;
  if (c) {
    const int v = s.get((uint32_t)c);
    if (v < 0) return 1;
    diff = extend(v, (uint32_t)c);
  }
  const int d = pred + diff;
  if (d < -1024 || d > 1023) return 1;
  pred = d;
  if (d) put(0u, d);
  for (uint32_t k = 1; k < 64;) {
    const int rs = decode_symbol(s, ac);
    if (rs < 0) return 1;
    const uint32_t r = (uint32_t)rs >> 4, sz = (uint32_t)rs & 15u;
    if (sz == 0) {
      if (r == 0) break;       // EOB
      if (r != 15) return 1;
      k += 16;                 // ZRL: a coefficient must follow
      if (k > 63) return 1;
      continue;
    }
    if (sz > 10) return 1;
    k += r;
    if (k > 63) return 1;
    const int v = s.get(sz);
    if (v < 0) return 1;
    put(zz(k), extend(v, sz));
    k++;
  }
  return 0;
}

template <class Src, class Put>
MYYUV_JP_HD int decode_block(Src& s, const DecTab& dc, const DecTab& ac, int& pred, Put put) {
  return decode_block(s, dc, ac, pred, put, [](uint32_t k) { return (uint32_t)myyuv_jpeg::kZigzag[k]; });
}

// ---- host only ---------------------------------------------------------------

// Words of a host buffer of any alignment; bytes past `size` read as 0.
struct HostWords {
  const uint8_t* p;
  uint32_t size;
  uint32_t operator()(uint32_t i) const {
    uint32_t v = 0;
    for (uint32_t b = 0; b < 4; b++) {
      const uint64_t a = 4ull * i + b;
      if (a < size) v |= (uint32_t)p[a] << (8 * b);
    }
    return v;
  }
};

struct Info {
  uint32_t W, H, Wp, Hp;
  uint8_t qt[3][64];    // plane p's quantisation table, natural order
  DecTab dc[3], ac[3];  // plane p's tables, as its scan names them
  Plan plan;
  uint32_t nseg;        // restart intervals of all scans (the segment table's length)
};

// Walks the markers of file[0, size): fills `I`, and segs[0, min(nseg,
// seg_cap)) with one entry per restart interval of every scan, in file order
// (segs may be null with seg_cap 0: I.nseg is the count).  Returns 0,
// kUnsupported or kSyntax, the first in file order.  Reads no byte outside the
// file.
inline int inspect(const uint8_t* file, uint32_t size, Info& I, Seg* segs, uint32_t seg_cap) {
  memset(&I, 0, sizeof(I));
  if (size < 4 || file[0] != 0xFF || file[1] != 0xD8) return kSyntax;
  uint8_t qtab[4][64];
  bool qdef[4] = {false, false, false, false};
  DecTab* htab = new DecTab[8];  // [tc * 4 + th]
  struct Free {
    DecTab* p;
    ~Free() { delete[] p; }
  } guard{htab};
  bool hdef[8] = {false, false, false, false, false, false, false, false};
  bool have_sof = false, covered[3] = {false, false, false};
  uint8_t cid[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
  uint32_t ri = 0, nseg = 0;
  uint64_t pos = 2;
  auto be16 = [&](uint64_t a) { return ((uint32_t)file[a] << 8) | file[a + 1]; };
  for (;;) {
    if (pos + 2 > size || file[pos] != 0xFF) return kSyntax;
    while (pos < size && file[pos] == 0xFF) pos++;  // (fill bytes)
    if (pos >= size) return kSyntax;
    const uint32_t m = file[pos++];
    if (m == 0xD9) break;
    if (m == 0x01) continue;  // TEM
    if (m == 0x00 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7)) return kSyntax;
    if (pos + 2 > size) return kSyntax;
    const uint32_t L = be16(pos);
    if (L < 2 || pos + L > size) return kSyntax;
    const uint8_t* b = file + pos + 2;
    uint32_t n = L - 2;
    pos += L;
    if (m == 0xC0) {
      if (have_sof) return kUnsupported;  // more than one frame
      if (n < 6) return kSyntax;
      const uint32_t nc = b[5];
      I.H = ((uint32_t)b[1] << 8) | b[2];
      I.W = ((uint32_t)b[3] << 8) | b[4];
      if (b[0] != 8 || nc != 3 || I.H == 0) return kUnsupported;  // (height 0: the frame's DNL)
      if (I.W == 0 || n != 6 + 3 * nc) return kSyntax;
      for (uint32_t i = 0; i < 3; i++) {
        cid[i] = b[6 + 3 * i];
        if (b[7 + 3 * i] != (i == 0 ? 0x22 : 0x11)) return kUnsupported;
        ctq[i] = b[8 + 3 * i];
        if (ctq[i] > 3) return kSyntax;
      }
      if (cid[0] == cid[1] || cid[0] == cid[2] || cid[1] == cid[2]) return kSyntax;
      have_sof = true;
      I.Wp = (I.W + 15) / 16 * 16;
      I.Hp = (I.H + 15) / 16 * 16;
      Plan& P = I.plan;
      P.mcux = I.Wp / 16;
      P.mcuy = I.Hp / 16;
      for (uint32_t p = 0; p < 3; p++) {
        P.bw[p] = p == 0 ? I.Wp / 8 : I.Wp / 16;
        P.cw[p] = p == 0 ? (I.W + 7) / 8 : P.mcux;
        P.ch[p] = p == 0 ? (I.H + 7) / 8 : P.mcuy;
        P.cum[p + 1] = P.cum[p] + P.bw[p] * (p == 0 ? I.Hp / 8 : I.Hp / 16);
      }
    } else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4) || m == 0xDC) {
      return kUnsupported;  // other frame types, arithmetic conditioning, DNL
    } else if (m == 0xDB) {
      while (n) {
        if (b[0] >> 4) return kUnsupported;  // 16-bit tables
        const uint32_t tq = b[0] & 15u;
        if (tq > 3 || n < 65) return kSyntax;
        for (uint32_t k = 0; k < 64; k++) {
          if (b[1 + k] == 0) return kSyntax;
          qtab[tq][myyuv_jpeg::kZigzag[k]] = b[1 + k];
        }
        qdef[tq] = true;
        b += 65;
        n -= 65;
      }
    } else if (m == 0xC4) {
      while (n) {
        if (n < 17) return kSyntax;
        const uint32_t tc = b[0] >> 4, th = b[0] & 15u;
        uint32_t nv = 0;
        for (uint32_t i = 0; i < 16; i++) nv += b[1 + i];
        if (tc > 1 || th > 3 || nv > 256 || n < 17 + nv) return kSyntax;
        if (!build_dectab(b + 1, b + 17, nv, htab[tc * 4 + th])) return kSyntax;
        hdef[tc * 4 + th] = true;
        b += 17 + nv;
        n -= 17 + nv;
      }
    } else if (m == 0xDD) {
      if (n != 2) return kSyntax;
      ri = ((uint32_t)b[0] << 8) | b[1];
    } else if (m == 0xEE) {
      if (n >= 12 && memcmp(b, "Adobe", 5) == 0 && b[11] != 1) return kUnsupported;
    } else if (m == 0xDA) {
      if (!have_sof || n < 1) return kSyntax;
      const uint32_t ns = b[0];
      if (ns == 0 || ns > 4 || n != 1 + 2 * ns + 3) return kSyntax;
      if (ns != 1 && ns != 3) return kUnsupported;
      Plan& P = I.plan;
      const uint32_t s = P.nscan;  // (< 3: every scan covers a component not covered before)
      for (uint32_t j = 0; j < ns; j++) {
        uint32_t p = 0;
        while (p < 3 && cid[p] != b[1 + 2 * j]) p++;
        if (p == 3 || (ns == 3 && p != j) || covered[p]) return kSyntax;
        const uint32_t td = b[2 + 2 * j] >> 4, ta = b[2 + 2 * j] & 15u;
        if (td > 3 || ta > 3 || !hdef[td] || !hdef[4 + ta] || !qdef[ctq[p]]) return kSyntax;
        covered[p] = true;
        memcpy(I.qt[p], qtab[ctq[p]], 64);
        I.dc[p] = htab[td];
        I.ac[p] = htab[4 + ta];
        P.plane[s] = p;
      }
      if (b[1 + 2 * ns] != 0 || b[2 + 2 * ns] != 63 || b[3 + 2 * ns] != 0) return kSyntax;
      P.ns[s] = ns;
      P.ri[s] = ri;
      if (ns == 3) P.plane[s] = 0;
      P.nscan = s + 1;
      const uint32_t total = ns == 3 ? P.mcux * P.mcuy : P.cw[P.plane[s]] * P.ch[P.plane[s]];
      // the entropy data: to the first FF that is followed by neither 00 nor (as a marker) RSTm
      uint64_t start = pos, at = pos;
      uint32_t mcu0 = 0, expect = 0;
      for (;;) {
        const uint8_t* f = at < size ? (const uint8_t*)memchr(file + at, 0xFF, size - at) : nullptr;
        if (!f) return kSyntax;  // no EOI
        const uint64_t q = (uint64_t)(f - file);
        uint64_t r = q;
        while (r < size && file[r] == 0xFF) r++;
        if (r >= size) return kSyntax;
        const uint32_t nx = file[r];
        if (nx == 0) {
          if (r != q + 1) return kSyntax;  // fill bytes in front of a stuffed zero
          at = r + 1;
          continue;
        }
        const bool rst = nx >= 0xD0 && nx <= 0xD7;
        if (rst && (ri == 0 || nx != 0xD0 + (expect & 7u))) return kSyntax;
        const uint32_t cnt = ri && total - mcu0 > ri ? ri : total - mcu0;
        if (rst ? mcu0 + cnt >= total : mcu0 + cnt != total) return kSyntax;  // restart count != ceil(MCUs / Ri) - 1
        if (nseg < seg_cap) segs[nseg] = Seg{(uint32_t)start, (uint32_t)(q - start), mcu0, cnt, s};
        nseg++;
        if (!rst) {
          pos = q;
          break;
        }
        mcu0 += cnt;
        expect++;
        start = at = r + 1;
      }
    }
    // (APPn, COM and every other segment: skipped)
  }
  if (!have_sof || !covered[0] || !covered[1] || !covered[2]) return kSyntax;
  I.nseg = nseg;
  return 0;
}

// The host decode: every interval of segs into img, int16 [cum[3]][64] in
// natural order and the stream's block order, zeroed by the caller.  A failing
// block and the rest of its interval stay all-zero.  Returns 0, or kData with
// *bad the lowest failing block.
inline int decode_scans(const uint8_t* file, uint32_t size, const Info& I, const Seg* segs, uint32_t nseg,
                        int16_t* img, int64_t* bad) {
  const Plan& P = I.plan;
  int64_t worst = -1;
  for (uint32_t i = 0; i < nseg; i++) {
    const Seg& S = segs[i];
    BitSrc<HostWords> src(HostWords{file, size}, S.off, S.len);
    int pred[3] = {0, 0, 0};
    const uint32_t nb = P.ns[S.scan] == 3 ? 6 : 1;
    bool ok = true;
    for (uint32_t m = S.mcu0; ok && m < S.mcu0 + S.nmcu; m++) {
      for (uint32_t j = 0; ok && j < nb; j++) {
        uint32_t p;
        const uint32_t g = block_of_mcu(P, S.scan, m, j, p);
        int16_t* blk = img + (size_t)g * 64;
        if (decode_block(src, I.dc[p], I.ac[p], pred[p], [&](uint32_t nat, int v) { blk[nat] = (int16_t)v; })) {
          memset(blk, 0, 128);
          if (worst < 0 || (int64_t)g < worst) worst = g;
          ok = false;
        }
      }
    }
  }
  if (bad) *bad = worst;
  return worst < 0 ? 0 : kData;
}
}  // namespace myyuv_jpegin

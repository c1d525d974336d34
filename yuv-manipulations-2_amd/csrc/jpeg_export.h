// jpeg_export.h — the arithmetic of the JPEG export (include/myyuv_hip.h,
// "Export to JPEG"): the Annex K code tables as (code, length) pairs, the
// category function, the baseline block encoder written against a bit sink,
// and the header writer.  Shared, operation for operation, by the gfx950
// kernel (k_huff_decode.hip k_jpeg_export) and the host program
// tools/jpeg_export_host.cpp (tests/test_jpeg_export_host.py), so the
// arithmetic exists once.  Plain C++, no HIP types.
//
// A block is 64 int16 coefficients in [-1024, 1023]; the encoder reads them in
// zig-zag order through `coef(k)`, k = 0..63.  One block's code:
//   DC   d = coef(0) - pred; c = category(d) (0..11); the DC table's code of c,
//        then the c low bits of d (d - 1 when d < 0);
//   AC   for every nonzero v = max(coef(k), -1023) after a run of r zeros: ZRL
//        (0xF0) for each full 16 of r, then the AC table's code of
//        (r % 16) << 4 | category(v) and category(v) value bits as above;
//   EOB  (0x00) when zeros follow the last nonzero coefficient.
// The sink takes (bits, count) with count <= 26, most significant bit first.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
// (no __forceinline__: that is the HIP runtime header's, which a host program need not include)
#define MYYUV_JP_HD __host__ __device__ inline __attribute__((always_inline))
#define MYYUV_JP_MEMBER __host__ __device__ inline __attribute__((always_inline))
#else
#define MYYUV_JP_HD static inline
#define MYYUV_JP_MEMBER inline
#endif
#if defined(__clang__)
#define MYYUV_JP_UNROLL _Pragma("unroll")
#else
#define MYYUV_JP_UNROLL _Pragma("GCC unroll 64")
#endif

namespace myyuv_jpeg {

// ITU-T T.81 Annex K.3 - K.6: BITS (codes per length 1..16) and HUFFVAL.
constexpr uint8_t kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVal[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumVal[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChrVal[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// JPEG's zig-zag scan: natural index (8 * row + column) of scan position k.
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// One plane class's codes: e[s] = code | length << 16 of symbol s (0: the
// symbol has no code).  ac is indexed by the run/size byte, dc by the category.
constexpr uint32_t kTabWords = 256 + 16;
struct CodeTables {
  uint32_t e[kTabWords];  // [0, 256): AC; [256, 268): DC
};

// The codes of Annex C: within a length in HUFFVAL order, counting up; the
// first code of the next length is the count shifted left.
constexpr CodeTables make_tables(const uint8_t (&dc_bits)[16], const uint8_t (&ac_bits)[16],
                                 const uint8_t (&ac_val)[162]) {
  CodeTables t{};
  uint32_t code = 0;
  int k = 0;
  for (uint32_t len = 1; len <= 16; len++) {
    for (int i = 0; i < dc_bits[len - 1]; i++) t.e[256 + kDcVal[k++]] = code++ | (len << 16);
    code <<= 1;
  }
  code = 0;
  k = 0;
  for (uint32_t len = 1; len <= 16; len++) {
    for (int i = 0; i < ac_bits[len - 1]; i++) t.e[ac_val[k++]] = code++ | (len << 16);
    code <<= 1;
  }
  return t;
}
constexpr CodeTables kLumTables = make_tables(kDcLumBits, kAcLumBits, kAcLumVal);
constexpr CodeTables kChrTables = make_tables(kDcChrBits, kAcChrBits, kAcChrVal);

constexpr uint32_t kRestartBlocks = 64;   // DRI: one interval is one 64-block group of a plane
constexpr uint32_t kMaxBlockBits = 1660;  // 11 + 11, then 63 x (16 + 10)
constexpr uint32_t kMaxBlockBytes = 208;
constexpr uint32_t kMaxDim = 65535;
// SOI, APP0, 3 x DQT, SOF0, 4 x DHT, DRI
constexpr uint32_t kHeaderBytes = 2 + 18 + 3 * 69 + 19 + 2 * (5 + 16 + 12) + 2 * (5 + 16 + 162) + 6;
constexpr uint32_t kSosBytes = 10;
// write_header's bytes as a kernel argument
struct Head {
  uint8_t b[kHeaderBytes];
};

// Bit length of |v|: 0 for 0, up to 11 for a DC difference of +-2047.
MYYUV_JP_HD uint32_t category(int v) {
  const uint32_t a = (uint32_t)(v < 0 ? -v : v);
  return a ? 32u - (uint32_t)__builtin_clz(a) : 0u;
}

// The `cat` bits that follow the code: v, or v - 1 for a negative v.
MYYUV_JP_HD uint32_t value_bits(int v, uint32_t cat) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u); }

// Baseline has no AC category 11: -1024 is written as -1023 (part of the definition).
MYYUV_JP_HD int clamp_ac(int v) { return v < -1023 ? -1023 : v; }

// Tab: dc(category) and ac(run/size byte) return code | length << 16.
// Returns the block's DC (the next block's prediction).
template <class Coef, class Tab, class Sink>
MYYUV_JP_HD int encode_block(Coef coef, int pred, const Tab& tab, Sink& sink) {
  const int dc = coef(0);
  {
    const int d = dc - pred;
    const uint32_t cat = category(d), e = tab.dc(cat);
    sink.put(((e & 0xFFFFu) << cat) | value_bits(d, cat), (e >> 16) + cat);
  }
  const uint32_t zrl = tab.ac(0xF0u);
  uint32_t run = 0;
  MYYUV_JP_UNROLL
  for (int k = 1; k < 64; k++) {
    const int v = clamp_ac(coef(k));
    if (v == 0) {
      run++;
    } else {
      for (; run >= 16; run -= 16) sink.put(zrl & 0xFFFFu, zrl >> 16);
      const uint32_t cat = category(v), e = tab.ac((run << 4) | cat);
      sink.put(((e & 0xFFFFu) << cat) | value_bits(v, cat), (e >> 16) + cat);
      run = 0;
    }
  }
  if (run) {
    const uint32_t e = tab.ac(0u);
    sink.put(e & 0xFFFFu, e >> 16);
  }
  return dc;
}

// A sink that only counts.
struct BitCount {
  uint32_t n = 0;
  MYYUV_JP_MEMBER void put(uint32_t, uint32_t count) { n += count; }
};

MYYUV_JP_HD uint8_t* put16(uint8_t* o, uint32_t v) {
  o[0] = (uint8_t)(v >> 8);
  o[1] = (uint8_t)v;
  return o + 2;
}

MYYUV_JP_HD uint8_t* put_dht(uint8_t* o, uint32_t tc_th, const uint8_t* bits, const uint8_t* val, uint32_t nval) {
  o = put16(o, 0xFFC4u);
  o = put16(o, 2 + 1 + 16 + nval);
  *o++ = (uint8_t)tc_th;
  for (int i = 0; i < 16; i++) *o++ = bits[i];
  for (uint32_t i = 0; i < nval; i++) *o++ = val[i];
  return o;
}

// Everything in front of the first SOS: kHeaderBytes bytes at `out`.  qt[p]:
// plane p's quantisation table in natural order, entries 1..255.
MYYUV_JP_HD uint32_t write_header(uint8_t* out, uint32_t w, uint32_t h, const uint8_t qt[3][64]) {
  uint8_t* o = out;
  o = put16(o, 0xFFD8u);  // SOI
  o = put16(o, 0xFFE0u);  // APP0: JFIF 1.01, no units, 1:1, no thumbnail
  o = put16(o, 16);
  const uint8_t jfif[12] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1};
  for (int i = 0; i < 12; i++) *o++ = jfif[i];
  *o++ = 0;
  *o++ = 0;
  for (uint32_t p = 0; p < 3; p++) {  // DQT: Pq 0, Tq p, zig-zag order
    o = put16(o, 0xFFDBu);
    o = put16(o, 2 + 1 + 64);
    *o++ = (uint8_t)p;
    for (int k = 0; k < 64; k++) *o++ = qt[p][kZigzag[k]];
  }
  o = put16(o, 0xFFC0u);  // SOF0
  o = put16(o, 8 + 3 * 3);
  *o++ = 8;
  o = put16(o, h);
  o = put16(o, w);
  *o++ = 3;
  for (uint32_t p = 0; p < 3; p++) {
    *o++ = (uint8_t)(p + 1);
    *o++ = p == 0 ? 0x22 : 0x11;
    *o++ = (uint8_t)p;
  }
  o = put_dht(o, 0x00, kDcLumBits, kDcVal, 12);
  o = put_dht(o, 0x10, kAcLumBits, kAcLumVal, 162);
  o = put_dht(o, 0x01, kDcChrBits, kDcVal, 12);
  o = put_dht(o, 0x11, kAcChrBits, kAcChrVal, 162);
  o = put16(o, 0xFFDDu);  // DRI
  o = put16(o, 4);
  o = put16(o, kRestartBlocks);
  return (uint32_t)(o - out);
}

// Plane p's scan header: kSosBytes bytes.
MYYUV_JP_HD void write_sos(uint8_t* o, uint32_t p) {
  o = put16(o, 0xFFDAu);
  o = put16(o, 6 + 2);
  *o++ = 1;
  *o++ = (uint8_t)(p + 1);
  *o++ = p == 0 ? 0x00 : 0x11;
  *o++ = 0;
  *o++ = 63;
  *o++ = 0;
}

// Restart intervals of a plane of n blocks.
MYYUV_JP_HD uint32_t intervals(uint32_t n) { return (n + kRestartBlocks - 1) / kRestartBlocks; }

// myyuv_jpeg_bound: the header, three scan headers and EOI, per block twice
// kMaxBlockBytes (byte stuffing at most doubles an interval), and the markers
// between the intervals.
MYYUV_JP_HD uint64_t file_bound(uint32_t w, uint32_t h) {
  const uint64_t ny = (uint64_t)(w / 8) * (h / 8), nc = (uint64_t)(w / 16) * (h / 16);
  const uint64_t iv = (ny + kRestartBlocks - 1) / kRestartBlocks + 2 * ((nc + kRestartBlocks - 1) / kRestartBlocks);
  return kHeaderBytes + 3 * kSosBytes + 2 + (ny + 2 * nc) * 2 * kMaxBlockBytes + 2 * iv;
}

}  // namespace myyuv_jpeg

// metric.h — the arithmetic of Compare (include/myyuv_hip.h, "Compare"): the
// seven integer quantities of one 8x8 block of a plane against the same block
// of another, and the block's SSIM as a 2^24-scaled integer.  Plain C++, no
// floating point.  Included by the kernels (k_huff_decode.hip k_decode_compare,
// k_color.hip k_frame_compare) and by the host program tools/metric_host.cpp
// (tests/test_metric_host.py), so the arithmetic under test is the kernels' own.
//
// x: the 64 reference samples, y: the 64 test samples (u8).  Everything is
// symmetric in x and y.
//   sse = sum (x - y)^2 = Sxx + Syy - 2 Sxy        max = max |x - y|
//   Sx = sum x, Sy = sum y, Sxx = sum x^2, Syy = sum y^2, Sxy = sum x y
//   A1 = 2 Sx Sy + C1              A2 = 2 (64 Sxy - Sx Sy) + C2   (may be negative)
//   B1 = Sx^2 + Sy^2 + C1          B2 = 64 (Sxx + Syy) - Sx^2 - Sy^2 + C2
//   ssim = floor(A1 A2 2^24 / (B1 B2)), floor towards minus infinity
// B1 < 2^29 and B2 < 2^27, so B1 B2 < 2^56; |A1 A2| <= B1 B2 (2ab <= a^2 + b^2
// in both factors), so the quotient is in [-2^24, 2^24]: one compare-subtract
// for the integer part, then 24 shift-subtract steps whose remainder stays
// below 2^57.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
// (no __forceinline__: that is the HIP runtime header's, which a host program need not include)
#define MYYUV_MT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MYYUV_MT_HD inline
#endif

namespace myyuv_metric {

constexpr uint32_t kC1 = 26634;   // round(4096 (0.01 * 255)^2)
constexpr uint32_t kC2 = 239708;  // round(4096 (0.03 * 255)^2)
constexpr int32_t kOne = 1 << 24;

// A block's sums, or any part of them (rows, words): parts add up with add().
struct Sums {
  uint32_t sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0, mx = 0;
};

// Four samples of each side, one per byte of the words.
MYYUV_MT_HD void add_word(Sums& s, uint32_t xw, uint32_t yw) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
  // the same sums on whole words (byte sums as v_sad_u8 against 0, the three
  // products as v_dot4_u32_u8): no sample is unpacked but for the maximum
  s.sx = __builtin_amdgcn_sad_u8(xw, 0u, s.sx);
  s.sy = __builtin_amdgcn_sad_u8(yw, 0u, s.sy);
  s.sxx = __builtin_amdgcn_udot4(xw, xw, s.sxx, false);
  s.syy = __builtin_amdgcn_udot4(yw, yw, s.syy, false);
  s.sxy = __builtin_amdgcn_udot4(xw, yw, s.sxy, false);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t m = 0xFFu << (8 * k);
    const uint32_t d = __builtin_amdgcn_sad_u8(xw & m, yw & m, 0u);
    s.mx = d > s.mx ? d : s.mx;
  }
  return;
#endif
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t x = (xw >> (8 * k)) & 0xFFu, y = (yw >> (8 * k)) & 0xFFu;
    const uint32_t d = x > y ? x - y : y - x;
    s.sx += x;
    s.sy += y;
    s.sxx += x * x;
    s.syy += y * y;
    s.sxy += x * y;
    s.mx = d > s.mx ? d : s.mx;
  }
}

MYYUV_MT_HD void add(Sums& s, const Sums& o) {
  s.sx += o.sx;
  s.sy += o.sy;
  s.sxx += o.sxx;
  s.syy += o.syy;
  s.sxy += o.sxy;
  s.mx = o.mx > s.mx ? o.mx : s.mx;
}

MYYUV_MT_HD uint32_t sse_of(const Sums& s) { return s.sxx + s.syy - 2u * s.sxy; }

// The numerator and the denominator of the block's SSIM.
MYYUV_MT_HD void ssim_terms(const Sums& s, int64_t& num, uint64_t& den) {
  const uint64_t sxsy = (uint64_t)s.sx * s.sy;
  const uint64_t sq = (uint64_t)s.sx * s.sx + (uint64_t)s.sy * s.sy;
  const int64_t a1 = (int64_t)(2u * sxsy + kC1);
  const int64_t a2 = 2 * (64 * (int64_t)s.sxy - (int64_t)sxsy) + (int64_t)kC2;
  const uint64_t b1 = sq + kC1;
  const uint64_t b2 = 64u * ((uint64_t)s.sxx + s.syy) - sq + kC2;
  num = a1 * a2;
  den = b1 * b2;
}

// floor(num 2^24 / den) for |num| <= den < 2^56.
MYYUV_MT_HD int32_t ssim_quotient(int64_t num, uint64_t den) {
  const bool neg = num < 0;
  uint64_t r = neg ? (uint64_t)(-num) : (uint64_t)num;
  uint32_t q = 0;
  if (r >= den) {  // the integer part: at most 1
    r -= den;
    q = 1;
  }
#pragma unroll 1
  for (int i = 0; i < 24; i++) {
    r <<= 1;
    q <<= 1;
    if (r >= den) {
      r -= den;
      q |= 1u;
    }
  }
  // floor of a negative quotient: one further down unless it is exact
  return neg ? -(int32_t)q - (r != 0 ? 1 : 0) : (int32_t)q;
}

MYYUV_MT_HD int32_t ssim_of(const Sums& s) {
  int64_t num;
  uint64_t den;
  ssim_terms(s, num, den);
  return ssim_quotient(num, den);
}

// Two 8x8 sample arrays, row-major.
MYYUV_MT_HD Sums block_sums(const uint8_t* x, const uint8_t* y) {
  Sums s;
  for (int i = 0; i < 64; i += 4) {
    const uint32_t xw = x[i] | ((uint32_t)x[i + 1] << 8) | ((uint32_t)x[i + 2] << 16) | ((uint32_t)x[i + 3] << 24);
    const uint32_t yw = y[i] | ((uint32_t)y[i + 1] << 8) | ((uint32_t)y[i + 2] << 16) | ((uint32_t)y[i + 3] << 24);
    add_word(s, xw, yw);
  }
  return s;
}

}  // namespace myyuv_metric

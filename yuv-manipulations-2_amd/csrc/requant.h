// requant.h — the arithmetic of the requantiser (include/myyuv_hip.h,
// "Requantise"): one decoded coefficient z of a block, quantised with the
// source table's entry qs, becomes the coefficient of the destination table's
// entry qd.  Shared, operation for operation, by the gfx950 kernel
// (k_huff_decode.hip k_requant) and the host program tools/requant_host.cpp
// (tests/test_requant_host.py), so the arithmetic exists once.  Plain C++, no
// HIP types.
//
//   t  = ((float)z * qs) / qd               fp32 multiply, then IEEE fp32 divide
//   z' = clamp((int)roundf(t), -1024, 1023) half away from zero (applyDCTBlock)
//
// z is in [-1024, 1023] and qs, qd are integers 1..255 held as floats
// (make_qtable), so the product is an exact integer below 2^24.  The divide is
// the correctly rounded one (the `/` operator: K1's exact path uses the same),
// never a multiply by a reciprocal.  qd == qs gives z' == z: (z * q) / q is
// exactly z, and z is inside the clamp.  The clamp is part of the definition:
// 1023 * 255 / 1 does not fit the chunk format's 11 bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
// (no __forceinline__: that is the HIP runtime header's, which a host program need not include)
#define MYYUV_RQ_HD __host__ __device__ inline __attribute__((always_inline))
#else
#include <math.h>
#define MYYUV_RQ_HD static inline
#endif

namespace myyuv_requant {

constexpr int kCoefMin = -1024, kCoefMax = 1023;  // the chunk format's 11-bit symbols

MYYUV_RQ_HD int requant_coef(int z, float qs, float qd) {
  const float t = ((float)z * qs) / qd;
  const int r = (int)roundf(t);
  return r < kCoefMin ? kCoefMin : (r > kCoefMax ? kCoefMax : r);
}

// One natural-order word of a block (coefficients 2w, 2w+1 in its halves, as
// the coefficient layout of codec_common.hpp packs them); qs / qd: the two
// tables' entries 2w, 2w+1.
MYYUV_RQ_HD uint32_t requant_word(uint32_t w, float qs0, float qs1, float qd0, float qd1) {
  const int lo = requant_coef((int16_t)(w & 0xFFFFu), qs0, qd0);
  const int hi = requant_coef((int16_t)(w >> 16), qs1, qd1);
  return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
}

}  // namespace myyuv_requant

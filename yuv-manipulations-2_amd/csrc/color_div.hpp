// color_div.hpp — K8's two true divisions (Y / 255, s / 4080) without a
// divide: q = fma(a, h, a * l) with h + l the reciprocal to 48 bits.  a / 255
// with a <= 4080 is exact or at least 2^-33 (relative) from a rounding
// boundary and the form's error is below 2^-47, so q is the correctly rounded
// quotient for every numerator that occurs.  Shared with the host so that the
// claim is checked on the code itself: tools/color_div_check.cpp runs these
// functions over all 256 and all 4081 numerators against the compiler's own
// division (tests/test_yuv_to_bmp_host.py).  Build with -ffp-contract=off:
// the product a * l is rounded on its own.
#pragma once

#if defined(__HIPCC__)
#define MYYUV_COLOR_FN __host__ __device__ __forceinline__
#else
#define MYYUV_COLOR_FN inline
#endif

namespace myyuv_gpu {

constexpr float kR255h = (float)(1.0 / 255.0), kR255l = (float)(1.0 / 255.0 - (double)kR255h);
constexpr float kR4080h = (float)(1.0 / 4080.0), kR4080l = (float)(1.0 / 4080.0 - (double)kR4080h);

MYYUV_COLOR_FN float div_const(float a, float h, float l) { return __builtin_fmaf(a, h, a * l); }
// (float)y / 255.0f for y in 0 .. 255
MYYUV_COLOR_FN float div255(float y) { return div_const(y, kR255h, kR255l); }
// (float)s / 4080.0f for s in 0 .. 4080
MYYUV_COLOR_FN float div4080(float s) { return div_const(s, kR4080h, kR4080l); }

}  // namespace myyuv_gpu

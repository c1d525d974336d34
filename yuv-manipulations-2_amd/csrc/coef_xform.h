// coef_xform.h — the in-block arithmetic and the block-index map of the
// coefficient-domain transform (include/myyuv_hip.h, "Transform"): flip,
// rotate and transpose a DCT stream without pixels.  Shared, operation for
// operation, by the gfx950 kernel (k_huff_decode.hip k_coef_xform) and the
// host program tools/coef_xform_host.cpp (tests/test_coef_xform_host.py), so
// both exist once.  Plain C++, no HIP types.
//
// op is a 3-bit code: bit 0 mirror x, bit 1 mirror y, bit 2 swap (transpose
// first, then the mirrors).  A block's coefficients z[u][v] (u the vertical
// frequency, natural order n = 8u + v) are held as requant.h holds them: 32
// words, word w = coefficients 2w (low half) and 2w + 1 (high half).
//
//   (u', v')   = swap ? (v, u) : (u, v)
//   z1         = requant_coef(z[u][v], Qs[u][v], Qd[u'][v'])          (requant.h)
//   z'[u'][v'] = clamp(s * z1, -1024, 1023),  s = -1 iff (mx and v' odd) xor (my and u' odd)
//
// A mirror of the pixels along an axis is the sign (-1)^k on that axis's k-th
// basis function (cos((2(7 - x) + 1) k pi / 16) = (-1)^k cos((2x + 1) k pi /
// 16)); a transpose of the pixels is the transpose of the coefficients.  The
// clamp matters for one value only: -(-1024) = 1024 -> 1023.
//
// The three steps run on the transposed block: xf_transpose moves the words,
// xf_rescale_row rescales a destination row with the source table read at the
// transposed position (the caller passes it already transposed: qs[n'] =
// Qs[n]) and xf_sign_row negates.  All indices are compile-time constants once
// the loops are unrolled, so a lane's block never leaves its registers.
#pragma once
#include <stdint.h>

#include "requant.h"

#define MYYUV_XF_HD MYYUV_RQ_HD

namespace myyuv_xform {

constexpr uint32_t kMirrorX = 1, kMirrorY = 2, kSwap = 4;

// -z inside the chunk format's 11 bits (only -1024 is touched by the clamp)
MYYUV_XF_HD int neg_coef(int z) {
  const int r = -z;
  return r > myyuv_requant::kCoefMax ? myyuv_requant::kCoefMax : r;
}

// in -> out (distinct arrays): out[u'][v'] = in[v'][u'].  Output word 4u' + k
// holds in[2k][u'] and in[2k + 1][u']: half u' & 1 of input words 8k + u'/2
// and 8k + 4 + u'/2.  Written as shifts and masks so that the host program
// runs the same expression; for gfx950 the compiler makes two VALU
// instructions of each word (and-or / shift-or / bit-field insert) where a
// byte-permute builtin would make one: 32 instructions a block behind a
// decode of thousands, not measurable ("Transform").
MYYUV_XF_HD void xf_transpose(const uint32_t (&in)[32], uint32_t (&out)[32]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int w = 0; w < 32; w++) {
    const int u = w >> 2, k = w & 3;
    const uint32_t a = in[8 * k + (u >> 1)], b = in[8 * k + 4 + (u >> 1)];
    out[w] = (u & 1) ? ((a >> 16) | (b & 0xFFFF0000u)) : ((a & 0xFFFFu) | (b << 16));
  }
}

// One destination row (words 4u' .. 4u' + 3) rescaled: qs, qd are the eight
// entries of the row, qs from the source table at the source position.
MYYUV_XF_HD void xf_rescale_row(uint32_t (&w)[32], int row, const float* qs, const float* qd) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 4; k++)
    w[4 * row + k] = myyuv_requant::requant_word(w[4 * row + k], qs[2 * k], qs[2 * k + 1], qd[2 * k], qd[2 * k + 1]);
}

// The mirrors' signs on one destination row: mirror x negates the odd columns
// (the high halves), mirror y the odd rows; where both apply the signs cancel.
MYYUV_XF_HD void xf_sign_row(uint32_t (&w)[32], int row, bool mx, bool my) {
  const bool nlo = my && (row & 1);         // v' even
  const bool nhi = mx != (my && (row & 1));  // v' odd
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 4; k++) {
    const uint32_t x = w[4 * row + k];
    int lo = (int16_t)(x & 0xFFFFu), hi = (int16_t)(x >> 16);
    lo = nlo ? neg_coef(lo) : lo;
    hi = nhi ? neg_coef(hi) : hi;
    w[4 * row + k] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
  }
}

// The source table as the rescale reads it on the transposed block:
// out[8u' + v'] = Qs[source position of (u', v')].
MYYUV_XF_HD void xf_source_table(uint32_t op, const float* qs, float* out) {
  for (int n = 0; n < 64; n++) out[n] = (op & kSwap) ? qs[8 * (n & 7) + (n >> 3)] : qs[n];
}

// Block (bx, by) of a plane of bw x bh blocks -> its index in the destination
// plane (row-major; bh x bw blocks after a swap).  A bijection of [0, bw * bh).
MYYUV_XF_HD uint32_t xf_dest_block(uint32_t op, uint32_t bw, uint32_t bh, uint32_t bx, uint32_t by) {
  const bool sw = (op & kSwap) != 0;
  const uint32_t bx1 = sw ? by : bx, by1 = sw ? bx : by, bw1 = sw ? bh : bw, bh1 = sw ? bw : bh;
  const uint32_t bxd = (op & kMirrorX) ? bw1 - 1 - bx1 : bx1;
  const uint32_t byd = (op & kMirrorY) ? bh1 - 1 - by1 : by1;
  return byd * bw1 + bxd;
}

// A whole block on the host (and the kernel's order of steps): transpose,
// rescale every row, signs.  qs_t: xf_source_table's table.
MYYUV_XF_HD void xf_block(uint32_t op, const uint32_t (&in)[32], const float* qs_t, const float* qd,
                          uint32_t (&out)[32]) {
  if (op & kSwap) {
    xf_transpose(in, out);
  } else {
    for (int w = 0; w < 32; w++) out[w] = in[w];
  }
  for (int r = 0; r < 8; r++) {
    xf_rescale_row(out, r, qs_t + 8 * r, qd + 8 * r);
    xf_sign_row(out, r, (op & kMirrorX) != 0, (op & kMirrorY) != 0);
  }
}

}  // namespace myyuv_xform

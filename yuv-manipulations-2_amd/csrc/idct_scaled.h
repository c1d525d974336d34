// idct_scaled.h — the arithmetic of the scaled decode (include/myyuv_hip.h,
// "Scaled decode"): the N x N inverse DCT of the low-frequency N x N corner
// of an 8 x 8 block, N = 8 / denom in {4, 2, 1}, which gives an N x N picture
// of the block.  Shared, operation for operation, by the gfx950 kernel
// (k_huff_decode.hip k_decode_scaled) and the host program
// tools/idct_scaled_host.cpp (tests/test_scaled_host.py), so the arithmetic
// exists once.  Plain C++, no HIP types.
//
//   Z[u][v] = (float)z[u][v] * Q[u][v]                  u, v < N
//   U = B_N^T Z,  R = U B_N      every sum from +0.0f, k ascending, products
//                                and sums rounded separately (no FMA)
//   pixel = clamp((int)roundf(R[i][j]) + 128, 0, 255)
//
// B_N is the N-point DCT-II basis with the 8-point norm,
//   B_N[k][i] = fp32(sqrt(N / 8) a_k cos((2 i + 1) k pi / 2 N)),
//   a_0 = sqrt(1 / N), a_k = sqrt(2 / N),
// as literals (computed in double, rounded once).  Every build that includes
// this header needs -ffp-contract=off: a fused multiply-add changes R.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
// (no __forceinline__: that is the HIP runtime header's, which a host program need not include)
#define MYYUV_SC_HD __host__ __device__ inline __attribute__((always_inline))
#define MYYUV_SC_UNROLL _Pragma("unroll")
#else
#include <math.h>
#define MYYUV_SC_HD static inline
#define MYYUV_SC_UNROLL
#endif

namespace myyuv_scaled {

// c: DCT_matrix8[0] of the full transform (0.3535533845424652); s, t: the
// 4-point basis' odd rows
constexpr float kC = 0x1.6a09e6p-2f;
constexpr float kS = 0x1.d906bcp-2f;
constexpr float kT = 0x1.87de2ap-3f;

template <int N>
struct Basis;
template <>
struct Basis<1> {
  static constexpr float b[1] = {kC};
};
template <>
struct Basis<2> {
  static constexpr float b[4] = {kC, kC, kC, -kC};
};
template <>
struct Basis<4> {
  static constexpr float b[16] = {kC, kC, kC, kC, kS, kT, -kT, -kS, kC, -kC, -kC, kC, kT, -kS, kS, -kT};
};

// One block: z and q are the N x N corner of the block's coefficients and of
// the plane's Q table, row-major (element [u][v] at u * N + v); out is the
// block's N x N pixels, row-major.
template <int N>
MYYUV_SC_HD void idct_scaled_block(const int16_t* z, const float* q, uint8_t* out) {
  constexpr const float* B = Basis<N>::b;
  float Z[N * N], U[N * N];
  MYYUV_SC_UNROLL
  for (int n = 0; n < N * N; n++) Z[n] = (float)z[n] * q[n];
  // U[i][j] = sum_k B[k][i] Z[k][j]
  MYYUV_SC_UNROLL
  for (int i = 0; i < N; i++) {
    MYYUV_SC_UNROLL
    for (int j = 0; j < N; j++) {
      float a = 0.0f;
      MYYUV_SC_UNROLL
      for (int k = 0; k < N; k++) a = a + B[k * N + i] * Z[k * N + j];
      U[i * N + j] = a;
    }
  }
  // R[i][j] = sum_k U[i][k] B[k][j], rounded half away from zero, + 128, clamped
  MYYUV_SC_UNROLL
  for (int i = 0; i < N; i++) {
    MYYUV_SC_UNROLL
    for (int j = 0; j < N; j++) {
      float a = 0.0f;
      MYYUV_SC_UNROLL
      for (int k = 0; k < N; k++) a = a + U[i * N + k] * B[k * N + j];
      const int v = (int)roundf(a) + 128;
      out[i * N + j] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
  }
}

}  // namespace myyuv_scaled

// fdct_bfly.h — K1's fast forward transform (round 5): the 8-point DCT of
// the reference's literal basis (DCT.cpp:221-230) evaluated as an even/odd
// butterfly over a NOMINAL basis N (the literal one made exactly symmetric),
// plus the error bound that decides per unit whether the result is provably
// the reference's.  Shared, operation for operation, by the gfx950 kernel
// (xform_common.hpp fdct_fast) and the host check tools/diag/
// fdct_bfly_check.cpp (tests/test_numerics.py), which emulates the kernel's
// arithmetic and compares every unit that passes the bound with the
// reference transform.  That the device build computes what the emulation
// computes is checked on the GPU by the blocks K1 lists
// (tests/test_gpu_fdct_edges.py).
//
// The reference: T = D X (k-ascending sums of rounded products), Y = T D^T,
// coefficient roundf(fl(Y / Q)) (DCT.cpp:232-254, 269-277).  The fast path:
//   stage 1, columns: x = pixel (unsigned; the -128 of DCT.cpp:303 folded
//     into the DC term), s/d butterflies in exact integer-valued floats, then
//     T0 = c0 (E0 - 1024), T4 = c4 E4, T2/T6 two-term, odd rows four-term
//     FMA chains: at most 4 roundings per output;
//   stage 2, rows: the same butterfly on float T, every operation rounded:
//     at most 5 roundings per output.
// With N the matrix this computes in exact arithmetic, delta = max|N - D|
// (<= 5.5 u, u = 2^-24), A = sum |x - 128| over the block, n = d = 0.4904:
//   |T_f - T*| <= (g4 n + delta) A_k =: e1 A_k          (T* = D X exactly)
//   |Y_f - Y*| <= (g5 n (d + e1) + n e1 + delta d) A    (Y* = T* D^T)
//   |Y_ref - Y*| <= g8 d^2 (2 + g8) A
// (g_k = k u / (1 - k u), Higham), so |Y_f - Y_ref| <= kappa A with kappa =
// 11.41 u; |Y_f| <= 0.2406 A.  The quantised value t = fl(Y_f * fl(1/Q))
// then lies within beta = A * r_max * (kappa (1 + 2^-20) + 0.2406 * 2^-21)
// of fl(Y_ref / Q) (the second term: the divide's and the reciprocal's
// roundings), r_max the largest 1/Q of the output's row.  kBflyK = 7.946e-7
// (13.33 u) is that factor with margin (tools/diag/fdct_bfly_derive.py
// computes N, delta and K from the literal basis); kb[row] = kBflyK r_max
// (1 + 2^-20) covers the float evaluation of A * kb.  An output whose t is
// further than beta from every half-integer rounds (half-even, magic add) to
// the reference's roundf of fl(Y_ref / Q): fl(Y_ref / Q) lies strictly inside
// the same (n - 1/2, n + 1/2).  A block with any closer output goes to the
// reference-order transform (k_fdct_fix).
//
// Zero rows.  Stage 2 works row by row (Y[i][.] depends on T[i][.] only), and
// a row of T that is small enough quantises to eight zeros whatever its
// shape; bfly_zero_row() decides that from S = sum_k |T[i][k]| before the row
// is transformed, and a wave whose 16 blocks all pass it for rows 4..7 leaves
// those rows' stage 2 out (fdct_fast: lane q owns rows q and q + 4, so rows
// 4..7 are one half of every lane's work).  The rule, for row i of a block:
//     fl(kb[i] * fma(S_f, kZeroRowK, A)) < 0.5,
// S_f the float sum of the eight |T[i][k]| (7 adds).  It implies the proof
// above for that row, with every output 0:
//   - each y[v] of bfly_rows is a sum of products of its inputs with entries
//     of N, and a rounding only scales a partial result by (1 + d), |d| <= u,
//     so |y_f[v]| <= max|N| (1 + u)^5 S (5 roundings at most, S the exact sum;
//     max|N| = kO1[0]: |y0| <= kC0 S, |y2|, |y6| <= kA2 S, the odd rows
//     max|o| * sum |d_j| <= kO1[0] S);
//   - S <= S_f / (1 - u)^7, and t = fl(y_f * fl(1/Q)) with fl(1/Q) <= r_max,
//     so max_v |t| <= B := max|N| r_max S_f (1 + u)^6 / (1 - u)^7 (a product
//     that underflows is below 2^-126 and passes everything below by itself:
//     A kb <= 8192 * 7.95e-7);
//   - kb[i] >= kBflyK r_max (bfly_row_bounds), so with kZeroRowK >= (max|N| /
//     kBflyK) (1 + u)^6 / (1 - u)^7 (1 + 4 u) the rule's exact value
//     kb (S_f kZeroRowK + A) is >= (A kb + B) + 4 u B, and its two roundings
//     (the fma, the product) lower it by less than 2 u of itself: a float
//     result < 0.5 means A kb + B + 4 u B < 0.5 (1 + 2.01 u), where B > 0.49
//     whenever A kb + B > 0.49 + 0.0066, hence A kb + B < 0.5 (1 - 1.9 u);
//   - then |t| <= B < 0.5, so every magic add of the row gives 0 and e = t,
//     and the existing decision value fma(A, kb[i], max |e|) <= fl(A kb + B)
//     (fma is monotone in its addend and rounds once) <= 0.5 - 2^-25 < 0.5.
// So a row the rule passes is a row the existing proof passes, with zero
// coefficients: what K1 stores and what it lists does not depend on whether a
// wave took the skip, and bfly_block below stays the reference for both.
// kZeroRowK is that minimum times (1 + 2^-20) (fdct_bfly_derive.py prints both;
// the rule could pass ~1e-6 more rows at most).  tools/diag/
// fdct_zero_rows_check.cpp (tests/test_fdct_zero_rows.py) checks the
// implication block by block against bfly_block and the reference transform.
#pragma once

#if defined(__HIPCC__)
#define MYYUV_BF_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define MYYUV_BF_HD static inline
#endif

// MYYUV_BFLY_MUTANT (host check only, tests/test_fdct_edges.py): a deliberately
// wrong build of the arithmetic below, to show that the test inputs tell it
// from the real one.  1: the FMA chains as separate multiplies and adds; 2:
// kC4 replaced by kC0 (one ulp of the constant); 3: kZeroRowK halved (the
// zero-row rule passes rows that are not zero, tests/test_fdct_zero_rows.py).
// Off (0) in every other build; never in device code.
#ifndef MYYUV_BFLY_MUTANT
#define MYYUV_BFLY_MUTANT 0
#endif
#if MYYUV_BFLY_MUTANT && defined(__HIPCC__)
#error "MYYUV_BFLY_MUTANT is for the host check only"
#endif
#if MYYUV_BFLY_MUTANT == 1
#define MYYUV_BF_FMA(a, b, c) ((a) * (b) + (c))
#else
#define MYYUV_BF_FMA(a, b, c) fmaf(a, b, c)
#endif

namespace myyuv_bfly {

// N: row 0 = c0 (the literal row 0 exactly), row 4 = c4 (+ - - + + - - +),
// rows 2 / 6 = (a, b, -b, -a, -a, -b, b, a) / (b, -a, a, -b, -b, a, -a, b),
// odd rows antisymmetric (N[i][7 - m] = -N[i][m]); each value the midpoint of
// the literal entries it stands for (fdct_bfly_derive.py)
#if MYYUV_BFLY_MUTANT == 2
constexpr float kC0 = 0.3535533845424652f, kC4 = kC0;
#else
constexpr float kC0 = 0.3535533845424652f, kC4 = 0.3535534143447876f;
#endif
constexpr float kA2 = 0.4619397521018982f, kB2 = 0.19134166836738586f;
constexpr float kA6 = 0.4619397521018982f, kB6 = 0.19134169816970825f;
constexpr float kO1[4] = {0.49039262533187866f, 0.41573476791381836f, 0.27778512239456177f, 0.09754513204097748f};
constexpr float kO3[4] = {0.41573482751846313f, -0.0975450873374939f, -0.49039262533187866f, -0.277785062789917f};
constexpr float kO5[4] = {0.2777852416038513f, -0.49039262533187866f, 0.09754514694213867f, 0.41573476791381836f};
constexpr float kO7[4] = {0.09754543751478195f, -0.2777852416038513f, 0.4157347083091736f, -0.49039262533187866f};
constexpr float kBflyK = 7.946e-7f;
#if MYYUV_BFLY_MUTANT == 3
constexpr float kZeroRowK = 0.5f * 617157.8125f;
#else
constexpr float kZeroRowK = 617157.8125f;  // 0x1.2d58bap+19 (the header's "Zero rows")
#endif

MYYUV_BF_HD float odd4(const float (&o)[4], float d0, float d1, float d2, float d3) {
  return MYYUV_BF_FMA(o[3], d3, MYYUV_BF_FMA(o[2], d2, MYYUV_BF_FMA(o[1], d1, o[0] * d0)));
}

// Column transform of one block column: p[m] = pixel of row m (0..255, as
// float); t[i] = T[i][k].  Everything before the last products is exact.
MYYUV_BF_HD void bfly_cols(const float (&p)[8], float (&t)[8]) {
  const float s0 = p[0] + p[7], s1 = p[1] + p[6], s2 = p[2] + p[5], s3 = p[3] + p[4];
  const float d0 = p[0] - p[7], d1 = p[1] - p[6], d2 = p[2] - p[5], d3 = p[3] - p[4];
  const float ss0 = s0 + s3, ss1 = s1 + s2, ds0 = s0 - s3, ds1 = s1 - s2;
  t[0] = kC0 * ((ss0 + ss1) - 1024.0f);
  t[4] = kC4 * (ss0 - ss1);
  t[2] = MYYUV_BF_FMA(kA2, ds0, kB2 * ds1);
  t[6] = MYYUV_BF_FMA(kB6, ds0, -kA6 * ds1);
  t[1] = odd4(kO1, d0, d1, d2, d3);
  t[3] = odd4(kO3, d0, d1, d2, d3);
  t[5] = odd4(kO5, d0, d1, d2, d3);
  t[7] = odd4(kO7, d0, d1, d2, d3);
}

// Row transform of one row of T: x[k] = T[i][k]; y[v] = Y[i][v].
MYYUV_BF_HD void bfly_rows(const float (&x)[8], float (&y)[8]) {
  const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
  const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
  const float ss0 = s0 + s3, ss1 = s1 + s2, ds0 = s0 - s3, ds1 = s1 - s2;
  y[0] = kC0 * (ss0 + ss1);
  y[4] = kC4 * (ss0 - ss1);
  y[2] = MYYUV_BF_FMA(kA2, ds0, kB2 * ds1);
  y[6] = MYYUV_BF_FMA(kB6, ds0, -kA6 * ds1);
  y[1] = odd4(kO1, d0, d1, d2, d3);
  y[3] = odd4(kO3, d0, d1, d2, d3);
  y[5] = odd4(kO5, d0, d1, d2, d3);
  y[7] = odd4(kO7, d0, d1, d2, d3);
}

// kb[i] for the rows of one plane: kBflyK * max_v r[i][v] * (1 + 2^-20),
// rounded up (r: the plane's 1 / Q table, natural order).
MYYUV_BF_HD void bfly_row_bounds(const float* r, float* kb) {
  for (int i = 0; i < 8; i++) {
    double m = 0.0;
    for (int v = 0; v < 8; v++) m = r[i * 8 + v] > m ? r[i * 8 + v] : m;
    kb[i] = (float)((double)kBflyK * m * (1.0 + 0x1p-20) * (1.0 + 0x1p-22));
  }
}

// The zero-row rule for one row of T (x[k] = T[i][k], a = the block's A as a
// float, kb = kb[i]): the decision value, and whether the row's eight
// coefficients are proven zero (the header's "Zero rows").  The kernel and
// the host checks run these same operations.
MYYUV_BF_HD float bfly_zero_row_dec(const float (&x)[8], float a, float kb) {
  const float s = ((fabsf(x[0]) + fabsf(x[1])) + (fabsf(x[2]) + fabsf(x[3]))) +
                  ((fabsf(x[4]) + fabsf(x[5])) + (fabsf(x[6]) + fabsf(x[7])));
  return kb * fmaf(s, kZeroRowK, a);
}
MYYUV_BF_HD bool bfly_zero_row(const float (&x)[8], float a, float kb) { return bfly_zero_row_dec(x, a, kb) < 0.5f; }

// Whether a plane's units are tested at all (kb4 = the plane's kb[4], a
// function of its table: kBflyK / the smallest Q of row 4, the row of 4..7 with
// the smallest entries in the quality tables).  With small quantisers hardly
// any unit passes and the test only costs: on a noisy 3968x2944 photo at q90
// (luma: row 4's smallest Q = 4, no unit of 11,408 passes; chroma: 20, 28-40 %
// pass) K1 ran 1.0 % slower than without the test, the parent's own spread
// being 0.2 % (profiles/r10a_zero_rows_ab.txt); at q75 (luma 9: 10 % pass,
// chroma 50: 56-77 %) the planes together gain.  The gate lies between: planes
// whose row 4 has an entry below 6 are not tested (luma from q ~ 84 up, chroma
// from q 98).  Output does not depend on it.
constexpr float kZeroRowGate = kBflyK / 5.5f;
MYYUV_BF_HD bool bfly_zero_rows_tested(float kb4) { return kb4 < kZeroRowGate; }

#if !defined(__HIPCC__)
// The kernel's arithmetic for one whole block (host check): coefficients in
// natural order; returns 0 when some output is not provably the reference's.
// d (may be null): what decided, for the per-block listing of the check.
struct BflyDetail {
  int row, col;  // the row with the largest fma(A, kb[row], max |e|), the output with the largest |e| in it
  float dec;     // that largest value (the block is unproven when dec >= 0.5)
  float a;       // A
  float t[64];   // every output's t = Y_f * fl(1 / Q)
};
static inline int bfly_block(const unsigned char* px, const float* R, const float* kb, short* out,
                             BflyDetail* d = nullptr) {
  unsigned a = 0;
  for (int i = 0; i < 64; i++) a += px[i] > 128 ? px[i] - 128u : 128u - px[i];
  const float af = (float)a;
  float T[8][8];
  for (int k = 0; k < 8; k++) {
    float p[8], t[8];
    for (int m = 0; m < 8; m++) p[m] = (float)px[m * 8 + k];
    bfly_cols(p, t);
    for (int i = 0; i < 8; i++) T[i][k] = t[i];
  }
  int ok = 1;
  for (int i = 0; i < 8; i++) {
    float y[8];
    bfly_rows(T[i], y);
    float em = 0.0f;
    int vm = 0;
    for (int v = 0; v < 8; v++) {
      const float t = y[v] * R[i * 8 + v];
      const float uu = t + 0x1.8p23f;
      const float e = t - (uu - 0x1.8p23f);
      if (fabsf(e) > em) vm = v;
      em = fmaxf(em, fabsf(e));
      out[i * 8 + v] = (short)(int)(uu - 0x1.8p23f);
      if (d) d->t[i * 8 + v] = t;
    }
    const float dec = fmaf(af, kb[i], em);
    if (dec >= 0.5f) ok = 0;  // (the kernel: one fma, max over the rows)
    if (d && (i == 0 || dec > d->dec)) {
      d->row = i;
      d->col = vm;
      d->dec = dec;
    }
  }
  if (d) d->a = af;
  return ok;
}
// The block's votes in fdct_fast: bit i - 4 set when row i (4..7) passes the
// zero-row rule; dec (may be null): the four decision values.  A wave skips
// the rows' stage 2 when all of its storing blocks return 15.
static inline int bfly_block_zero_rows(const unsigned char* px, const float* kb, float* dec = nullptr) {
  unsigned a = 0;
  for (int i = 0; i < 64; i++) a += px[i] > 128 ? px[i] - 128u : 128u - px[i];
  float T[8][8];
  for (int k = 0; k < 8; k++) {
    float p[8], t[8];
    for (int m = 0; m < 8; m++) p[m] = (float)px[m * 8 + k];
    bfly_cols(p, t);
    for (int i = 0; i < 8; i++) T[i][k] = t[i];
  }
  int votes = 0;
  for (int i = 4; i < 8; i++) {
    if (dec) dec[i - 4] = bfly_zero_row_dec(T[i], (float)a, kb[i]);
    if (bfly_zero_row(T[i], (float)a, kb[i])) votes |= 1 << (i - 4);
  }
  return votes;
}
#endif

}  // namespace myyuv_bfly

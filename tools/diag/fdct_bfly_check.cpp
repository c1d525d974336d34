/* Diagnostic + test harness (CPU, test infrastructure): K1's butterfly fast
 * path (xform_common.hpp fdct_fast, round 5) emulated operation for operation
 * in IEEE binary32 (gcc -ffp-contract=off, explicit fmaf), against the
 * reference transform (myyuv_DCT/DCT.cpp:232-254, 269-277: k-ascending sums of
 * rounded products, roundf(Y / Q)).  Per 16-block unit: the fast path's
 * bound test (beta_h = A * kb[row], kb = K * max_v r[row][v]); a unit that
 * passes must equal the reference in every coefficient (any mismatch is a
 * failure of the bound: exit 1).  Counts the units the exact path must take.
 *
 * stdin: u32 nblocks, then per block 64 u8 pixels (row-major) + u8 plane id;
 * then 3 x 64 f32 Q tables (natural order).  Units are 16 consecutive blocks
 * of one plane (the caller orders them that way).
 * stdout: "units <n> exact <m> mismatches <k> outputs <o> blocks <b> fixblocks <f>"
 * (exact: units with a block over the bound; fixblocks: such blocks, which
 * k_fdct_fix recomputes — every other block is checked against the reference)
 *
 * --per-block: after that line, "maxratio <x>": the largest |t - fl(Y_ref / Q)|
 * / (A * kb[row]) over every output of every block with A > 0 (the bound of
 * fdct_bfly.h says < 1), t the fast path's quantised value; then one line per
 * block: "<index> <ok> <row> <col> <dec> <t> <tie row> <tie col> <tie>": the
 * deciding row (the arg max of fma(A, kb[i], max |e|) over the rows) and
 * column (the arg max of |e| in that row), the float bits (hex) of that
 * maximum and of the deciding output's t, and where the reference's
 * fl(Y_ref / Q) comes nearest to a half-integer and how near (float bits of
 * the distance).  --dec-window W / --tie-window W: only the blocks whose
 * maximum lies within W of 0.5 / whose distance is at most W (searches).
 * -DMYYUV_BFLY_MUTANT=n builds a deliberately wrong emulation (fdct_bfly.h);
 * its mismatches do not fail the run.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const float Dm[64] = {
    0.3535533845424652f,   0.3535533845424652f,  0.3535533845424652f,  0.3535533845424652f,
    0.3535533845424652f,   0.3535533845424652f,  0.3535533845424652f,  0.3535533845424652f,
    0.4903925955295563f,   0.4157347679138184f,  0.277785062789917f,   0.09754510968923569f,
    -0.09754515439271927f, -0.2777851521968842f, -0.4157347977161407f, -0.4903926253318787f,
    0.4619397222995758f,   0.1913416981697083f,  -0.1913417428731918f, -0.4619397819042206f,
    -0.4619397222995758f,  -0.1913415491580963f, 0.1913417875766754f,  0.4619397521018982f,
    0.4157347679138184f,   -0.09754515439271927f, -0.4903926253318787f, -0.2777849733829498f,
    0.2777851819992065f,   0.4903925955295563f,  0.09754502773284912f, -0.4157348573207855f,
    0.3535533547401428f,   -0.3535533547401428f, -0.353553295135498f,  0.3535534739494324f,
    0.3535533547401428f,   -0.3535535931587219f, -0.3535532355308533f, 0.3535533845424652f,
    0.277785062789917f,    -0.4903926253318787f, 0.09754519909620285f, 0.4157346487045288f,
    -0.4157348573207855f,  -0.09754510223865509f, 0.4903926253318787f, -0.2777853906154633f,
    0.1913416981697083f,   -0.4619397222995758f, 0.4619397521018982f,  -0.1913419365882874f,
    -0.1913414746522903f,  0.4619396328926086f,  -0.4619398415088654f, 0.1913419365882874f,
    0.09754510968923569f,  -0.2777849733829498f, 0.4157346487045288f,  -0.4903925657272339f,
    0.4903926849365234f,   -0.4157347679138184f, 0.2777855396270752f,  -0.09754576534032822f};

#include "../../yuv-manipulations-2_amd/csrc/fdct_bfly.h"
using namespace myyuv_bfly;

/* reference: T = D X, Y = T D^T, roundf(Y / Q) (DCT.cpp:232-254, 269-277) */
static void ref_block(const uint8_t* px, const float* Q, int16_t* out, float* tq = nullptr) {
  float X[64], T[64], Y[64];
  for (int i = 0; i < 64; i++) X[i] = (float)((int)px[i] - 128);
  for (int i = 0; i < 8; i++)
    for (int j = 0; j < 8; j++) {
      float s = 0.0f;
      for (int k = 0; k < 8; k++) s = s + Dm[i * 8 + k] * X[k * 8 + j];
      T[i * 8 + j] = s;
    }
  for (int i = 0; i < 8; i++)
    for (int j = 0; j < 8; j++) {
      float s = 0.0f;
      for (int k = 0; k < 8; k++) s = s + T[i * 8 + k] * Dm[j * 8 + k];
      Y[i * 8 + j] = s;
    }
  for (int i = 0; i < 64; i++) out[i] = (int16_t)roundf(Y[i] / Q[i]);
  if (tq)
    for (int i = 0; i < 64; i++) tq[i] = Y[i] / Q[i];
}

static uint32_t fbits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char** argv) {
  int per_block = 0;
  double dec_window = -1.0, tie_window = -1.0;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--per-block"))
      per_block = 1;
    else if (!strcmp(argv[i], "--dec-window") && i + 1 < argc)
      dec_window = atof(argv[++i]);
    else if (!strcmp(argv[i], "--tie-window") && i + 1 < argc)
      tie_window = atof(argv[++i]);
    else
      return 2;
  }
  uint32_t n;
  if (fread(&n, 4, 1, stdin) != 1) return 2;
  uint8_t* px = (uint8_t*)malloc((size_t)n * 65);
  if (fread(px, 65, n, stdin) != n) return 2;
  float Q[3][64], R[3][64], KB[3][8];
  if (fread(Q, 4, 192, stdin) != 192) return 2;
  for (int p = 0; p < 3; p++) {
    for (int i = 0; i < 64; i++) R[p][i] = 1.0f / Q[p][i];
    bfly_row_bounds(R[p], KB[p]);
  }
  long units = 0, exact = 0, mism = 0, outputs = 0, fixblocks = 0;
  struct Line {
    uint32_t index;
    int ok, row, col, trow, tcol;
    float dec, t, tie;
  };
  Line* lines = per_block ? (Line*)malloc((size_t)(n ? n : 1) * sizeof(Line)) : nullptr;
  size_t nlines = 0;
  double maxratio = 0.0;
  for (uint32_t u0 = 0; u0 < n; u0 += 16) {
    const uint32_t nb = n - u0 < 16 ? n - u0 : 16;
    int ok = 1;
    int16_t fast[16][64];
    int okb[16];
    for (uint32_t b = 0; b < nb; b++) {
      const uint8_t* blk = px + (size_t)(u0 + b) * 65;
      const int p = blk[64];
      BflyDetail d;
      okb[b] = bfly_block(blk, R[p], KB[p], fast[b], per_block ? &d : nullptr);
      ok &= okb[b];
      fixblocks += !okb[b];
      if (per_block) {
        int16_t ref[64];
        float tq[64];
        ref_block(blk, Q[p], ref, tq);
        Line L = {u0 + b, okb[b], d.row, d.col, 0, 0, d.dec, d.t[d.row * 8 + d.col], 1.0f};
        for (int i = 0; i < 64; i++) {
          const double fr = (double)tq[i] - floor((double)tq[i]);
          const float dist = (float)fabs(fr - 0.5);
          if (dist < L.tie) {
            L.tie = dist;
            L.trow = i / 8;
            L.tcol = i % 8;
          }
          if (d.a > 0.0f) {
            const double ratio = fabs((double)d.t[i] - (double)tq[i]) / ((double)d.a * (double)KB[p][i / 8]);
            if (ratio > maxratio) maxratio = ratio;
          }
        }
        const bool all = dec_window < 0.0 && tie_window < 0.0;
        if (all || (dec_window >= 0.0 && fabs((double)d.dec - 0.5) <= dec_window) ||
            (tie_window >= 0.0 && (double)L.tie <= tie_window))
          lines[nlines++] = L;
      }
    }
    units++;
    exact += !ok;
    /* K1 stores every block that passes its own bound (the exact path takes
       the blocks that do not): each passing block must be the reference's */
    for (uint32_t b = 0; b < nb; b++) {
      if (!okb[b]) continue;
      const uint8_t* blk = px + (size_t)(u0 + b) * 65;
      int16_t ref[64];
      ref_block(blk, Q[blk[64]], ref);
      for (int i = 0; i < 64; i++) {
        outputs++;
        if (ref[i] != fast[b][i]) {
          if (mism < 10) fprintf(stderr, "mismatch block %u coef %d: fast %d ref %d\n", u0 + b, i, fast[b][i], ref[i]);
          mism++;
        }
      }
    }
  }
  printf("units %ld exact %ld mismatches %ld outputs %ld blocks %u fixblocks %ld\n", units, exact, mism, outputs, n,
         fixblocks);
  if (per_block) {
    printf("maxratio %.9g\n", maxratio);
    for (size_t i = 0; i < nlines; i++)
      printf("%u %d %d %d %08x %08x %d %d %08x\n", lines[i].index, lines[i].ok, lines[i].row, lines[i].col,
             fbits(lines[i].dec), fbits(lines[i].t), lines[i].trow, lines[i].tcol, fbits(lines[i].tie));
  }
  return mism && !MYYUV_BFLY_MUTANT ? 1 : 0;
}

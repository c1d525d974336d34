// k_transform.hip — K1 fdct_quant and K6 dequant_idct for gfx950,
// k_coef_compare, K6's transform against a source frame, and k_bmp_fdct, K1's
// transform fed from BMP pixels (at the end).
//
// Streaming kernels: K1 reads 1 B/sample (u8 pixel) and writes 2 B/sample
// (int16 coefficient), K6 the reverse (3 B/sample each).  The
// bit-exact transform is 8 fp32 products + 7 sums per output per stage in a
// fixed order (~30 VALU per sample); at the 8 TB/s ridge the budget is ~10
// lane-ops per byte, so the arithmetic and the memory stream both set the
// pace, and the code is shaped to overlap them:
//   * persistent waves: each wave strides over 16-block units of the frame
//     and issues the NEXT unit's loads (pixel rows / coefficient quads)
//     before transforming the current one, so HBM latency hides behind the
//     wave's own arithmetic; every wave is independent (no workgroup
//     barrier; all LDS traffic is wave-local);
//   * issue rates measured on this chip (tools/ubench/valu_mix.hip,
//     profiles/r01_ubench_valu_mix.txt): independent VOP2 f32 ops with an
//     inline literal issue every ~1.0 ns per SIMD; packed v_pk_* ops do two
//     lanes of work in ~1.9 ns but take no literals, so the transform is
//     scalar with the basis as literals;
//   * dependent chains slow issue (a v_add waiting on its v_mul): every stage
//     keeps 16 independent accumulators per lane and advances them together;
//   * quantisation by multiply-by-reciprocal and the 1.5*2^23 magic add, with
//     a cheap test that routes the rare near-tie samples to the IEEE divide
//     (below); K6 rounds with the same magic add;
//   * no zig-zag here: coefficients are stored in natural order (the
//     permutation is free where they are consumed/produced, K2/K5).
//
// Geometry: four lanes per 8x8 block, 16 blocks (a "unit", never straddling
// planes, so the tables are uniform per unit) per wave.  Lane (b, q),
// q = lane & 3:
//   stage 1 owns columns 2q, 2q+1 (T[i][2q], T[i][2q+1] for i = 0..7),
//   stage 2 owns rows 2q, 2q+1    (Y[2q][v], Y[2q+1][v] for v = 0..7) in K6,
//           and rows q, q+4       (Y[q][v], Y[q+4][v]) in K1, so that rows
//           4..7 of all 16 blocks are one half of every lane's stage 2 and
//           the wave can leave it out together (zero rows, below),
// and the 8x8 transposes (pixel rows -> columns, stage 1 -> stage 2) go
// through a per-wave LDS tile (tix(); K1's second one tixf()).  Lane (b, q)
// loads / stores the block's pixel rows 2q, 2q+1 directly (8 B each; 16
// blocks x 8 B = 128 B runs per row); K6 loads the coefficient quads 2q,
// 2q+1, K1 stores the quads q, q+4 (codec_common.hpp layout; 256 B runs
// either way).  The per-quality tables (QTables) are a device buffer.
// A launch covers a batch of frames (FrameGeom::nframes): the waves stride
// over the units of all of them, frame f's unit u being f * ucum[3] + u.
//
// Bit-exactness (SURVEY.md §7 hard part 1, App. C).  K1's fast path
// (fdct_fast, xform_common.hpp) is an even/odd BUTTERFLY over a nominal
// basis N (the literal DCT_matrix8 of DCT.cpp:221-230 made exactly symmetric,
// fdct_bfly.h): it does not reproduce the reference's operation order, so
// each 16-block unit carries a proof instead.  With A = sum |x - 128| over the
// block, |Y_fast - Y_ref| <= kappa * A (Higham gamma_k bounds on both
// evaluations plus max|N - D|; fdct_bfly.h), and a row whose every
// t = Y_fast * fl(1/Q) stays further than A * kb[row] from a half-integer
// quantises to the reference's roundf(fl(Y_ref / Q)).  A BLOCK where any row
// fails is listed (the proof is per block: A and the row factors are the
// block's own) and recomputed by k_fdct_fix in the reference's order: the
// straight k-ascending sums of fp32-rounded products (DCT.cpp:232-266),
// -ffp-contract=off (fdct_exact; its only fma is the near-tie test below).
// Zero rows: before stage 2, S = sum_k |T[i][k]| bounds every output of row
// i, and fl(kb[i] * fma(S, kZeroRowK, A)) < 0.5 implies both that all eight
// t of the row round to 0 and that the row's proof above passes (fdct_bfly.h,
// "Zero rows").  When every storing lane of a wave finds that for its row
// q + 4, the wave skips stage 2, the quantisation, the packing, the info
// word's counts and the store of rows 4..7: the bytes K1 writes and the blocks
// it lists are those of the full path, whichever way a wave went.
// tools/diag/fdct_bfly_check.cpp (tests/test_numerics.py) replays the fast
// arithmetic on the host and checks every proven block equals the reference;
// tools/diag/fdct_zero_rows_check.cpp (tests/test_fdct_zero_rows.py) checks
// that the zero-row rule implies the proof.  K6 keeps the reference's order
// throughout.
//   exact path /Q + roundf: t = y * fl(1/Q) is within |t| * 1.5 * 2^-23 of fl(y/Q)
//     (two roundings of relative error 2^-24 plus fl(y/Q)'s own), so
//     roundf(fl(y/Q)) == rint(t) unless a half-integer lies within
//     |t| * 2^-21 of t.  rint(t) comes from u = t + 1.5*2^23 (|t| < 2^22:
//     the sum rounds to an integer, half-even; its low 16 bits are the int16
//     two's complement), e = t - (u - 1.5*2^23) is exact, and the distance
//     to the nearest half-integer is 0.5 - |e|.  Each sample's
//     x = fma(|t|, 2^-21, |e|) is >= 0.5 whenever 0.5 - |e| <= |t| * 2^-21
//     (fma rounds once and 0.5 is a float, so no near-tie is missed; exact
//     ties, where rint and roundf disagree, give x >= 0.5 too); a lane whose
//     max x reaches 0.5 recomputes its 16 outputs with the reference's divide
//     and roundf.  tools/check_numerics.c (tests/test_numerics.py) checks the
//     rule against the divide around every half-integer for every Q (a 2^-24
//     window already fails it).
//   K6 roundf + clamp: s' = med3(s, -128, 127) then u = s' + (1.5*2^23 + 128)
//     rounds half-even to an integer whose low byte is the pixel; only exact
//     ties (fract(s') == 0.5: v_fract_f32 is exact here, and a non-tie never
//     has a fractional part of exactly 0.5), where roundf goes away from zero,
//     differ, and the lane redoes those with truncf(x + copysignf(0.49999997f,
//     x)) == roundf(x) (exhaustively checked for all 2^32 floats).
// No MFMA: this is not a dense contraction, and the bound above admits only
// evaluations whose every operation rounds once to nearest.
#include <stddef.h>

#include "bmp_fdct.h"
#include "codec_common.hpp"
#include "color_px.hpp"
#include "k1_store.hpp"
#include "k_metric.hpp"
#include "xform_common.hpp"

// K1: 8 waves per SIMD (its LDS allows 8 workgroups per CU); the compiler
// otherwise settles at 69 VGPRs (7 waves) with the block-info computation
#ifndef MYYUV_K1_OCC
#define MYYUV_K1_OCC 8
#endif
#define MYYUV_K1_ATTR __attribute__((amdgpu_waves_per_eu(MYYUV_K1_OCC, MYYUV_K1_OCC)))

namespace myyuv_gpu {

using namespace xf;

// K1: u8 planes -> int16 coefficients (natural order, quad layout).
// DCT.cpp:297-306 (gather, x - 128), :269-277 (applyDCTBlock).
// (its hand-off to K2, store_block_rows[_buf]: k1_store.hpp)

// K1's exact path out of line: a unit whose fast result is not provably the
// reference's is appended by K1 to one of kFixLists lists (unit ua to list
// ua % kFixLists, fix_count / fix_list in codec_common.hpp; each launch uses
// the counts of its parity `par`) and transformed by k_fdct_fix, which runs
// next in the stream.  Kept in K1, the exact path's code raised K1 from 64 to
// 99 VGPRs (7 -> 5 waves per SIMD) and cost it 15 % (profiles/r4g_*).  One
// count for all units serialised the appends on one address (at q90, 18 % of
// the units: 47k atomics per 8192x8192 frame, K1 83 -> 215 us); a per-wave
// register list flushed 64 at a time fixed that but cost K1 4 % at q50
// (profiles/r4r_*).

__global__ __launch_bounds__(256) MYYUV_K1_ATTR void k_fdct_quant(const uint8_t* __restrict__ frame, FrameGeom G,
                                                   const QTables* __restrict__ qt,
                                                   uint4* __restrict__ coef, uint8_t* __restrict__ rmask,
                                                   uint32_t* __restrict__ binfo, uint4* __restrict__ sink,
                                                   uint32_t* __restrict__ k2ctl, uint32_t* __restrict__ fix,
                                                   uint32_t par) {
  // K2's overflow count for the launch that follows in the stream (nullptr: none)
  if (k2ctl != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *k2ctl = 0u;
  __shared__ float tile[4][kXfUnit * kTile];
  __shared__ float sqr[kSqWords];  // QTables::q, r, kb
  __shared__ uint4 szz[8];
  static_assert(offsetof(QTables, r) == sizeof(float) * kSqR && offsetof(QTables, kb) == sizeof(float) * kSqKb,
                "layout");
  stage_zz(szz);
  stage_tables<kSqWords>(qt->q[0], sqr);
  if (kSinkSlots > 1) sink += (size_t)((blockIdx.x * 4u + (threadIdx.x >> 6)) % kSinkSlots) * kSinkQuads;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = lane & 3u, b = lane >> 2;  // quarter, block in the unit
  float* tb = tile[threadIdx.x >> 6] + b * kTile;
  uint8_t* img = reinterpret_cast<uint8_t*>(tb);  // the block's 8 x 8 B pixel image (aliases tb)
#if MYYUV_K1_BUF
  const K1Rsrc rs = k1_rsrc(coef, rmask, binfo, G);
#endif
  // batch units: unit u of frame f is ua = f * ucum[3] + u
  const uint32_t nall = G.ucum[3] * G.nframes, stride = unit_stride();
  uint32_t ua = first_unit();
  uint4 nx = ua < nall ? load_rows(frame, G, ua, b, q) : make_uint4(0, 0, 0, 0);
  // two stores behind the first loads, as every iteration has behind its
  // prefetch: the loop top then waits with vmcnt(2) on every path
  sink[lane] = make_uint4(0, 0, 0, 0);
  sink[64 + lane] = make_uint4(0, 0, 0, 0);
  reinterpret_cast<uint8_t*>(sink + 128)[lane] = 0;

  for (; ua < nall; ua += stride) {
    const uint32_t f = div_magic(ua, G.umag);
    const Unit U = unit_of(G, ua - f * G.ucum[3]);
    const uint32_t local = U.local0 + b;
    const bool live = local < U.nb;
    const uint32_t g = f * G.cum[3] + U.cum + local;
    // ---- this unit's rows 2q, 2q+1 into the block's image; the next unit's
    // rows in flight behind this unit's arithmetic
    *reinterpret_cast<uint2*>(img + 16u * q) = make_uint2(nx.x, nx.y);
    *reinterpret_cast<uint2*>(img + 16u * q + 8u) = make_uint2(nx.z, nx.w);
    // (the last unit reloads itself: an unconditional load keeps the
    // in-order vmcnt accounting exact, so the loop top waits for these two
    // loads only, not for the stores behind them)
    nx = load_rows(frame, G, ua + stride < nall ? ua + stride : ua, b, q);
    wave_sync();

    // stores of lanes past the plane's end, and of blocks left to the exact
    // path, go to the sink (no branch: see load_rows)
    auto store = [&](const uint32_t (&c)[16], bool keep, auto hz) {
      constexpr bool kHz = decltype(hz)::value;  // rows 4..7 of the unit are zero
      const bool lv = live && keep;
#if MYYUV_K1_BUF
      store_block_rows_buf<kHz>(c, q, lv, g, rs, szz);
#else
      uint4* dlo = lv ? coef + coef_quad(g, q) : sink + lane;
      uint4* dhi = lv ? coef + coef_quad(g, q + 4) : sink + 64 + lane;
      store_block_rows<kHz>(c, q, lane, lv, g, dlo, dhi, rmask, binfo, szz, sink);
#endif
    };
    uint32_t xr[4];
    fdct_load(img, q, xr);
    const uint64_t bad = fdct_fast<true>(xr, tb, q, live, sqr, U.p, store);
    if (bad != 0) {  // (wave-uniform) the unproven blocks, listed by their lane 4b
      const bool mine = ((bad >> lane) & 1u) && q == 0 && live;
      const uint64_t m = __ballot(mine);
      const uint32_t c = ua % kFixLists;
      uint32_t base = 0;
      // (a launch lists each block at most once, so a count below the list's
      // capacity is guaranteed while k_fdct_fix resets the counts; the clamp
      // keeps a stale count, e.g. a diagnostic skip of the fix kernel, in bounds)
      if (lane == 0 && m != 0) base = atomicAdd(fix_count(fix, par, c), (uint32_t)__popcll(m));
      base = __builtin_amdgcn_readfirstlane(base);
      const uint32_t idx = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (mine && idx < fix_list_cap(nall)) fix_list(fix, G, c)[idx] = ua * kXfUnit + b;
    }
  }
}

// K1's exact path for the blocks K1 listed (kFixLists lists, the counts of
// parity par; entry ua * 16 + b: block slot b of unit ua): a wave takes 16
// listed blocks at a time, in any planes and frames (lane (b, q) takes
// entry b: its geometry, plane and Q tables per lane), the reference's order
// (fdct_exact), the same stores.  Wave w takes list w % kFixLists (the grid's
// waves are a multiple of kFixLists).  Workgroup 0 zeroes the other parity's
// counts, which the next K1 fills (the previous fix launch, their reader, is
// done: stream order).  Per block rather than per unit: at q90 on the bench
// frame 20 % of the units but 1.8 % of the blocks are unproven
// (tools/diag/fdct_bfly_check.cpp).
__global__ __launch_bounds__(64 * kFixWaves) void k_fdct_fix(const uint8_t* __restrict__ frame, FrameGeom G,
                                                  const QTables* __restrict__ qt, uint4* __restrict__ coef,
                                                  uint8_t* __restrict__ rmask, uint32_t* __restrict__ binfo,
                                                  uint4* __restrict__ sink,
                                                  uint32_t* __restrict__ fix, uint32_t par) {
  __shared__ float tile[kFixWaves][kXfUnit * kTile];
  __shared__ float sqr[2 * 3 * 64];
  __shared__ uint4 szz[8];
  __shared__ uint32_t s_any;
  if (blockIdx.x == 0 && threadIdx.x < kFixLists) *fix_count(fix, par ^ 1u, threadIdx.x) = 0u;
  if (threadIdx.x == 0) s_any = 0u;
  __syncthreads();
  const uint32_t gw = blockIdx.x * kFixWaves + (threadIdx.x >> 6), nw = gridDim.x * kFixWaves;
  const uint32_t c = gw % kFixLists;
  const uint32_t n = __builtin_amdgcn_readfirstlane(*fix_count(fix, par, c));
  if ((threadIdx.x & 63u) == 0 && gw / kFixLists * kXfUnit < n) s_any = 1u;
  __syncthreads();
  if (s_any == 0u) return;  // (uniform over the workgroup)
  stage_zz(szz);
#pragma unroll
  for (uint32_t i = threadIdx.x; i < 2u * 3u * 64u; i += 64u * kFixWaves) sqr[i] = qt->q[0][i];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = lane & 3u, b = lane >> 2;
  float* tb = tile[threadIdx.x >> 6] + b * kTile;
  uint8_t* img = reinterpret_cast<uint8_t*>(tb);
  const uint32_t* list = fix_list(fix, G, c);
#if MYYUV_K1_BUF
  const K1Rsrc rs = k1_rsrc(coef, rmask, binfo, G);
#endif
  for (uint32_t i = gw / kFixLists * kXfUnit; i < n; i += nw / kFixLists * kXfUnit) {
    // lanes past the list's end redo entry i (a real block) into the sink
    const bool real = i + b < n;
    const uint32_t ent = list[real ? i + b : i];
    const uint32_t ua = ent / kXfUnit, bb = ent % kXfUnit;
    const uint32_t f = div_magic(ua, G.umag);
    const Unit U = unit_of(G, ua - f * G.ucum[3]);
    const uint32_t g = f * G.cum[3] + U.cum + U.local0 + bb;
    const uint4 r = load_rows(frame, G, ua, bb, q);
    wave_sync();  // (the previous blocks' tile reads are done)
    *reinterpret_cast<uint2*>(img + 16u * q) = make_uint2(r.x, r.y);
    *reinterpret_cast<uint2*>(img + 16u * q + 8u) = make_uint2(r.z, r.w);
    wave_sync();
    uint32_t xr[4];
    fdct_load(img, q, xr);
#if MYYUV_K1_BUF
    fdct_exact(xr, tb, q, sqr, U.p, [&](const uint32_t (&cc)[16]) { store_block_rows_buf(cc, q, real, g, rs, szz); });
#else
    uint4* dlo = real ? coef + coef_quad(g, q) : sink + lane;
    uint4* dhi = real ? coef + coef_quad(g, q + 4) : sink + 64 + lane;
    fdct_exact(xr, tb, q, sqr, U.p,
               [&](const uint32_t (&cc)[16]) {
                 store_block_rows(cc, q, lane, real, g, dlo, dhi, rmask, binfo, szz, sink);
               });
#endif
  }
}

// K6's per-wave walk over the launch's 16-block units, shared by K6 and
// k_coef_compare: dequantise, both stages of the inverse transform in the
// reference's order, roundf and clamp; `out` says what becomes of the pixel
// rows.  out.begin(ua, b, q) runs once the next unit's loads are issued (a
// place to issue loads of its own for unit ua, which then fly behind the
// unit's arithmetic); out.rows(ua, f, U, local, q, lane, w0, w1) takes rows
// 2q (w0) and 2q+1 (w1) of block `local` of the unit's plane in frame f;
// out.end() runs after the wave's last unit.  tile: the workgroup's transpose
// tiles, sq: QTables::q staged by the kernel.
template <class Out>
__device__ __forceinline__ void dequant_idct_units(const uint4* __restrict__ coef,
                                                   const uint8_t* __restrict__ rmask,
                                                   const uint4* __restrict__ zq, const FrameGeom& G,
                                                   float (*tile)[kXfUnit * kTile], const float* sq,
                                                   uint4* __restrict__ sink, Out& out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = lane & 3u, b = lane >> 2;
  float* tb = tile[threadIdx.x >> 6] + b * kTile;
  uint32_t* tw = reinterpret_cast<uint32_t*>(tb);  // the block's int16 image (aliases tb)
  const uint32_t nall = G.ucum[3] * G.nframes, stride = unit_stride();
  uint32_t ua = first_unit();
  uint4 na = make_uint4(0, 0, 0, 0), nc = na;
  uint32_t un = ua + stride < nall ? ua + stride : ua, nm = 0;
  if (ua < nall) {
    const uint32_t g0 = unit_block(G, ua, b);
    load_quads(coef, zq, g0, q, rmask[g0], na, nc);
    nm = rmask[unit_block(G, un, b)];
  }
  sink[lane] = make_uint4(0, 0, 0, 0);  // see K1
  sink[64 + lane] = make_uint4(0, 0, 0, 0);

  for (; ua < nall; ua += stride) {
    const uint32_t f = div_magic(ua, G.umag);
    const Unit U = unit_of(G, ua - f * G.ucum[3]);
    const uint32_t local = U.local0 + b;
    // ---- rows 2q, 2q+1 of coefficients into the block's image (first 32
    // dwords of its tile); the next unit's quads in flight
    *reinterpret_cast<uint4*>(tw + 8 * q) = na;
    *reinterpret_cast<uint4*>(tw + 8 * q + 4) = nc;
    load_quads(coef, zq, unit_block(G, un, b), q, nm, na, nc);  // unconditional: see K1
    un = un + stride < nall ? un + stride : un;
    nm = rmask[unit_block(G, un, b)];
    out.begin(ua, b, q);
    wave_sync();
    // (Z[k][2q], Z[k][2q+1]) = word k*4 + q
    uint32_t zc[8];
#pragma unroll
    for (int k = 0; k < 8; k++) zc[k] = tw[k * 4 + q];
    wave_sync();
    // the quantisers of columns 2q, 2q+1: qk[2k + h] = Q[k][2q + h]
    const float* Qt = sq + U.p * 64;
    float qk[16];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const float2 v = *reinterpret_cast<const float2*>(Qt + k * 8 + 2 * q);
      qk[2 * k] = v.x;
      qk[2 * k + 1] = v.y;
    }

    // ---- dequantise (DCT.cpp:331) and stage 1: U[i][j] = sum_k D[k][i] * Z[k][j],
    // j in {2q, 2q+1} (squareMatrixMulT2<8>(DCT, Z), DCT.cpp:256-266)
    // Quantised blocks are sparse: a coefficient row k that is zero in all 16
    // blocks of the unit (61 % of the (unit, k) pairs of the bench frame)
    // contributes only +-0 products, and a sum that starts at +0 (as the
    // reference's does, DCT.cpp:259-263) is unchanged by them — so the wave
    // skips that step outright, bit-exactly.  Stage 2 skips the zero columns
    // of Z the same way (U's column k is zero exactly when Z's is).
    float Um[16];  // Um[2i + h] = U[i][2q + h]
#pragma unroll
    for (int j = 0; j < 16; j++) Um[j] = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      if (!__any(zc[k] != 0u)) continue;
      const float z0 = (float)(int16_t)zc[k] * qk[2 * k];
      const float z1 = (float)(int16_t)(zc[k] >> 16) * qk[2 * k + 1];
      float pr[16];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        pr[2 * i] = c_dct[k * 8 + i] * z0;
        pr[2 * i + 1] = c_dct[k * 8 + i] * z1;
      }
#pragma unroll
      for (int j = 0; j < 16; j++) Um[j] = Um[j] + pr[j];
      fence16(Um);
    }

    // ---- transpose (the float tile reuses the block's LDS)
    float P[16];  // P[2k + h] = U[2q + h][k]
    transpose_tile(tb, q, Um, P);

    // ---- stage 2: R[i][v] = sum_k U[i][k] * D[k][v] (squareMatrixMul<8>(U, DCT)),
    // then clamp(roundf(R) + 128) (DCT.cpp:358-362)
    float S[16];  // S[2v + h] = R[2q + h][v]
    dot_rows<true, true>(P, S);
    uint32_t px[16];  // low byte = pixel
    bool tie = false;  // an exact .5 in the lane: fract(s') == 0.5 (exact for |s'| <= 128)
#pragma unroll
    for (int j = 0; j < 16; j++) {
      S[j] = __builtin_amdgcn_fmed3f(S[j], -128.0f, 127.0f);
      const float uu = S[j] + kMagicPx;
      tie = tie || __builtin_amdgcn_fractf(S[j]) == 0.5f;
      px[j] = bits(uu);
    }
    if (tie) {  // an exact .5 somewhere in the lane: roundf goes away from zero
#pragma unroll
      for (int j = 0; j < 16; j++)
        px[j] = (uint32_t)((int)__builtin_truncf(S[j] + __builtin_copysignf(kHalfDown, S[j])) + 128);
    }
    // rows 2q (even j) and 2q+1 (odd j): bytes v = 0..7 of each
    const uint2 w0 = make_uint2(__builtin_amdgcn_perm(__builtin_amdgcn_perm(px[6], px[4], 0x0c0c0400u),
                                                      __builtin_amdgcn_perm(px[2], px[0], 0x0c0c0400u),
                                                      0x05040100u),
                                __builtin_amdgcn_perm(__builtin_amdgcn_perm(px[14], px[12], 0x0c0c0400u),
                                                      __builtin_amdgcn_perm(px[10], px[8], 0x0c0c0400u),
                                                      0x05040100u));
    const uint2 w1 = make_uint2(__builtin_amdgcn_perm(__builtin_amdgcn_perm(px[7], px[5], 0x0c0c0400u),
                                                      __builtin_amdgcn_perm(px[3], px[1], 0x0c0c0400u),
                                                      0x05040100u),
                                __builtin_amdgcn_perm(__builtin_amdgcn_perm(px[15], px[13], 0x0c0c0400u),
                                                      __builtin_amdgcn_perm(px[11], px[9], 0x0c0c0400u),
                                                      0x05040100u));
    out.rows(ua, f, U, local, q, lane, w0, w1);
  }
  out.end();
}

// K6's sink: pixel rows 2q, 2q+1 of the block out (8 B each; lanes past the
// plane's end write the sink)
struct StoreRows {
  const FrameGeom& G;
  uint8_t* __restrict__ frame;
  uint4* __restrict__ sink;
  __device__ __forceinline__ void begin(uint32_t, uint32_t, uint32_t) {}
  __device__ __forceinline__ void rows(uint32_t, uint32_t f, const Unit& U, uint32_t local, uint32_t q, uint32_t lane,
                                       uint2 w0, uint2 w1) {
    const bool live = local < U.nb;
    const uint32_t off = block_row_offset(U, live ? local : 0u, 2u * q);
    uint8_t* fr = frame + (size_t)f * G.fbytes;
    uint2* d0 = live ? reinterpret_cast<uint2*>(fr + off) : reinterpret_cast<uint2*>(sink + lane);
    uint2* d1 = live ? reinterpret_cast<uint2*>(fr + off + U.pw) : reinterpret_cast<uint2*>(sink + 64 + lane);
    *d0 = w0;
    *d1 = w1;
  }
  __device__ __forceinline__ void end() {}
};

// K6: int16 coefficients (natural order, quad layout) -> u8 planes.
// DCT.cpp:330-334 (dequant, squareMatrixMulT2, squareMatrixMul), :358-362
// (roundf, +128, clamp).
__global__ __launch_bounds__(256) void k_dequant_idct(const uint4* __restrict__ coef,
                                                     const uint8_t* __restrict__ rmask,
                                                     const uint4* __restrict__ zq, FrameGeom G,
                                                     const QTables* __restrict__ qt,
                                                     uint8_t* __restrict__ frame, uint4* __restrict__ sink) {
  __shared__ float tile[4][kXfUnit * kTile];
  __shared__ float sq[3 * 64];  // QTables::q
  stage_tables<3 * 64>(qt->q[0], sq);
  StoreRows out{G, frame, sink};
  dequant_idct_units(coef, rmask, zq, G, tile, sq, sink, out);
}

// k_coef_compare: K6 with a source frame where K6 has its output (include/
// myyuv_hip.h, "Probe").  The coefficient image is the one K1 and k_fdct_fix
// leave (coef, rmask: K5's hand-off to K6 is the same contract), so the rows
// are those of "compress at q, decode": where K6 stores rows 2q, 2q+1 of a
// block, this kernel has loaded the source frame's rows from the same offsets
// (load_rows, issued before the unit's transform, which hides the latency) and
// adds the rows' part of the block's sums (metric.h); the block's four lanes
// then hold its sums (mt::fold_lanes<4>).  A wave keeps four units' blocks,
// the blocks of its unit number n in the lanes with q == n % 4, and then
// finishes 64 blocks at once (mt::finish_units): the 24-step quotient runs
// once per four units, every lane busy, as in k_decode_compare.  Each unit's
// totals go to its own slot part[ua] (16 B per 16 blocks, 1/64 of the source
// read), which k_metric_reduce adds up per plane with the planes' unit counts:
// no atomics, every slot written by every launch.  Neither a chunk nor a
// decoded frame exists in HBM.
struct CompareRows {
  const FrameGeom& G;
  const uint8_t* __restrict__ src;
  uint4* __restrict__ part;
  myyuv_block_metric* __restrict__ map;
  uint4 x = make_uint4(0, 0, 0, 0);  // the unit's source rows 2q (x, y), 2q+1 (z, w)
  mt::Sums held;                     // the block this lane keeps
  uint32_t held_g = 0, held_ua = 0;  // its index in the launch, its unit
  bool held_live = false, held_unit = false;
  uint32_t n = 0;  // units since the last finish (wave-uniform)
  __device__ __forceinline__ void begin(uint32_t ua, uint32_t b, uint32_t q) { x = load_rows(src, G, ua, b, q); }
  __device__ __forceinline__ void rows(uint32_t ua, uint32_t f, const Unit& U, uint32_t local, uint32_t q, uint32_t,
                                       uint2 w0, uint2 w1) {
    mt::Sums ps;
    myyuv_metric::add_word(ps, x.x, w0.x);
    myyuv_metric::add_word(ps, x.y, w0.y);
    myyuv_metric::add_word(ps, x.z, w1.x);
    myyuv_metric::add_word(ps, x.w, w1.y);
    mt::fold_lanes<4>(ps);  // (the whole wave is active: the loop's branch is wave-uniform)
    if (q == n) {
      held = ps;
      held_g = f * G.cum[3] + U.cum + local;
      held_ua = ua;
      held_live = local < U.nb;
      held_unit = true;
    }
    if (++n == 4u) end();
  }
  __device__ __forceinline__ void end() {
    if (n == 0u) return;  // (wave-uniform)
    mt::finish_units(held, held_live, held_unit, part + held_ua, map != nullptr ? map + held_g : nullptr);
    held_live = held_unit = false;
    n = 0;
  }
};

__global__ __launch_bounds__(256) void k_coef_compare(const uint4* __restrict__ coef,
                                                     const uint8_t* __restrict__ rmask,
                                                     const uint4* __restrict__ zq, FrameGeom G,
                                                     const QTables* __restrict__ qt,
                                                     const uint8_t* __restrict__ src, uint4* __restrict__ part,
                                                     myyuv_block_metric* __restrict__ map,
                                                     uint4* __restrict__ sink) {
  __shared__ float tile[4][kXfUnit * kTile];
  __shared__ float sq[3 * 64];  // QTables::q
  stage_tables<3 * 64>(qt->q[0], sq);
  CompareRows out{G, src, part, map};
  dequant_idct_units(coef, rmask, zq, G, tile, sq, sink, out);
}

// ---- compress from BMP ------------------------------------------------------
//
// k_bmp_fdct<BPP>: K7's conversion and K1's transform in one launch, the IYUV
// frame never in HBM (include/myyuv_hip.h, "Compress from BMP").  The work map
// is bmp_fdct.h's: wave blockIdx.x of frame blockIdx.y owns a strip of 16 pixel
// rows by up to 256 columns, up to 16 macroblocks.
//  - Conversion: lane l converts the eight 4 x 2 tiles of the strip's tile
//    column l (px::tile_row: K7's arithmetic), one 16-B (BGRA) or 12-B (BGR)
//    load per tile row, a wave-instruction reading 1 KiB (768 B) of one pixel
//    row; the loads of four tiles are issued before the first is converted, so
//    HBM latency hides behind the wave's own arithmetic.  The luma dwords and
//    chroma byte pairs go into the wave's image of block pictures (72-B slots:
//    the stores and fdct_load's reads are bank-conflict-free, bmp_fdct.h).
//  - Transform: up to four Y units, one U, one V unit of 16 slots, four lanes
//    per block (fdct_core: K1's fast path and, on a failed proof, the exact path
//    in the same wave, so there is no fix list).  Each unit's quads, row masks
//    and info words go out as K1's do (store_block_rows_buf) at the block's
//    index in the frame; slots past the strip's blocks are dropped by the
//    descriptors' range (a narrow strip's unused slots hold pixel 128).
// Every block of the frame belongs to exactly one wave, every source pixel is
// read once, nothing depends on another wave, and there is no barrier.
// (3 waves per SIMD: the wave's LDS, 13 KiB with the image, the transpose tile
// and K1's tables, admits 12 workgroups per CU)
#ifndef MYYUV_BMP_DEPTH
// tiles whose loads are issued before the first is converted (1, 2, 4 or 8);
// all 8 measured the same as 4 (8192x8192 BGRA: 157 against 159 us), for 3 more VGPRs
#define MYYUV_BMP_DEPTH 4
#endif
template <int BPP>
__global__ __launch_bounds__(64) void k_bmp_fdct(const uint8_t* __restrict__ src, myyuv_bmpfdct::Map M, FrameGeom G,
                                                 const QTables* __restrict__ qt, uint4* __restrict__ coef,
                                                 uint8_t* __restrict__ rmask, uint32_t* __restrict__ binfo) {
  namespace bf = myyuv_bmpfdct;
  static_assert(bf::kUnit == kXfUnit && bf::kSlotBytes % 8 == 0, "fdct_load's 8-B rows, K1's units");
  static_assert(offsetof(QTables, r) == sizeof(float) * kSqR && offsetof(QTables, kb) == sizeof(float) * kSqKb,
                "layout");
  __shared__ uint2 simg[bf::kSlots * bf::kSlotBytes / 8];
  __shared__ float tile[kXfUnit * kTile];
  __shared__ float sqr[kSqWords];  // QTables::q, r, kb
  __shared__ uint4 szz[8];
  const uint32_t lane = threadIdx.x;
  const bf::Strip S = bf::strip_of(M, blockIdx.x);
  uint8_t* img = reinterpret_cast<uint8_t*>(simg);
  stage_zz(szz);
  for (uint32_t i = lane; i < (uint32_t)kSqWords; i += kWave) sqr[i] = qt->q[0][i];
  if (S.nmb < 16u) {  // (wave-uniform) a narrow strip: its unused slots are transformed with the rest of their unit
    for (uint32_t i = lane; i < bf::kSlots * bf::kSlotBytes / 8; i += kWave) simg[i] = make_uint2(0x80808080u, 0x80808080u);
    wave_sync();
  }

  // ---- conversion: tile column `lane`, kDepth tiles' loads in flight at a time
  constexpr uint32_t kDepth = MYYUV_BMP_DEPTH;
  static_assert(bf::kTileRows % kDepth == 0, "whole batches");
  if (lane < bf::live_lanes(S)) {
    // the lane's first tile row; row r of the strip is r * step bytes further (wave-uniform)
    const uint8_t* fr = src + (size_t)blockIdx.y * ((size_t)M.w * M.h * BPP) + (size_t)bf::tile_src(M, S, lane, 0, 0) * BPP;
    const int64_t step = bf::row_step(M) * BPP;
#pragma unroll
    for (uint32_t t0 = 0; t0 < bf::kTileRows; t0 += kDepth) {
      uint32_t w[kDepth][2][BPP];
#pragma unroll
      for (uint32_t i = 0; i < kDepth; i++)
#pragma unroll
        for (uint32_t dr = 0; dr < 2; dr++) px::load4<BPP>(fr + (int64_t)(2 * (t0 + i) + dr) * step, 0, w[i][dr]);
#pragma unroll
      for (uint32_t i = 0; i < kDepth; i++) {
        const uint32_t ty = t0 + i;
        uint32_t Y[2] = {0, 0}, cb[2] = {0, 0}, cr[2] = {0, 0};
        px::tile_row<BPP>(w[i][0], M.orient == 1, Y[0], cb, cr);
        px::tile_row<BPP>(w[i][1], M.orient == 1, Y[1], cb, cr);
        *reinterpret_cast<uint32_t*>(img + bf::luma_byte(S, lane, ty, 0)) = Y[0];
        *reinterpret_cast<uint32_t*>(img + bf::luma_byte(S, lane, ty, 1)) = Y[1];
        uint8_t* uc = img + bf::chroma_byte(lane, ty);
        *reinterpret_cast<uint16_t*>(uc) = (uint16_t)((cb[0] & 0xFFu) | (cb[1] & 0xFFu) << 8);
        *reinterpret_cast<uint16_t*>(uc + (bf::kSlotV - bf::kSlotU) * bf::kSlotBytes) =
            (uint16_t)((cr[0] & 0xFFu) | (cr[1] & 0xFFu) << 8);
      }
    }
  }
  wave_sync();  // the image is complete

  // ---- K1's per-unit body on the strip's blocks, lane (b, q)
  const uint32_t q = lane & 3u, b = lane >> 2;
  float* tb = tile + b * kTile;
  const K1Rsrc rs = k1_rsrc(coef, rmask, binfo, G);
  const uint32_t nu = bf::units(S);
#pragma unroll 1
  for (uint32_t k = 0; k < nu; k++) {
    const bf::UnitOf U = bf::unit_of(S, k);
    const bool lv = b < U.nlive;
    const uint32_t g = blockIdx.y * G.cum[3] + (U.p == 0 ? G.cum[0] : (U.p == 1 ? G.cum[1] : G.cum[2])) +
                       bf::plane_block(M, S, U, lv ? b : 0u);
    fdct_core(img + bf::kSlotBytes * (U.slot0 + b), tb, q, lv, sqr, U.p,
              [&](const uint32_t (&c)[16], bool keep, auto hz) {
                store_block_rows_buf<decltype(hz)::value>(c, q, lv && keep, g, rs, szz);
              });
    wave_sync();  // the next unit rewrites the tile
  }
}

template __global__ void k_bmp_fdct<3>(const uint8_t*, myyuv_bmpfdct::Map, FrameGeom, const QTables*, uint4*, uint8_t*,
                                       uint32_t*);
template __global__ void k_bmp_fdct<4>(const uint8_t*, myyuv_bmpfdct::Map, FrameGeom, const QTables*, uint4*, uint8_t*,
                                       uint32_t*);

}  // namespace myyuv_gpu

// downscale.h — the work map of the downscaler (include/myyuv_hip.h,
// "Downscale"): which wave decodes which source blocks, where a lane's
// N x N pixels land, and which output block they belong to.  Shared by the
// gfx950 kernel (k_huff_decode.hip k_downscale) and the host program
// tools/downscale_host.cpp (tests/test_downscale_host.py), so the map exists
// once.  Plain C++, no HIP types.
//
// With denom in {2, 4, 8} and N = 8 / denom, an output block is the N x N
// pictures of a denom x denom square of source blocks.  A BAND is the denom
// source block rows under one output block row; a SEGMENT is up to kSeg = 64
// consecutive block columns of a band.  Wave t owns one segment: it decodes
// the band as denom RUNS, run r being the segment's columns in source block
// row orow * denom + r (one contiguous byte range of the plane's content, one
// chunk per lane), and then owns the segment's n / denom output blocks.  n is
// a multiple of denom: the planes' widths in blocks are (W and H are multiples
// of 16 denom), and so is kSeg.
//
// Waves are numbered plane-major, band-major, segment-minor.  The wave's
// pixel image holds its output blocks one after the other, each as 8 rows of
// 8 bytes (what fdct_load reads).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MYYUV_DS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MYYUV_DS_HD static inline
#endif

namespace myyuv_downscale {

constexpr uint32_t kSeg = 64;  // source block columns per wave (one lane each)

// Per plane: source and output blocks per block row, output block rows
// (bands), segments per band; wcum: the planes' waves, cumulative.
struct Map {
  uint32_t denom;
  uint32_t sbw[3], dbw[3], dbh[3], spr[3];
  uint32_t wcum[4];
};

// The map of a W x H frame at 1 / denom (W and H multiples of 16 denom; the
// callers have checked).
MYYUV_DS_HD Map make_map(uint32_t w, uint32_t h, uint32_t denom) {
  Map M;
  M.denom = denom;
  M.wcum[0] = 0;
  for (int p = 0; p < 3; p++) {
    const uint32_t sh = p ? 4 : 3;  // log2 of the plane's block size in luma pixels
    M.sbw[p] = w >> sh;
    M.dbw[p] = M.sbw[p] / denom;
    M.dbh[p] = (h >> sh) / denom;
    M.spr[p] = (M.sbw[p] + kSeg - 1) / kSeg;
    M.wcum[p + 1] = M.wcum[p] + M.spr[p] * M.dbh[p];
  }
  return M;
}

// Wave t: its plane, band (= output block row), first source block column,
// source columns n, output blocks nout, and the first of them inside the
// output plane.
struct Wave {
  int p;
  uint32_t orow, col0, n, nout, ob0;
};

MYYUV_DS_HD Wave wave_of(const Map& M, uint32_t t) {
  Wave W;
  W.p = t >= M.wcum[1] ? (t >= M.wcum[2] ? 2 : 1) : 0;
  const int p = W.p;
  const uint32_t ts = t - (p == 0 ? 0u : (p == 1 ? M.wcum[1] : M.wcum[2]));
  const uint32_t spr = p == 0 ? M.spr[0] : (p == 1 ? M.spr[1] : M.spr[2]);
  const uint32_t sbw = p == 0 ? M.sbw[0] : (p == 1 ? M.sbw[1] : M.sbw[2]);
  const uint32_t dbw = p == 0 ? M.dbw[0] : (p == 1 ? M.dbw[1] : M.dbw[2]);
  W.orow = ts / spr;
  const uint32_t k = ts - W.orow * spr;
  W.col0 = kSeg * k;
  W.n = sbw - W.col0 < kSeg ? sbw - W.col0 : kSeg;
  W.nout = W.n / M.denom;
  W.ob0 = W.orow * dbw + W.col0 / M.denom;
  return W;
}

// Run r of wave W: the first source block of the run inside its plane (lane l
// decodes block run_first + l, l < W.n).
MYYUV_DS_HD uint32_t run_first(const Map& M, const Wave& W, uint32_t r) {
  const uint32_t sbw = W.p == 0 ? M.sbw[0] : (W.p == 1 ? M.sbw[1] : M.sbw[2]);
  return (W.orow * M.denom + r) * sbw + W.col0;
}

// Lane l of run r: the wave's output block its pixels belong to, and the byte
// of the wave's image where pixel row i (i < N) of its N x N picture starts:
// block slot l / denom, cell (r, l % denom) of the block's denom x denom cells.
MYYUV_DS_HD uint32_t lane_slot(uint32_t denom, uint32_t l) { return l / denom; }
MYYUV_DS_HD uint32_t lane_pixel(uint32_t denom, uint32_t r, uint32_t l, uint32_t i) {
  const uint32_t N = 8 / denom;
  return 64 * (l / denom) + 8 * (r * N + i) + N * (l % denom);
}

// The wave's output block slot j (j < W.nout) inside the output plane.
MYYUV_DS_HD uint32_t out_block(const Wave& W, uint32_t j) { return W.ob0 + j; }

}  // namespace myyuv_downscale

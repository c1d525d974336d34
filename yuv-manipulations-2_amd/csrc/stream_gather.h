// stream_gather.h — crop and join of DCTYUV streams on their chunk bytes
// (include/myyuv_hip.h, "Crop and join"): the run map k_gather_sizes and
// k_stream_gather walk, and a host gather that does a whole crop or join on
// host buffers with the same map (tools/stream_gather_host.cpp; the CPU
// implementation the tests compare against).  Plain C++: no HIP types.
//
// Both operations are one map.  The output frame is a grid of cols x rows
// pieces of tbw x tbh blocks (per plane); piece (tx, ty) comes from source
// stream ty * cols + tx, from the rectangle of tbw x tbh blocks whose first
// block is (bx, by) of a source plane sbw blocks wide:
//   crop: one piece (cols = rows = 1), (bx, by) the rectangle's corner;
//   join: bx = by = 0, sbw = tbw: the whole tile.
// A run is a maximal set of at most kRun output blocks of one output row of
// one plane that come from one source stream: consecutive blocks in the
// source plane and in the destination's, so one contiguous byte range of the
// content on both sides.  Runs are numbered plane-major, row-major, left to
// right (as RegionSegs numbers segments): an output row splits at the pieces'
// borders, each piece row every kRun blocks.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MYYUV_GATHER_HD __host__ __device__ __forceinline__
#else
#define MYYUV_GATHER_HD inline
#endif

namespace myyuv_gather {

constexpr uint32_t kRun = 64;

struct GatherMap {
  uint32_t cols, rows;  // pieces per output row / column
  uint32_t sbw[3];      // source plane: blocks per row
  uint32_t bx[3], by[3];  // the piece's first block column / row in the source plane
  uint32_t tbw[3], tbh[3];  // piece size in blocks
  uint32_t rpp[3];      // runs per piece row: ceil(tbw / kRun)
  uint32_t rcum[4];     // runs, cumulative per plane
  uint32_t scum[4];     // source frame's blocks, cumulative per plane
  uint32_t dcum[4];     // output frame's blocks, cumulative per plane
};

struct Run {
  uint32_t plane;
  uint32_t dst;     // first block inside the output plane
  uint32_t stream;  // source stream (tile) index
  uint32_t src;     // first block inside the source plane
  uint32_t n;       // blocks, 1..kRun
};

// The map of a crop (rx, ry, rw, rh) of a w x h frame: all in luma pixels,
// multiples of 16 (the caller has checked the rectangle).
MYYUV_GATHER_HD GatherMap crop_map(uint32_t w, uint32_t h, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh) {
  GatherMap M{};
  M.cols = M.rows = 1;
  for (int p = 0; p < 3; p++) {
    const uint32_t sh = p ? 4 : 3;  // log2 of the plane's block size in luma pixels
    M.sbw[p] = w >> sh;
    M.bx[p] = rx >> sh;
    M.by[p] = ry >> sh;
    M.tbw[p] = rw >> sh;
    M.tbh[p] = rh >> sh;
    M.rpp[p] = (M.tbw[p] + kRun - 1) / kRun;
    M.rcum[p + 1] = M.rcum[p] + M.rpp[p] * M.tbh[p];
    M.scum[p + 1] = M.scum[p] + M.sbw[p] * (h >> sh);
    M.dcum[p + 1] = M.dcum[p] + M.tbw[p] * M.tbh[p];
  }
  return M;
}

// The map of a join of cols x rows tiles of tw x th luma pixels (multiples of
// 16; the caller has checked the grid and the output frame's size).
MYYUV_GATHER_HD GatherMap join_map(uint32_t cols, uint32_t rows, uint32_t tw, uint32_t th) {
  GatherMap M{};
  M.cols = cols;
  M.rows = rows;
  for (int p = 0; p < 3; p++) {
    const uint32_t sh = p ? 4 : 3;
    M.sbw[p] = M.tbw[p] = tw >> sh;
    M.tbh[p] = th >> sh;
    M.rpp[p] = (M.tbw[p] + kRun - 1) / kRun;
    M.rcum[p + 1] = M.rcum[p] + M.rpp[p] * cols * M.tbh[p] * rows;
    M.scum[p + 1] = M.scum[p] + M.tbw[p] * M.tbh[p];
    M.dcum[p + 1] = M.dcum[p] + M.tbw[p] * M.tbh[p] * cols * rows;
  }
  return M;
}

// Run r of the map (r < rcum[3]).
MYYUV_GATHER_HD Run run_at(const GatherMap& M, uint32_t r) {
  const int p = r >= M.rcum[1] ? (r >= M.rcum[2] ? 2 : 1) : 0;
  // (static indices: the map is a kernel argument)
  const uint32_t rc = p == 0 ? 0u : (p == 1 ? M.rcum[1] : M.rcum[2]);
  const uint32_t rpp = p == 0 ? M.rpp[0] : (p == 1 ? M.rpp[1] : M.rpp[2]);
  const uint32_t tbw = p == 0 ? M.tbw[0] : (p == 1 ? M.tbw[1] : M.tbw[2]);
  const uint32_t tbh = p == 0 ? M.tbh[0] : (p == 1 ? M.tbh[1] : M.tbh[2]);
  const uint32_t sbw = p == 0 ? M.sbw[0] : (p == 1 ? M.sbw[1] : M.sbw[2]);
  const uint32_t bx = p == 0 ? M.bx[0] : (p == 1 ? M.bx[1] : M.bx[2]);
  const uint32_t by = p == 0 ? M.by[0] : (p == 1 ? M.by[1] : M.by[2]);
  const uint32_t rr = r - rc;
  const uint32_t rpr = rpp * M.cols;  // runs per output row
  const uint32_t row = rr / rpr, k = rr - row * rpr;
  const uint32_t tx = k / rpp, seg = k - tx * rpp;
  const uint32_t ty = row / tbh, ly = row - ty * tbh;
  const uint32_t lx = seg * kRun;
  Run R;
  R.plane = (uint32_t)p;
  R.dst = row * (tbw * M.cols) + tx * tbw + lx;
  R.stream = ty * M.cols + tx;
  R.src = (by + ly) * sbw + bx + lx;
  R.n = tbw - lx < kRun ? tbw - lx : kRun;
  return R;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host gather --------------------------------------------------------
// Error codes are MYYUV_E_* of include/myyuv_hip.h (numbers only: this header
// stands alone).
struct HostStream {
  uint32_t sizes_pos[3], content_pos[3], content_size[3];
};

inline uint32_t rd32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
inline void wr32(uint8_t* p, uint32_t v) {
  for (int k = 0; k < 4; k++) p[k] = (uint8_t)(v >> (8 * k));
}

// The stream header checks of myyuv_gpu_dct_decompress's step 2 (parse_stream,
// k_chain.hpp, in its order), the block counts against the source geometry.
inline int parse_host(const uint8_t* in, uint32_t size, const uint32_t scum[4], HostStream& S) {
  if (size <= 12) return 6;
  const uint32_t ps[3] = {rd32(in), rd32(in + 4), rd32(in + 8)};
  if (12ull + ps[0] + ps[1] + ps[2] > size) return 6;
  uint64_t off = 12;
  uint32_t hn[3];
  for (int p = 0; p < 3; p++) {
    if (ps[p] <= 8) return 7;
    hn[p] = rd32(in + off);
    const uint32_t hc = rd32(in + off + 4);
    if (hn[p] == 0) return 8;
    if (hc == 0) return 9;
    if (8ull + hn[p] + hc > ps[p]) return 7;
    S.sizes_pos[p] = (uint32_t)(off + 8);
    S.content_pos[p] = (uint32_t)(off + 8 + hn[p]);
    S.content_size[p] = hc;
    off += ps[p];
  }
  for (int p = 0; p < 3; p++)
    if (hn[p] < scum[p + 1] - scum[p]) return 8;
  return 0;
}

// A whole crop or join on host buffers: srcs[t] / sizes[t] for the cols * rows
// source streams -> `out` (capacity cap), *out_size the size needed.  Returns
// 0 or the code; *bad_block as the C ABI reports it (-1: none).  `off` is
// scratch for the source streams' chunk offsets: scum[3] + 1 words.
inline int gather_host(const GatherMap& M, const uint8_t* const* srcs, const uint32_t* sizes, uint8_t* out,
                       uint32_t cap, uint32_t* out_size, int64_t* bad_block, uint32_t* off) {
  *bad_block = -1;
  const uint32_t nsrc = M.cols * M.rows;
  for (uint32_t t = 0; t < nsrc; t++) {
    HostStream S;
    if (const int code = parse_host(srcs[t], sizes[t], M.scum, S)) {
      *bad_block = t ? (int64_t)t * M.scum[3] : -1;
      return code;
    }
  }
  // pass 1: the output planes' content sizes and the plane-content check
  // (lowest key: source stream, then plane); pass 2: the bytes
  uint64_t content[3] = {0, 0, 0};
  int code = 0;
  uint64_t key = ~0ull;
  for (int pass = 0; pass < 2; pass++) {
    uint64_t ppos[3], total = 0;  // the output planes' header positions
    if (pass == 1) {
      uint64_t pos = 12;
      for (int p = 0; p < 3; p++) {
        ppos[p] = pos;
        pos += 8ull + (M.dcum[p + 1] - M.dcum[p]) + content[p];
      }
      total = pos;
      *out_size = (uint32_t)total;
      if (code) {
        *bad_block = key ? (int64_t)key : -1;
        return code;
      }
      if (total > cap) return 5;
      for (int p = 0; p < 3; p++) {
        const uint32_t nb = M.dcum[p + 1] - M.dcum[p];
        wr32(out + 4 * p, (uint32_t)(8 + nb + content[p]));
        wr32(out + ppos[p], nb);
        wr32(out + ppos[p] + 4, (uint32_t)content[p]);
      }
    }
    uint64_t dpos[3] = {0, 0, 0};  // bytes of plane p's output content so far
    uint32_t cached = ~0u;
    HostStream S{};
    for (uint32_t r = 0; r < M.rcum[3]; r++) {
      const Run R = run_at(M, r);
      const int p = (int)R.plane;
      const uint8_t* in = srcs[R.stream];
      if (cached != R.stream) {  // the stream's chunk offsets, plane by plane
        (void)parse_host(in, sizes[R.stream], M.scum, S);
        for (int q = 0; q < 3; q++) {
          uint32_t acc = 0;
          for (uint32_t g = M.scum[q]; g < M.scum[q + 1]; g++) {
            off[g] = acc;
            acc += in[S.sizes_pos[q] + (g - M.scum[q])];
          }
        }
        cached = R.stream;
      }
      uint32_t bytes = 0;
      for (uint32_t i = 0; i < R.n; i++) bytes += in[S.sizes_pos[p] + R.src + i];
      const uint32_t start = off[M.scum[p] + R.src];
      if (pass == 0) {
        content[p] += bytes;
        if ((uint64_t)start + bytes > S.content_size[p]) {
          const uint64_t k = (uint64_t)R.stream * M.scum[3] + M.scum[p];
          if (k < key) key = k, code = 9;
        }
      } else {
        uint8_t* so = out + ppos[p] + 8 + R.dst;
        for (uint32_t i = 0; i < R.n; i++) so[i] = in[S.sizes_pos[p] + R.src + i];
        uint8_t* co = out + ppos[p] + 8 + (M.dcum[p + 1] - M.dcum[p]) + dpos[p];
        const uint8_t* ci = in + S.content_pos[p] + start;
        for (uint32_t i = 0; i < bytes; i++) co[i] = ci[i];
      }
      dpos[p] += bytes;
    }
  }
  return 0;
}
#endif  // host

}  // namespace myyuv_gather

// k_metric.hpp — what the Compare kernels share on the device
// (k_decode_compare, k_huff_decode.hip; k_frame_compare, k_color.hip;
// k_coef_compare, k_transform.hip): the
// exchanges that bring a block's partial sums together, and the wave's last
// step, one lane per block (metric.h has the arithmetic).
#pragma once
#include "codec_common.hpp"
#include "metric.h"
#include "myyuv_hip.h"

namespace myyuv_gpu {
namespace mt {

using myyuv_metric::Sums;

// Sums over aligned groups of 4 or 8 lanes (a block's lanes in a 16-block or an
// 8-block transform unit), every lane of the group left with the total: DPP
// quad_perm [1, 0, 3, 2] and [2, 3, 0, 1], then row_half_mirror, which after
// the two quad steps swaps the totals of an 8-lane group's two quads.  The
// whole wave must be active (the DPP rule).
template <int kCtrl>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, kCtrl, 0xF, 0xF, false);
}
template <int kCtrl>
__device__ __forceinline__ void fold(Sums& s) {
  Sums o;
  o.sx = dpp<kCtrl>(s.sx);
  o.sy = dpp<kCtrl>(s.sy);
  o.sxx = dpp<kCtrl>(s.sxx);
  o.syy = dpp<kCtrl>(s.syy);
  o.sxy = dpp<kCtrl>(s.sxy);
  o.mx = dpp<kCtrl>(s.mx);
  myyuv_metric::add(s, o);
}
template <int kLanes>
__device__ __forceinline__ void fold_lanes(Sums& s) {
  static_assert(kLanes == 4 || kLanes == 8, "a block's lanes in a transform unit");
  fold<0xB1>(s);
  fold<0x4E>(s);
  if (kLanes == 8) fold<0x141>(s);
}

// The wave's last step.  Lane l holds the sums of its own block (`live`: it has
// one; all 64 lanes call this).  Each live lane evaluates its block's sse and
// ssim and writes the map entry `entry` (nullptr: no map); the wave's totals go
// to its own slot `part` (sse, ssim, blocks, max), which k_metric_reduce adds up
// per plane.  (Atomic adds from every wave straight into the plane's record
// measured 1.08 ms for the 24,576 waves of an 8192x8192 frame, ten times the
// decode: they all meet in one cache line.  DESIGN.md §4, "Compare".)  A wave
// holds at most 64 blocks: its sse total is below 2^29 and its ssim total
// within +-2^30.
__device__ __forceinline__ void finish(const Sums& s, bool live, uint4* part, myyuv_block_metric* entry) {
  uint32_t sse = 0, mx = 0;
  int32_t ss = 0;
  if (live) {
    sse = myyuv_metric::sse_of(s);
    ss = myyuv_metric::ssim_of(s);
    mx = s.mx;
    if (entry != nullptr) *reinterpret_cast<uint2*>(entry) = make_uint2(sse, (uint32_t)ss);
  }
  const uint32_t n = (uint32_t)__popcll(__ballot(live));
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sse += (uint32_t)__shfl_xor((int)sse, m, 64);
    ss += __shfl_xor(ss, m, 64);
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, m, 64));
  }
  if (threadIdx.x % kWave == 0) *part = make_uint4(sse, (uint32_t)ss, n, mx);
}

// finish() for a wave that holds four 16-block transform units at once
// (k_coef_compare, k_transform.hip): lane (b, q) holds block b of the wave's
// unit q (`live`: it has one; `unit`: the wave has a unit q at all; all 64
// lanes call this).  The totals are taken over the lanes of equal q, and lane
// q < 4 writes unit q's slot `part` (the slot of the lane's own unit), so each
// unit's totals stay apart: the units of a wave may lie in different planes
// and frames.  A unit's sse total is below 2^26.
__device__ __forceinline__ void finish_units(const Sums& s, bool live, bool unit, uint4* part,
                                             myyuv_block_metric* entry) {
  uint32_t sse = 0, mx = 0, n = 0;
  int32_t ss = 0;
  if (live) {
    sse = myyuv_metric::sse_of(s);
    ss = myyuv_metric::ssim_of(s);
    mx = s.mx;
    n = 1;
    if (entry != nullptr) *reinterpret_cast<uint2*>(entry) = make_uint2(sse, (uint32_t)ss);
  }
#pragma unroll
  for (int m = 32; m >= 4; m >>= 1) {
    sse += (uint32_t)__shfl_xor((int)sse, m, 64);
    ss += __shfl_xor(ss, m, 64);
    n += (uint32_t)__shfl_xor((int)n, m, 64);
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, m, 64));
  }
  if (threadIdx.x % kWave < 4u && unit) *part = make_uint4(sse, (uint32_t)ss, n, mx);
}

// The slot of the wave of group (blockIdx.x) of frame (blockIdx.y) on the
// decoders' grid.
__device__ __forceinline__ uint4* wave_slot(uint4* part) {
  return part + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
}

}  // namespace mt
}  // namespace myyuv_gpu

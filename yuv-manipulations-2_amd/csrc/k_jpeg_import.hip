// k_jpeg_import.hip — the front of the JPEG import (include/myyuv_hip.h,
// "Import from JPEG"): a baseline Huffman decoder on gfx950 that leaves K1's
// hand-off (coefficient quads, row masks, block info words) for K2, as
// k_requant does.  The block decoder, the bit source and the MCU map are
// jpeg_import.h's, shared with the host.
//
// k_jpeg_import: one lane per restart interval, one wave per 64 consecutive
// entries of the segment table (jpeg_import.h inspect).  A lane walks its
// interval's MCUs; for every block it zeroes its column of a 64 x int16 block
// image in LDS (8 KiB per wave: the zig-zag index is dynamic, so the block
// cannot sit in registers), decodes into it, reads the 32 natural-order words
// back with static indices, rescales the nonzero rows when the plane's table
// is not the destination's (requant.h) and writes the hand-off
// (requant_handoff, huff_common.hpp).  A lane's column is its own: no barrier
// after the tables are staged.  A failing block is reported with its index
// (the lowest wins, as in the decoders) and it and the rest of its interval
// are handed over all-zero, so K2 never reads what the workspace held.
// Blocks no scan covers (non-interleaved scans of a picture whose last MCU
// column or row is half empty) are zeroed by the host before the launch.
// Reads: aligned words of the file inside the interval's bytes rounded to 4;
// writes: block indices below cum[3] only (checked per block).
//
// k_jpeg_import_coef: the same hand-off from a coefficient image (int16
// [blocks][64], natural order, the stream's block order) that the host
// decoded: one lane per block, the wave's 8 KiB read as 16-B quads in address
// order and turned through LDS.
#include "codec_common.hpp"
#include "huff_common.hpp"
#include "jpeg_import.h"
#include "requant.h"

namespace myyuv_gpu {

namespace {

typedef uint32_t __attribute__((may_alias)) u32_alias;
typedef uint16_t __attribute__((may_alias)) u16_alias;

struct DevWords {
  const uint32_t* p;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return p[i]; }
};

}  // namespace

__global__ __launch_bounds__(64) void k_jpeg_import(const uint32_t* __restrict__ file,
                                                    const myyuv_jpegin::Seg* __restrict__ segs, uint32_t nseg,
                                                    myyuv_jpegin::Plan P,
                                                    const myyuv_jpegin::DecTab* __restrict__ tabs,
                                                    const RequantTables* __restrict__ rt, uint32_t rescale_mask,
                                                    uint4* __restrict__ coef, uint8_t* __restrict__ rmask,
                                                    uint32_t* __restrict__ binfo,
                                                    unsigned long long* __restrict__ err) {
  using namespace myyuv_jpegin;
  __shared__ uint32_t blk[32 * 64];  // word w of lane l's block: blk[w * 64 + l]
  __shared__ DecTab stab[6];         // dc[3], ac[3] by plane
  __shared__ RequantTables sq;
  __shared__ uint8_t szz[64];        // kZigzag
  const uint32_t lane = threadIdx.x;
  szz[lane] = myyuv_jpeg::kZigzag[lane];
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tabs);
    u32_alias* dst = reinterpret_cast<u32_alias*>(stab);
    for (uint32_t i = lane; i < sizeof(stab) / 4; i += 64) dst[i] = src[i];
    src = reinterpret_cast<const uint32_t*>(rt);
    dst = reinterpret_cast<u32_alias*>(&sq);
    for (uint32_t i = lane; i < sizeof(RequantTables) / 4; i += 64) dst[i] = src[i];
  }
  __syncthreads();
  const uint32_t si = blockIdx.x * 64 + lane;
  if (si >= nseg) return;
  const Seg S = segs[si];
  if (S.scan >= 3) return;
  BitSrc<DevWords> src(DevWords{file}, S.off, S.len);
  u32_alias* col32 = reinterpret_cast<u32_alias*>(blk) + lane;
  u16_alias* col16 = reinterpret_cast<u16_alias*>(blk) + 2 * lane;
  const uint32_t nb = P.ns[S.scan] == 3 ? 6u : 1u;
  int pred[3] = {0, 0, 0};
  bool ok = true;
  for (uint32_t m = S.mcu0; m < S.mcu0 + S.nmcu; m++) {
    for (uint32_t j = 0; j < nb; j++) {
      uint32_t p;
      const uint32_t g = block_of_mcu(P, S.scan, m, j, p);
      if (p > 2 || g >= P.cum[3]) return;  // (no table the host built names such a block)
      if (!ok) {  // the rest of a failed interval: all-zero blocks
        rmask[g] = 0;
        binfo[g] = binfo_word(0u, 0u, kClassSingle, 0u);
        continue;
      }
#pragma unroll
      for (int w = 0; w < 32; w++) col32[w * 64] = 0u;
      int pr = p == 0 ? pred[0] : (p == 1 ? pred[1] : pred[2]);
      const int bad = decode_block(src, stab[p], stab[3 + p], pr, [&](uint32_t nat, int v) {
        col16[(nat >> 1) * 128u + (nat & 1u)] = (uint16_t)v;
      }, [&](uint32_t k) { return (uint32_t)szz[k]; });
      if (p == 0) pred[0] = pr;
      else if (p == 1) pred[1] = pr;
      else pred[2] = pr;
      CoefRegs R;
#pragma unroll
      for (int w = 0; w < 32; w++) R.w[w] = bad ? 0u : col32[w * 64];
      if (bad) {
        ok = false;
        atomicMin(err, (unsigned long long)(((2ull * g + 1) << 8) | (unsigned)kData));
      }
      requant_handoff(R, g, ((rescale_mask >> p) & 1u) != 0, sq.qs[p], sq.qd[p], coef, rmask, binfo);
    }
  }
}

__global__ __launch_bounds__(64) void k_jpeg_import_coef(const uint4* __restrict__ img, uint32_t nblk,
                                                         uint32_t cum1, uint32_t cum2,
                                                         const RequantTables* __restrict__ rt,
                                                         uint32_t rescale_mask, uint4* __restrict__ coef,
                                                         uint8_t* __restrict__ rmask,
                                                         uint32_t* __restrict__ binfo) {
  __shared__ uint4 st[8 * 64];  // quad c of the wave's block b: st[c * 64 + b]
  __shared__ RequantTables sq;
  const uint32_t lane = threadIdx.x;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(rt);
    u32_alias* dst = reinterpret_cast<u32_alias*>(&sq);
    for (uint32_t i = lane; i < sizeof(RequantTables) / 4; i += 64) dst[i] = src[i];
  }
#pragma unroll
  for (uint32_t i = 0; i < 8; i++) {
    const uint32_t q = i * 64 + lane;
    const uint64_t gq = (uint64_t)blockIdx.x * 512 + q;
    st[(q & 7u) * 64 + (q >> 3)] = gq < (uint64_t)nblk * 8 ? img[gq] : make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  const uint32_t g = blockIdx.x * 64 + lane;
  if (g >= nblk) return;
  CoefRegs R;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const uint4 v = st[c * 64 + lane];
    R.w[4 * c] = v.x;
    R.w[4 * c + 1] = v.y;
    R.w[4 * c + 2] = v.z;
    R.w[4 * c + 3] = v.w;
  }
  const uint32_t p = g >= cum1 ? (g >= cum2 ? 2u : 1u) : 0u;
  requant_handoff(R, g, ((rescale_mask >> p) & 1u) != 0, sq.qs[p], sq.qd[p], coef, rmask, binfo);
}

}  // namespace myyuv_gpu

// k1_store.hpp — K1's hand-off to K2 (the block's nonzero rows as natural-order
// quads, its row mask and its info word), shared by k_transform.hip (K1,
// k_fdct_fix) and the downscaler (k_huff_decode.hip, k_downscale), which runs
// K1's per-unit forward transform on blocks it has just decoded.
#pragma once
#include "codec_common.hpp"
#include "xform_common.hpp"

namespace myyuv_gpu {
namespace xf {

typedef unsigned short k1_us2 __attribute__((ext_vector_type(2)));

// Rows q, q + 4 of lane (b, q)'s block (coefficient quads q, q + 4), the
// block's row mask (bit c: row c has a nonzero coefficient, from the block's
// four lanes) and its K2 info word (binfo_word: row mask, msz, class, DC),
// which lets K2 classify its blocks from 4 B each instead of their rows.  An
// all-zero row is not stored (K2 reads masked-off rows from a zero buffer),
// which saves most of the 128 B per block of a q=50 frame twice (this write,
// K2's read).  Every lane still issues its four stores (the sink takes the
// skipped ones and those of lanes past the plane's end).  szz: the (zig-zag
// index + 1) pairs, kZzPairs (quad r: row r's four pairs).  kHiZero
// (wave-uniform, fdct_fast): rows 4..7 of the wave's blocks are zero, so the
// hi quad's packing, its counts and its store are left out.
template <bool kHiZero = false>
__device__ __forceinline__ void store_block_rows(const uint32_t (&c)[16], uint32_t q, uint32_t lane, bool live,
                                                 uint32_t g, uint4* dlo, uint4* dhi, uint8_t* __restrict__ rmask,
                                                 uint32_t* __restrict__ binfo, const uint4* szz,
                                                 uint4* __restrict__ sink) {
  uint4 lo, hi;
  uint32_t rm;
  pack_quads<kHiZero>(c, q, lo, hi, rm);
  // nonzero count and msz of the lane's natural pairs (lo: row q, hi: row
  // q + 4) in packed 16-bit arithmetic, as K2's block_class_msz:
  // flag = min(v, 1) per half, count += flag, max of (0 - flag) & (index + 1)
  const uint4 z0 = szz[q], z1 = szz[kHiZero ? q : q + 4];
  const uint32_t wv[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const uint32_t zv[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
  k1_us2 cnt = {0, 0}, mx = {0, 0};
#pragma unroll
  for (int i = 0; i < (kHiZero ? 4 : 8); i++) {
    uint32_t fu, m16;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(fu) : "v"(wv[i]), "s"(0x00010001u));
    cnt += __builtin_bit_cast(k1_us2, fu);
    // flag * (index + 1): the indices are VGPRs here, so the packed multiply takes them
    asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(m16) : "v"(fu), "v"(zv[i]));
    mx = __builtin_elementwise_max(mx, __builtin_bit_cast(k1_us2, m16));
  }
  // the block's four lanes: counts add, msz is the maximum (one shuffle per
  // step carries both)
  uint32_t nnz = (uint32_t)cnt.x + (uint32_t)cnt.y;
  uint32_t msz = mx.x > mx.y ? (uint32_t)mx.x : (uint32_t)mx.y;
#pragma unroll
  for (int d = 1; d < 4; d <<= 1) {
    const uint32_t o = d == 1 ? quad_xor1(nnz | (msz << 16)) : quad_xor2(nnz | (msz << 16));
    nnz += o & 0xFFFFu;
    msz = max(msz, o >> 16);
  }
  const bool nzl = (rm >> q) & 1u, nzh = (rm >> (q + 4)) & 1u;
  *(live ? rmask + g : reinterpret_cast<uint8_t*>(sink + 128) + lane) = (uint8_t)rm;
  // the block's four lanes store the same word (lane 4b holds row 0: the DC
  // is the low half of its lo.x)
  const uint32_t dc = quad_lane0(lo.x);
  *(live ? binfo + g : reinterpret_cast<uint32_t*>(sink + 132) + lane) = binfo_word(rm, msz, class_of(nnz, msz), dc);
  *(nzl ? dlo : sink + lane) = lo;
  if (!kHiZero) *(nzh ? dhi : sink + 64 + lane) = hi;
}

// K1's stores as buffer stores (1; 0: flat stores with per-lane pointers):
// 32-bit offsets from wave-uniform descriptors, and a store that must not
// happen (a zero row, a lane past the plane's end, a block left to the exact
// path) gets an offset past the descriptor's range, which the hardware drops.
// The flat form selects a sink pointer per store instead: two 64-bit selects
// and a 64-bit add, each a VOP3 instruction (half the issue rate of the VOP2
// forms on gfx950, tools/ubench/iforms.hip).  The launch's coefficient image
// must stay below 4 GiB (make_geom / the batch split guarantee it).
#ifndef MYYUV_K1_BUF
#define MYYUV_K1_BUF 1
#endif
typedef unsigned int k1_v4u __attribute__((ext_vector_type(4)));
constexpr uint32_t kOob = 0xFFFFFFFFu;  // a buffer offset past every range: the store is dropped

struct K1Rsrc {
  __amdgpu_buffer_rsrc_t coef, rmask, binfo;
};
// descriptors of the launch's coefficient image, row masks and block words
// (from kernel arguments only: wave-uniform)
__device__ __forceinline__ K1Rsrc k1_rsrc(uint4* coef, uint8_t* rmask, uint32_t* binfo, const FrameGeom& G) {
  const uint32_t nblk = G.cum[3] * G.nframes;
  K1Rsrc r;
  r.coef = __builtin_amdgcn_make_buffer_rsrc(coef, 0, (int)(((nblk + 63u) / 64u) * (kCoefQuadsPerWave * 16u)),
                                             0x00020000);
  r.rmask = __builtin_amdgcn_make_buffer_rsrc(rmask, 0, (int)nblk, 0x00020000);
  r.binfo = __builtin_amdgcn_make_buffer_rsrc(binfo, 0, (int)(nblk * 4u), 0x00020000);
  return r;
}

// store_block_rows through the descriptors: the same bytes, the skipped
// stores dropped by an out-of-range offset instead of a sink
template <bool kHiZero = false>
__device__ __forceinline__ void store_block_rows_buf(const uint32_t (&c)[16], uint32_t q, bool live, uint32_t g,
                                                     const K1Rsrc& R, const uint4* szz) {
  uint4 lo, hi;
  uint32_t rm;
  pack_quads<kHiZero>(c, q, lo, hi, rm);
  const uint4 z0 = szz[q], z1 = szz[kHiZero ? q : q + 4];
  const uint32_t wv[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const uint32_t zv[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
  k1_us2 cnt = {0, 0}, mx = {0, 0};
#pragma unroll
  for (int i = 0; i < (kHiZero ? 4 : 8); i++) {
    uint32_t fu, m16;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(fu) : "v"(wv[i]), "s"(0x00010001u));
    cnt += __builtin_bit_cast(k1_us2, fu);
    asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(m16) : "v"(fu), "v"(zv[i]));
    mx = __builtin_elementwise_max(mx, __builtin_bit_cast(k1_us2, m16));
  }
  uint32_t nnz = (uint32_t)cnt.x + (uint32_t)cnt.y;
  uint32_t msz = mx.x > mx.y ? (uint32_t)mx.x : (uint32_t)mx.y;
#pragma unroll
  for (int d = 1; d < 4; d <<= 1) {
    const uint32_t o = d == 1 ? quad_xor1(nnz | (msz << 16)) : quad_xor2(nnz | (msz << 16));
    nnz += o & 0xFFFFu;
    msz = max(msz, o >> 16);
  }
  const bool nzl = (rm >> q) & 1u, nzh = (rm >> (q + 4)) & 1u;
  const uint32_t dc = quad_lane0(lo.x);
  __builtin_amdgcn_raw_buffer_store_b8((uint8_t)rm, R.rmask, live ? g : kOob, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b32(binfo_word(rm, msz, class_of(nnz, msz), dc), R.binfo, live ? 4u * g : kOob,
                                        0, 0);
  const uint32_t qo = coef_quad(g, q) * 16u;  // quad q + 4 is 4 * 64 quads further
  __builtin_amdgcn_raw_buffer_store_b128(k1_v4u{lo.x, lo.y, lo.z, lo.w}, R.coef, live && nzl ? qo : kOob, 0, 0);
  if (!kHiZero)
    __builtin_amdgcn_raw_buffer_store_b128(k1_v4u{hi.x, hi.y, hi.z, hi.w}, R.coef, live && nzh ? qo + 4096u : kOob, 0,
                                           0);
}

// The zig-zag pair table in LDS (kZzPairs; before the tables' barrier)
__device__ __forceinline__ void stage_zz(uint4* szz) {
  if (threadIdx.x < 32) reinterpret_cast<uint32_t*>(szz)[threadIdx.x] = kZzPairs.v[threadIdx.x];
}

}  // namespace xf
}  // namespace myyuv_gpu

// color_px.hpp — BMP -> IYUV's per-pixel arithmetic and its 4-pixel loads,
// shared by K7 (k_color.hip, k_bmp_to_iyuv) and compress-from-BMP
// (k_transform.hip, k_bmp_fdct), so both compile the same expressions.  The
// numerics are described at the head of k_color.hip; both files are built with
// -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace myyuv_gpu {
namespace px {

__device__ __forceinline__ uint32_t trunc_u8(float x) { return (uint32_t)(int32_t)x & 0xFFu; }

// getYUV444FromRGB2x2's per-pixel step; returns Y and the two chroma values
// already divided by 4 with round-to-nearest (divide_roundnearest(c, 4)).
__device__ __forceinline__ void pixel(uint32_t b, uint32_t g, uint32_t r, uint32_t& y,
                                      uint32_t& cb4, uint32_t& cr4) {
  const float B = (float)b, G = (float)g, R = (float)r;
  const float Y = 0.299f * R + 0.587f * G + 0.114f * B;
  y = trunc_u8(Y);
  cb4 = (((trunc_u8((B - Y) * 0.564f) + 128u) & 0xFFu) + 2u) >> 2;
  cr4 = (((trunc_u8((R - Y) * 0.713f) + 128u) & 0xFFu) + 2u) >> 2;
}

// byte k of a little-endian word array (k static after unrolling)
template <int N>
__device__ __forceinline__ uint32_t byte_at(const uint32_t (&w)[N], int k) {
  return (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
}

// Four consecutive source pixels starting at pixel index `pix` (pix % 4 == 0).
template <int BPP>
__device__ __forceinline__ void load4(const uint8_t* __restrict__ src, size_t pix,
                                      uint32_t (&w)[BPP]) {
  const uint32_t* p = reinterpret_cast<const uint32_t*>(src + pix * BPP);
  if constexpr (BPP == 4) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
#pragma unroll
    for (int i = 0; i < BPP; i++) w[i] = p[i];
  }
}

// One row of a 4 x 2 tile from its four source pixels w (in reverse order when
// rev, colorData's width < 0): the row's luma dword, and the pixels' chroma
// quarters added to the tile's two 2 x 2 quads.
template <int BPP>
__device__ __forceinline__ void tile_row(const uint32_t (&w)[BPP], bool rev, uint32_t& Y, uint32_t (&cb)[2],
                                         uint32_t (&cr)[2]) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    uint32_t b, g, rr;
    if (rev) {  // uniform branch: both orders keep static byte indices
      b = byte_at(w, (3 - k) * BPP), g = byte_at(w, (3 - k) * BPP + 1), rr = byte_at(w, (3 - k) * BPP + 2);
    } else {
      b = byte_at(w, k * BPP), g = byte_at(w, k * BPP + 1), rr = byte_at(w, k * BPP + 2);
    }
    uint32_t y, cb4, cr4;
    pixel(b, g, rr, y, cb4, cr4);
    Y |= y << (8 * k);
    cb[k >> 1] += cb4;
    cr[k >> 1] += cr4;
  }
}

}  // namespace px
}  // namespace myyuv_gpu

// bmp_fdct.h — the work map of compress-from-BMP (include/myyuv_hip.h,
// "Compress from BMP"): which wave converts which pixels, where they land in
// the wave's image of block pictures, and which blocks of the frame the wave
// then transforms.  Shared by the gfx950 kernel (k_transform.hip k_bmp_fdct)
// and the host program tools/bmp_fdct_host.cpp
// (tests/test_bmp_compress_host.py), so the map exists once.  Plain C++, no
// HIP types.
//
// A STRIP is 16 pixel rows by up to kStripCols = 256 columns of the frame
// (top-down, as colorData presents it): up to 16 macroblocks of 16 x 16, each
// four Y blocks, one U and one V block.  W is a multiple of 16, so a narrower
// last strip of a strip row still holds whole macroblocks.  Wave s of a frame
// owns strip s (strip rows top to bottom, strips left to right).
//
// Conversion: lane l takes the 4 x 2 tiles of tile column l of the strip
// (pixel columns 4l .. 4l+3), tile rows ty = 0 .. 7, so consecutive lanes read
// consecutive 16-B (12-B) pieces of a pixel row; lanes from ncols / 4 on have
// no tile.  colorData's orientation is folded into the source offset.
//
// Image: kSlots block pictures, each 8 rows of 8 bytes (what fdct_load reads)
// at a stride of kSlotBytes = 72 bytes: 18 dwords, so the luma dword stores of
// a tile row (lanes 2j, 2j+1 in slot j) and the 16-block units' reads fall on
// distinct banks (a 64-byte stride puts lanes l and l + 8 on one bank).  Y
// blocks take slots 0 .. 4 nmb - 1, block row major inside the strip (so the
// live blocks of a narrow strip fill the fewest units), U blocks slots
// kSlotU .. kSlotU + nmb - 1, V blocks kSlotV .. kSlotV + nmb - 1.
//
// Transform: units of 16 consecutive slots of one plane: ceil(nmb / 4) Y
// units, one U, one V.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MYYUV_BMPF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MYYUV_BMPF_HD static inline
#endif

namespace myyuv_bmpfdct {

constexpr uint32_t kStripCols = 256, kStripRows = 16;
constexpr uint32_t kTileRows = kStripRows / 2;  // 4 x 2 tiles per lane
constexpr uint32_t kSlotBytes = 72;
constexpr uint32_t kSlotU = 64, kSlotV = 80, kSlots = 96;
constexpr uint32_t kUnit = 16;  // blocks per transform unit (kXfUnit)

// A |w| x |h| frame (multiples of 16) in orientation `orient` (0: rows as
// stored, 1: pixel order reversed, 2: rows bottom-up: BMP::colorData's cases).
struct Map {
  uint32_t w, h, orient;
  uint32_t spr;     // strips per strip row
  uint32_t nstrips;
};

MYYUV_BMPF_HD Map make_map(uint32_t w, uint32_t h, uint32_t orient) {
  Map M;
  M.w = w;
  M.h = h;
  M.orient = orient;
  M.spr = (w + kStripCols - 1) / kStripCols;
  M.nstrips = M.spr * (h / kStripRows);
  return M;
}

// Strip s: its strip row, first pixel column, and macroblocks.
struct Strip {
  uint32_t sy, col0, nmb;
};

MYYUV_BMPF_HD Strip strip_of(const Map& M, uint32_t s) {
  Strip S;
  S.sy = s / M.spr;
  S.col0 = (s - S.sy * M.spr) * kStripCols;
  const uint32_t ncols = M.w - S.col0 < kStripCols ? M.w - S.col0 : kStripCols;
  S.nmb = ncols / 16;
  return S;
}

// Lanes with a tile column.
MYYUV_BMPF_HD uint32_t live_lanes(const Strip& S) { return S.nmb * 4; }

// The source pixel index (in the frame's pixel array as stored; times bpp / 8
// for the byte) of the four pixels of row dr (0, 1) of lane l's tile ty: they
// are source pixels base .. base + 3, in reverse order when M.orient == 1.
MYYUV_BMPF_HD uint64_t tile_src(const Map& M, const Strip& S, uint32_t l, uint32_t ty, uint32_t dr) {
  const uint64_t npx = (uint64_t)M.w * M.h;
  const uint32_t r = S.sy * kStripRows + 2 * ty + dr, c = S.col0 + 4 * l;
  const uint64_t lin = (uint64_t)r * M.w + c;  // colorData pixel index of the tile row
  if (M.orient == 0) return lin;
  if (M.orient == 1) return npx - 4 - lin;
  return (uint64_t)(M.h - 1 - r) * M.w + c;
}

// tile_src(M, S, l, ty, dr) == tile_src(M, S, l, 0, 0) + (2 ty + dr) * row_step(M):
// the next pixel row of the strip is one source row further on, or back (the
// kernel's form: one per-lane address, wave-uniform row offsets).
MYYUV_BMPF_HD int64_t row_step(const Map& M) { return M.orient == 0 ? (int64_t)M.w : -(int64_t)M.w; }

// Image byte of the luma dword of row dr of lane l's tile ty.
MYYUV_BMPF_HD uint32_t luma_byte(const Strip& S, uint32_t l, uint32_t ty, uint32_t dr) {
  const uint32_t slot = (ty >> 2) * 2 * S.nmb + (l >> 1);
  return slot * kSlotBytes + ((2 * ty + dr) & 7u) * 8 + 4 * (l & 1u);
}

// Image byte of the chroma byte pair of lane l's tile ty in the U block
// pictures (the V pair: (kSlotV - kSlotU) * kSlotBytes further).
MYYUV_BMPF_HD uint32_t chroma_byte(uint32_t l, uint32_t ty) {
  return (kSlotU + (l >> 2)) * kSlotBytes + ty * 8 + 2 * (l & 3u);
}

// Units of the strip, and unit k: its plane, first slot and live blocks.
MYYUV_BMPF_HD uint32_t units(const Strip& S) { return (S.nmb + 3) / 4 + 2; }

struct UnitOf {
  int p;
  uint32_t slot0, nlive;
};

MYYUV_BMPF_HD UnitOf unit_of(const Strip& S, uint32_t k) {
  const uint32_t nyu = (S.nmb + 3) / 4;
  UnitOf U;
  U.p = k < nyu ? 0 : (k == nyu ? 1 : 2);
  U.slot0 = k < nyu ? k * kUnit : (k == nyu ? kSlotU : kSlotV);
  const uint32_t left = 4 * S.nmb - (k < nyu ? k : 0u) * kUnit;
  U.nlive = k < nyu ? (left < kUnit ? left : kUnit) : S.nmb;
  return U;
}

// Block slot0 + b (b < nlive) of unit U: its index inside its plane of the
// frame (row-major blocks; the Y plane is w / 8 blocks wide, U and V w / 16).
MYYUV_BMPF_HD uint32_t plane_block(const Map& M, const Strip& S, const UnitOf& U, uint32_t b) {
  if (U.p == 0) {
    const uint32_t j = U.slot0 + b, by = j >= 2 * S.nmb ? 1u : 0u, bx = j - by * 2 * S.nmb;
    return (2 * S.sy + by) * (M.w / 8) + S.col0 / 8 + bx;
  }
  return S.sy * (M.w / 16) + S.col0 / 16 + b;
}

}  // namespace myyuv_bmpfdct

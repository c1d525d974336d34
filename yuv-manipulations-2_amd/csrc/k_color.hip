// k_color.hip — the colour conversions at the two ends of the pixel path:
// K7 BMP -> IYUV (below) and K8 IYUV -> BMP (further down); and, at the end,
// the two pixel-side kernels of Compare: k_frame_compare (two raw frames) and
// k_metric_reduce (the per-group totals of either compare kernel, per plane).
//
// K7: BMP (BGR / BGRA) -> IYUV 4:2:0, the step before compress
// (SURVEY.md §8f row 3).  Replaces YUV(const BMP&, IYUV): bmp_to_yuv_map[IYUV]
// (myyuv_lib/myyuv_yuv.cpp:88-128) over BMP::colorData (myyuv_bmp.cpp:77-101),
// getYUV444FromRGB2x2 (myyuv_yuv.cpp:34-52) and divide_roundnearest<uint8_t>
// (:20-27).
//
// Pure streaming: 3 or 4 B read + 1.5 B written per pixel, no reuse, so the
// bound is HBM.  A lane converts a 4x2 pixel tile (two 2x2 chroma quads):
// one 16-B (BGRA) or 12-B (BGR) load per pixel row — consecutive lanes read
// consecutive tiles, and width % 4 == 0 (BMP::isValidHeader) keeps every load
// dword aligned — then a 4-B luma store per row and a 2-B store per chroma
// plane.  colorData's re-orientation is folded into the source addressing
// (no flipped copy of the image).
//
// The per-pixel arithmetic, the 4-pixel loads and the tile-row loop are in
// color_px.hpp, shared with compress-from-BMP (k_transform.hip, k_bmp_fdct).
// Numerics are the reference x86-64 build's (checked against it and against
// the golden chef-with-trumpet.myyuv in tests/test_color.py): fp32
// Y = 0.299 R + 0.587 G + 0.114 B, products and sums left to right, no FMA
// (-ffp-contract=off); float -> uint8_t casts truncate through a 32-bit
// integer (cvttss2si) and keep the low byte (the +128 offset of a negative
// chroma value wraps through it); the 4-term chroma sum wraps mod 256, so a
// saturated-blue quad has Cb 0, as the reference's has.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "codec_common.hpp"
#include "color_div.hpp"
#include "color_px.hpp"
#include "k_metric.hpp"

namespace myyuv_gpu {

using px::load4;
using px::tile_row;

// One lane per 4x2 tile, grid-stride.  orient: 0 = rows as stored (width > 0,
// height < 0), 1 = pixel order reversed (width < 0, height > 0), 2 = rows
// bottom-up (width > 0, height > 0): the three cases of BMP::colorData.
template <int BPP>
__global__ __launch_bounds__(256) void k_bmp_to_iyuv(const uint8_t* __restrict__ src, uint32_t W,
                                                     uint32_t H, uint32_t orient,
                                                     uint8_t* __restrict__ dst) {
  const uint32_t tiles_x = W / 4;
  const uint32_t ntiles = tiles_x * (H / 2);
  const size_t npx = (size_t)W * H;
  uint8_t* __restrict__ u = dst + npx;
  uint8_t* __restrict__ v = u + npx / 4;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < ntiles; t += gridDim.x * blockDim.x) {
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    const uint32_t r = 2 * ty, c = 4 * tx;
    uint32_t Y[2] = {0, 0}, cb[2] = {0, 0}, cr[2] = {0, 0};
#pragma unroll
    for (int dr = 0; dr < 2; dr++) {
      const size_t lin = (size_t)(r + dr) * W + c;  // colorData pixel index of the tile row
      size_t base;
      if (orient == 0)
        base = lin;
      else if (orient == 1)
        base = npx - 4 - lin;  // pixels lin..lin+3 are source npx-1-lin .. npx-4-lin
      else
        base = (size_t)(H - 1 - (r + dr)) * W + c;
      uint32_t w[BPP];
      load4<BPP>(src, base, w);
      tile_row<BPP>(w, orient == 1, Y[dr], cb, cr);
    }
    *reinterpret_cast<uint32_t*>(dst + (size_t)r * W + c) = Y[0];
    *reinterpret_cast<uint32_t*>(dst + (size_t)(r + 1) * W + c) = Y[1];
    const size_t k = (size_t)ty * (W / 2) + 2 * tx;
    *reinterpret_cast<uint16_t*>(u + k) = (uint16_t)((cb[0] & 0xFFu) | (cb[1] & 0xFFu) << 8);
    *reinterpret_cast<uint16_t*>(v + k) = (uint16_t)((cr[0] & 0xFFu) | (cr[1] & 0xFFu) << 8);
  }
}

template __global__ void k_bmp_to_iyuv<3>(const uint8_t*, uint32_t, uint32_t, uint32_t, uint8_t*);
template __global__ void k_bmp_to_iyuv<4>(const uint8_t*, uint32_t, uint32_t, uint32_t, uint8_t*);

// ---- K8: IYUV -> BMP (BGR / BGRA), the inverse of K7 ------------------------
//
// The conversion the reference's viewers perform when they draw a frame
// (myyuv_opengl/viewer/frag_yuv.glsl over the plane textures of
// myyuv_opengl_shared.cpp:109-121), as a BMP pixel array.  Defined bit for
// bit in include/myyuv_hip.h (myyuv_gpu_iyuv_to_bmp): fp32, left to right, no
// FMA contraction, then the UNORM8 write floor(clamp(c, 0, 1) * 255 + 0.5).
//
// Pure streaming, 1.5 B read + 3 or 4 B written per pixel; the stores
// dominate.  K7's shape: a lane converts a 4x2 tile and writes one 16-B
// (BGRA) or 12-B (BGR) store per tile row, consecutive lanes on consecutive
// tiles of one tile row (1 KiB per wave-instruction).  A workgroup is four
// waves on four tile rows (block 64 x 4) and walks tile rows (y) and frames
// (z), so a wave's row addressing is uniform and no lane divides.  The re-orientation is folded into the
// destination addressing.
//
// LINEAR chroma needs, per plane, columns 2tx-1 .. 2tx+2 of chroma rows
// ty-1 .. ty+1: one dword load per row from the (unaligned) byte 2tx-1.  At
// the frame's left / right edge the load starts inside the row (column 0 /
// Wc-4) and the window is shifted in the register with the edge sample
// repeated; rows clamp to the frame's own plane, so no byte outside a row is
// read and a batch's neighbours never come from another frame.
//
// The two true divisions (Y / 255, s / 4080) are two operations each
// (div255 / div4080, color_div.hpp: correctly rounded for every numerator
// that occurs, which tests/test_yuv_to_bmp_host.py checks on the host).
namespace {

// the framebuffer write: UNORM8 of a colour component (the cast truncates,
// which is the definition's floor: the sum is in [0.5, 255.5])
__device__ __forceinline__ uint32_t unorm8(float c) {
  return (uint32_t)(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f + 0.5f);
}

// A chroma pair's contributions to r, g, g, b from the sample sums (16 x the
// sample for NEAREST, the 9/3/3/1 sum for LINEAR: both over 4080).
struct Chroma {
  float rv, gv, gu, bu;
};
__device__ __forceinline__ Chroma chroma(uint32_t su, uint32_t sv) {
  const float uf = div4080((float)su) - 0.5f;
  const float vf = div4080((float)sv) - 0.5f;
  return {1.403f * vf, 0.714f * vf, 0.344f * uf, 1.773f * uf};
}

// B | G << 8 | R << 16 of one pixel
__device__ __forceinline__ uint32_t bgr(uint32_t y, const Chroma& c) {
  const float yf = div255((float)y);
  const float r = yf + c.rv;
  const float g = (yf - c.gv) - c.gu;
  const float b = yf + c.bu;
  return unorm8(b) | unorm8(g) << 8 | unorm8(r) << 16;
}

__device__ __forceinline__ uint32_t load32(const uint8_t* p) {  // any alignment
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// Columns 2tx-1 .. 2tx+2 of a chroma row (one per byte, low byte first), the
// row's edge samples repeated past its ends (CLAMP_TO_EDGE).  wc >= 2, even.
__device__ __forceinline__ uint32_t window4(const uint8_t* __restrict__ row, uint32_t tx, uint32_t tiles_x,
                                            uint32_t wc) {
  if (wc == 2) {  // (uniform) one tile per row: c0 c0 c1 c1
    const uint32_t v = *reinterpret_cast<const uint16_t*>(row);
    return (v & 0xFFu) * 0x0101u | (v >> 8) * 0x01010000u;
  }
  const uint32_t s = tx == 0 ? 0u : (tx == tiles_x - 1 ? wc - 4 : 2 * tx - 1);
  const uint32_t v = load32(row + s);
  if (tx == 0) return v << 8 | (v & 0xFFu);                   // c0 c0 c1 c2
  if (tx == tiles_x - 1) return v >> 8 | (v & 0xFF000000u);  // c[wc-3] c[wc-2] c[wc-1] c[wc-1]
  return v;
}

// 3 * sample + neighbour along x for the tile's four luma columns: column k
// samples window byte 1 + k / 2, its neighbour is byte k / 2 + 2 * (k & 1)
// (left for even x, right for odd x).
__device__ __forceinline__ void hsum(uint32_t w, uint32_t (&h)[4]) {
  const uint32_t b0 = w & 0xFFu, b1 = (w >> 8) & 0xFFu, b2 = (w >> 16) & 0xFFu, b3 = w >> 24;
  h[0] = 3 * b1 + b0;
  h[1] = 3 * b1 + b2;
  h[2] = 3 * b2 + b1;
  h[3] = 3 * b2 + b3;
}

template <int BPP>
__device__ __forceinline__ void store4(uint8_t* __restrict__ dst, size_t pix, const uint32_t (&p)[4]) {
  uint32_t* q = reinterpret_cast<uint32_t*>(dst + pix * BPP);
  if constexpr (BPP == 4) {
    *reinterpret_cast<uint4*>(q) =
        make_uint4(p[0] | 0xFF000000u, p[1] | 0xFF000000u, p[2] | 0xFF000000u, p[3] | 0xFF000000u);
  } else {
    q[0] = p[0] | p[1] << 24;
    q[1] = p[1] >> 8 | p[2] << 16;
    q[2] = p[2] >> 16 | p[3] << 8;
  }
}

}  // namespace

// Block (64, 4); grid (ceil(W / 4 / 64), tile rows / 4, frames), the last two strided.  Frame f
// at src + f * W * H * 3 / 2 -> dst + f * W * H * BPP.  orient as K7's, for
// the destination.  LINEAR: 0 = nearest chroma sample, 1 = the bilinear
// 9/3/3/1 weights of GL_LINEAR at 1:1.
template <int BPP, int LINEAR>
__global__ __launch_bounds__(256) void k_iyuv_to_bmp(const uint8_t* __restrict__ src, uint32_t W, uint32_t H,
                                                     uint32_t nframes, uint32_t orient,
                                                     uint8_t* __restrict__ dst) {
  const uint32_t tiles_x = W / 4, tiles_y = H / 2, wc = W / 2, hc = H / 2;
  const size_t npx = (size_t)W * H;
  const uint32_t tx = blockIdx.x * 64 + threadIdx.x;
  if (tx >= tiles_x) return;
  const uint32_t c = 4 * tx;
  for (uint32_t f = blockIdx.z; f < nframes; f += gridDim.z) {
    const uint8_t* __restrict__ yp = src + (size_t)f * (npx / 2 * 3);
    const uint8_t* __restrict__ up = yp + npx;
    const uint8_t* __restrict__ vp = up + npx / 4;
    uint8_t* __restrict__ out = dst + (size_t)f * npx * BPP;
    for (uint32_t ty = blockIdx.y * 4 + threadIdx.y; ty < tiles_y; ty += gridDim.y * 4) {
      const uint32_t r = 2 * ty;
      const uint32_t Y[2] = {*reinterpret_cast<const uint32_t*>(yp + (size_t)r * W + c),
                             *reinterpret_cast<const uint32_t*>(yp + (size_t)(r + 1) * W + c)};
      // chroma sums of the tile's 2 x 4 pixels
      uint32_t su[2][4], sv[2][4];
      if constexpr (LINEAR) {
        // rows ty-1, ty, ty+1 of this frame's plane: the even luma row's
        // neighbour is the row above, the odd one's the row below
        const size_t rows[3] = {(size_t)(ty == 0 ? 0 : ty - 1) * wc, (size_t)ty * wc,
                                (size_t)(ty + 1 == hc ? ty : ty + 1) * wc};
        uint32_t hu[3][4], hv[3][4];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          hsum(window4(up + rows[i], tx, tiles_x, wc), hu[i]);
          hsum(window4(vp + rows[i], tx, tiles_x, wc), hv[i]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          su[0][k] = 3 * hu[1][k] + hu[0][k], su[1][k] = 3 * hu[1][k] + hu[2][k];
          sv[0][k] = 3 * hv[1][k] + hv[0][k], sv[1][k] = 3 * hv[1][k] + hv[2][k];
        }
      } else {
        const uint32_t u2 = *reinterpret_cast<const uint16_t*>(up + (size_t)ty * wc + 2 * tx);
        const uint32_t v2 = *reinterpret_cast<const uint16_t*>(vp + (size_t)ty * wc + 2 * tx);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          su[0][k] = su[1][k] = 16 * ((u2 >> (8 * (k >> 1))) & 0xFFu);
          sv[0][k] = sv[1][k] = 16 * ((v2 >> (8 * (k >> 1))) & 0xFFu);
        }
      }
#pragma unroll
      for (int dr = 0; dr < 2; dr++) {
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          // NEAREST: a 2x2 quad shares its chroma terms (the compiler merges the equal expressions)
          p[k] = bgr((Y[dr] >> (8 * k)) & 0xFFu, chroma(su[dr][k], sv[dr][k]));
        }
        const size_t lin = (size_t)(r + dr) * W + c;  // top-down pixel index of the tile row
        if (orient == 0) {
          store4<BPP>(out, lin, p);
        } else if (orient == 1) {  // pixels lin .. lin+3 go to npx-1-lin .. npx-4-lin
          const uint32_t q[4] = {p[3], p[2], p[1], p[0]};
          store4<BPP>(out, npx - 4 - lin, q);
        } else {
          store4<BPP>(out, (size_t)(H - 1 - (r + dr)) * W + c, p);
        }
      }
    }
  }
}

template __global__ void k_iyuv_to_bmp<3, 0>(const uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint8_t*);
template __global__ void k_iyuv_to_bmp<3, 1>(const uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint8_t*);
template __global__ void k_iyuv_to_bmp<4, 0>(const uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint8_t*);
template __global__ void k_iyuv_to_bmp<4, 1>(const uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint8_t*);

// ---- compare --------------------------------------------------------------
//
// k_frame_compare: PSNR's and block SSIM's integers between two raw IYUV
// frames in HBM (include/myyuv_hip.h, "Compare"; the arithmetic is metric.h).
// The fused decoder's grid (k_decode_compare): one wave per 64-block group of
// one plane (blockIdx.x: tiles_p0 groups of Y, tiles_p1 of U, then V) of frame
// blockIdx.y, lane l the group's block l, so a wave's totals belong to one
// plane.  A lane reads its block's 8 rows of both frames, 8 B each: the
// group's blocks are consecutive in a block row, so a row of the wave is one
// 512-B run.  Pure streaming: 128 B read per block, 8 B written with a map.
// ref_fbytes: G.fbytes, or 0 when every frame is compared with one reference.
__global__ __launch_bounds__(64) void k_frame_compare(const uint8_t* __restrict__ ref, uint32_t ref_fbytes,
                                                      const uint8_t* __restrict__ test, FrameGeom G,
                                                      uint32_t tiles_p0, uint32_t tiles_p1,
                                                      uint4* __restrict__ part,
                                                      myyuv_block_metric* __restrict__ map) {
  const uint32_t lane = threadIdx.x, t = blockIdx.x, f = blockIdx.y;
  const int p = t >= tiles_p0 ? (t >= tiles_p0 + tiles_p1 ? 2 : 1) : 0;
  auto sel3 = [p](uint32_t a0, uint32_t a1, uint32_t a2) { return p == 0 ? a0 : (p == 1 ? a1 : a2); };
  const uint32_t cum = sel3(G.cum[0], G.cum[1], G.cum[2]), nb = sel3(G.cum[1], G.cum[2], G.cum[3]) - cum;
  const uint32_t poff = sel3(G.poff[0], G.poff[1], G.poff[2]);
  const uint32_t pw = sel3(G.pw[0], G.pw[1], G.pw[2]), bw = sel3(G.bw[0], G.bw[1], G.bw[2]);
  const uint64_t bmag = p == 0 ? G.bmag[0] : (p == 1 ? G.bmag[1] : G.bmag[2]);
  const uint32_t local = (t - sel3(0u, tiles_p0, tiles_p0 + tiles_p1)) * kWave + lane;
  const bool live = local < nb;
  const uint32_t lc = live ? local : nb - 1;  // (lanes past the plane's end read its last block)
  const uint32_t by = div_magic(lc, bmag), bx = lc - by * bw;
  const uint32_t off = poff + by * 8u * pw + bx * 8u;
  const uint8_t* x = ref + (size_t)f * ref_fbytes + off;
  const uint8_t* y = test + (size_t)f * G.fbytes + off;
  uint2 xr[8], yr[8];
#pragma unroll
  for (uint32_t r = 0; r < 8; r++) {
    xr[r] = *reinterpret_cast<const uint2*>(x + r * pw);
    yr[r] = *reinterpret_cast<const uint2*>(y + r * pw);
  }
  myyuv_metric::Sums s;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    myyuv_metric::add_word(s, xr[r].x, yr[r].x);
    myyuv_metric::add_word(s, xr[r].y, yr[r].y);
  }
  mt::finish(s, live, mt::wave_slot(part), map != nullptr ? map + (size_t)f * G.cum[3] + cum + lc : nullptr);
}

// k_metric_reduce: the waves' totals of either Compare kernel (one uint4 per
// wave of the decoders' grid: sse, ssim, blocks, max; frame f's group t at
// part[f * (t0 + t1 + t2) + t]) added up per plane.  One workgroup per plane
// (blockIdx.x) of frame blockIdx.y; it writes the whole record, so nothing
// needs clearing between calls.  Integer sums: their order cannot change them.
__global__ __launch_bounds__(256) void k_metric_reduce(const uint4* __restrict__ part, uint32_t t0, uint32_t t1,
                                                       uint32_t t2, myyuv_frame_metric* __restrict__ out) {
  const uint32_t p = blockIdx.x, f = blockIdx.y;
  const uint32_t first = p == 0 ? 0u : (p == 1 ? t0 : t0 + t1), cnt = p == 0 ? t0 : (p == 1 ? t1 : t2);
  const uint4* src = part + (size_t)f * (t0 + t1 + t2) + first;
  unsigned long long sse = 0;
  long long ss = 0;
  uint32_t n = 0, mx = 0;
  // eight totals per thread and round, loaded unconditionally (slots past the
  // end read the round's first) so that all eight loads are in flight together:
  // one dependent load per round took 82 us for the 98,304 unit totals of an
  // 8192x8192 probe (profiles/target_rate.json)
  constexpr uint32_t kBatch = 8;
  for (uint32_t i0 = threadIdx.x; i0 < cnt; i0 += 256u * kBatch) {
    uint4 v[kBatch];
#pragma unroll
    for (uint32_t k = 0; k < kBatch; k++) v[k] = src[i0 + 256u * k < cnt ? i0 + 256u * k : i0];
#pragma unroll
    for (uint32_t k = 0; k < kBatch; k++) {
      if (i0 + 256u * k >= cnt) continue;
      sse += v[k].x;
      ss += (int32_t)v[k].y;
      n += v[k].z;
      mx = max(mx, v[k].w);
    }
  }
  __shared__ unsigned long long s_sse[256];
  __shared__ long long s_ss[256];
  __shared__ uint32_t s_n[256], s_mx[256];
  s_sse[threadIdx.x] = sse;
  s_ss[threadIdx.x] = ss;
  s_n[threadIdx.x] = n;
  s_mx[threadIdx.x] = mx;
  __syncthreads();
  for (uint32_t k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) {
      s_sse[threadIdx.x] += s_sse[threadIdx.x + k];
      s_ss[threadIdx.x] += s_ss[threadIdx.x + k];
      s_n[threadIdx.x] += s_n[threadIdx.x + k];
      s_mx[threadIdx.x] = max(s_mx[threadIdx.x], s_mx[threadIdx.x + k]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    myyuv_plane_metric r;
    r.sse = s_sse[0];
    r.ssim_sum = s_ss[0];
    r.nblocks = s_n[0];
    r.max_abs = s_mx[0];
    out[f].plane[p] = r;
  }
}

// k_probe_out: a probe's records (include/myyuv_hip.h, "Probe"), one thread
// per frame.  heads: the 12 bytes k_tile_scan writes at a stream's start (the
// three plane sizes) per frame, sizes: its payload sizes, rec: k_metric_reduce's
// records; `what` says which of them the launch produced, the rest of a record
// is zero.  Every record is written whole.
__global__ __launch_bounds__(64) void k_probe_out(const uint32_t* __restrict__ heads,
                                                  const uint32_t* __restrict__ sizes,
                                                  const myyuv_frame_metric* __restrict__ rec, uint32_t what,
                                                  uint32_t nframes, myyuv_probe* __restrict__ out) {
  const uint32_t f = blockIdx.x * 64u + threadIdx.x;
  if (f >= nframes) return;
  myyuv_probe r = {};
  if (what & MYYUV_PROBE_SIZE) {
    for (int p = 0; p < 3; p++) r.plane_bytes[p] = heads[3 * f + p];
    r.payload_bytes = sizes[f];
  }
  if (what & MYYUV_PROBE_METRIC) r.metric = rec[f];
  out[f] = r;
}

}  // namespace myyuv_gpu

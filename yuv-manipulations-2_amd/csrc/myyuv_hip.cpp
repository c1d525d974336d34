// myyuv_hip.cpp — implementation of the C ABI in include/myyuv_hip.h.
//
// Host side of the gfx950 codec: frame geometry, quantisation tables, the
// per-context workspace, and the launch sequences
//   compress:   K1 fdct_quant -> K2 huff_encode (+ overflow pass) -> K4 stream_out
//   from BMP:   bmp_fdct (K7's conversion + K1's FDCT) -> K2 (+ overflow pass) -> K4
//   decompress: parse -> scan -> K5 huff_decode -> K6 dequant_idct
//   region:     parse -> scan -> decode_region (a rectangle's blocks only)
//   scaled:     parse -> scan -> decode_scaled (every block, at 1/2, 1/4 or 1/8 size)
//   compare:    parse -> scan -> decode_compare (every block, against a reference frame's rows);
//               two raw frames: frame_compare
//   requantise: parse -> scan -> requant (decode + rescale) -> K2 (+ overflow pass) -> K4
//   downscale:  parse -> scan -> downscale (decode + scaled IDCT + K1's FDCT) -> K2 (+ overflow pass) -> K4
//   transform:  parse -> scan -> coef_xform (decode + move + rescale) -> K2 (+ overflow pass) -> K4
//   crop, join: parse -> scan -> gather_sizes -> scan -> gather_heads -> stream_gather (bytes only)
// Every launch goes to one stream; nothing synchronises inside the
// device-resident entry points, so frames pipeline back to back.
// The context, the owners of its HIP resources and the entry points'
// prologue (Entry: lock, device, stream, StreamOrder) are in host_ctx.hpp; the
// diagnostic and known-answer entry points in myyuv_hip_diag.cpp.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "host_ctx.hpp"
// (after the HIP runtime header)
#include "coef_xform.h"
#include "fdct_bfly.h"
#include "rate_search.h"

#ifndef MYYUV_R16_BATCH
#define MYYUV_R16_BATCH 1  // batches take the CAP-16 overflow tier too (0: single frames only)
#endif

namespace {

constexpr float kLumQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                             14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                             18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr float kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// DCT.cpp:286-290: Q = clamp(roundf(base * mul), 1, 255), mul in float.
void make_qtable(int q, bool chroma, float out[64]) {
  const float* base = chroma ? kChromaQ : kLumQ;
  const float fq = (float)q;
  const float mul = (fq >= 50.5f) ? (100.0f - fq) / 50.0f : 50.0f / fq;
  for (int i = 0; i < 64; i++) out[i] = std::min(std::max(std::roundf(base[i] * mul), 1.0f), 255.0f);
}

// K1/K6 grid: persistent waves (four per 256-thread workgroup) striding over
// the frame's 16-block units: as many workgroups as are resident at once
// (`resident`, from the occupancy query at context creation), never more
// waves than units.
dim3 xf_grid(const FrameGeom& G, uint32_t resident) {
  const uint32_t wgs = ceil_div(G.ucum[3] * G.nframes, 4);
  return dim3(wgs < resident ? wgs : resident);
}

// ceil(2^64 / bw) for FrameGeom::bmag; 0 marks bw = 1 (block_row returns local).
uint64_t block_magic(uint32_t bw) { return bw > 1 ? ~0ull / bw + 1 : 0; }

// Dimension checks in the reference's order: per plane, width then height
// (applyDCTPlane / restoreDCTPlane, DCT.cpp:280-285, :338-343).
int make_geom(uint32_t w, uint32_t h, FrameGeom& G) {
  if (w == 0 || h == 0) return MYYUV_E_WIDTH;
  if ((uint64_t)w * h * 3 / 2 > 0xFFFFFFFFull) return MYYUV_E_ARG;
  const uint32_t pw[3] = {w, w / 2, w / 2}, ph[3] = {h, h / 2, h / 2};
  for (int p = 0; p < 3; p++) {
    if (pw[p] % 8) return MYYUV_E_WIDTH;
    if (ph[p] % 8) return MYYUV_E_HEIGHT;
  }
  std::memset(&G, 0, sizeof(G));
  G.cum[0] = 0;
  for (int p = 0; p < 3; p++) {
    G.pw[p] = pw[p];
    G.ph[p] = ph[p];
    G.bw[p] = pw[p] / 8;
    G.cum[p + 1] = G.cum[p] + G.bw[p] * (ph[p] / 8);
    G.bmag[p] = block_magic(G.bw[p]);
    G.ucum[p + 1] = G.ucum[p] + ceil_div(G.cum[p + 1] - G.cum[p], kXfUnit);
    G.tcum[p + 1] = G.tcum[p] + ceil_div(G.cum[p + 1] - G.cum[p], kK2Group);
  }
  G.poff[0] = 0;
  G.poff[1] = w * h;
  G.poff[2] = w * h + (w / 2) * (h / 2);
  G.nframes = 1;
  G.fbytes = w * h / 2 * 3;
  G.umag = block_magic(G.ucum[3]);
  G.fbase = 0;
  // one frame's coefficient image within the kernels' 32-bit offsets (> 1.4 G
  // pixels; the reference's getImageSize overflows from 537 M pixels)
  if (G.cum[3] > kMaxLaunchBlocks) return MYYUV_E_ARG;
  return 0;
}

}  // namespace

FrameGeom block_geom(uint32_t nblocks) {
  FrameGeom G;
  std::memset(&G, 0, sizeof(G));
  G.pw[0] = 8;
  G.ph[0] = 8 * nblocks;
  G.bw[0] = 1;
  G.bmag[0] = block_magic(1);
  G.cum[1] = G.cum[2] = G.cum[3] = nblocks;
  G.ucum[1] = G.ucum[2] = G.ucum[3] = ceil_div(nblocks, kXfUnit);
  G.tcum[1] = G.tcum[2] = G.tcum[3] = ceil_div(nblocks, kK2Group);
  G.nframes = 1;
  G.fbytes = nblocks * 64;
  G.umag = block_magic(G.ucum[3]);
  return G;
}

// Reciprocals and K1's fast-path row bounds from the Q tables.
void finish_qtables(QTables& t, int planes) {
  for (int p = 0; p < planes; p++) {
    for (int n = 0; n < 64; n++) t.r[p][n] = 1.0f / t.q[p][n];
    myyuv_bfly::bfly_row_bounds(t.r[p], t.kb[p]);
  }
}

void drain_profile(myyuv_hip_ctx* c) {
  for (auto& it : c->pending) {
    float ms = 0;
    (void)hipEventSynchronize(it.stop);
    if (hipEventElapsedTime(&ms, it.start, it.stop) == hipSuccess) {
      c->ms[it.kid] += ms;
      c->launches[it.kid] += 1;
    }
    c->free_events.push_back(std::move(it.start));
    c->free_events.push_back(std::move(it.stop));
  }
  c->pending.clear();
}

myyuv_hip_ctx::~myyuv_hip_ctx() {
  if (stream) (void)hipStreamSynchronize(stream);
  if (pipe) {
    (void)hipStreamSynchronize(pipe->cin);
    (void)hipStreamSynchronize(pipe->cout);
  }
  if (last_stream) (void)hipEventSynchronize(done);
  drain_profile(this);
}

namespace {

// Frames per launch of geometry G (kMaxLaunchBlocks, or a smaller
// diagnostic cap: MYYUV_LAUNCH_BLOCKS, read at context creation).
uint32_t launch_frames(const FrameGeom& G, uint32_t cap_blocks = kMaxLaunchBlocks) {
  return std::max(1u, std::min(cap_blocks, kMaxLaunchBlocks) / G.cum[3]);
}

// A batch of nf frames of G's geometry (block, unit and byte counts of the
// whole batch must fit 32 bits).
int set_batch(FrameGeom& G, uint32_t nf) {
  if (nf == 0) return MYYUV_E_ARG;
  if ((uint64_t)G.cum[3] * nf > 0xFFFFFFFFull - 4096 || (uint64_t)G.fbytes * nf > 0xFFFFFFFFull)
    return MYYUV_E_ARG;
  G.nframes = nf;
  return 0;
}

// (C names, like the helpers further down that sit between the entry points:
// the library's dynamic symbol table has always listed them, and keeps them)
extern "C" {

int check_q(const uint8_t q[3]) {
  for (int p = 0; p < 3; p++)
    if (q[p] < 1 || q[p] > 100) return MYYUV_E_QUALITY;
  return 0;
}

// The kernels' error word (record_error, k_stream.hip) -> code, with the
// failing block counted from the call's first frame: the launch began at
// frame f0, nblk blocks per frame.  ~0: no error; a key of 0 in a launch
// that began at the call's first frame: no block (a later launch's key 0 is
// its first frame's block 0, as in a launch that holds the whole batch).
int chunk_err(unsigned long long v, uint32_t f0, uint32_t nblk, int64_t* bad_block) {
  if (v == ~0ull) return 0;
  const uint64_t key = v >> 8;
  if (bad_block) *bad_block = key == 0 && f0 == 0 ? -1 : (int64_t)(key >> 1) + (int64_t)f0 * nblk;
  return (int)(v & 0xFF);
}

}  // extern "C"

int set_qtables(myyuv_hip_ctx* c, const uint8_t q[3], hipStream_t s) {
  if (int e = check_q(q)) return e;
  if (c->q_valid && std::memcmp(c->q_cached, q, 3) == 0 && c->qt_stream == s) return 0;
  for (int p = 0; p < 3; p++) {
    make_qtable(q[p], p != 0, c->qt.q[p]);
  }
  finish_qtables(c->qt, 3);
  if (c->qtd.grow(sizeof(QTables))) return MYYUV_E_HIP;
  // kernels queued on another stream may still read the old tables
  if (c->qt_stream && c->qt_stream != s && hipStreamSynchronize(c->qt_stream) != hipSuccess)
    return MYYUV_E_HIP;
  // pageable source: the copy is staged before the call returns
  if (hipMemcpyAsync(c->qtd.p, &c->qt, sizeof(QTables), hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  c->qt_stream = s;
  std::memcpy(c->q_cached, q, 3);
  c->q_valid = true;
  return 0;
}

}  // namespace

// What k_scan_chain writes for a batch of G.nframes frames and the decoders
// read: the group offsets (4 B per block), the scan tiles' prefixes and
// look-back status words, the stream descriptors, the error word.  All a
// region decode needs (launch_decompress_region).
static int reserve_scan(myyuv_hip_ctx* c, const FrameGeom& G) {
  const uint32_t nf = G.nframes;
  const uint32_t ntiles = ceil_div(G.cum[3], kScanTile);
  int e = 0;
  e |= c->loff.grow((size_t)G.cum[3] * nf * 4);
  e |= c->tiles.grow((size_t)nf * (ntiles + 1) * 4);
  e |= c->err.grow(8);
  e |= c->desc.grow((size_t)nf * sizeof(StreamDesc));
  const size_t st_bytes = (size_t)nf * (ntiles + 1) * 8;
  if (c->status.n < st_bytes) {
    e |= c->status.grow(st_bytes);
    // zeroed before any kernel on any stream reads it
    if (!e && (hipMemset(c->status.p, 0, st_bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
      e |= MYYUV_E_HIP;
  }
  return e ? MYYUV_E_HIP : 0;
}

// Workspace for a batch of G.nframes frames (blocks numbered batch-globally;
// scan tiles, stream descriptors and look-back status words per frame).
int reserve(myyuv_hip_ctx* c, const FrameGeom& G) {
  const uint32_t nf = G.nframes;
  const uint32_t nblk = G.cum[3] * nf;
  const uint32_t nwaves = ceil_div(nblk, kWave);
  int e = 0;
  e |= c->coef.grow((size_t)nwaves * kCoefQuadsPerWave * 16);  // natural-order quads
  e |= c->stage.grow((size_t)win_tiles_alloc(nf * G.tcum[3]) * kTileCap);
  e |= c->oslots.grow((size_t)nblk * kMaxChunk);
  // (plus a guard band of one big window's tiles past the launch's last tile:
  // myyuv_debug_tinfo_guard checks that no kernel writes into it)
  e |= c->tinfo.grow((size_t)(nf * G.tcum[3] + kWinTilesBig) * kTInfoWords * 4);
  e |= c->srcoff.grow((size_t)nblk * 4);
  e |= c->sizes.grow((size_t)nwaves * kWave);
  e |= c->rmask.grow((size_t)nblk);
  e |= c->binfo.grow((size_t)nblk * 4);
  if (c->zq.n == 0) {
    e |= c->zq.grow(256);
    if (!e && hipMemset(c->zq.p, 0, 256) != hipSuccess) e |= MYYUV_E_HIP;
  }
  e |= reserve_scan(c, G);
  e |= c->sink.grow((size_t)kSinkQuads * 16 * kSinkSlots);  // K1/K6: 2 x 64 quads + K1's 64 mask bytes + 64 words
  e |= c->psize.grow(4);
  // [0], [1]: overflow counts, then K2's list and (single frames) the CAP-16 tier's (launch_overflow)
  e |= c->work.grow((size_t)nblk * (nf == 1 || MYYUV_R16_BATCH ? 8 : 4) + 256);
  {
    const size_t fb = fix_words(G.ucum[3] * nf) * 4;
    if (c->fix.n < fb) {
      e |= c->fix.grow(fb);
      if (!e && (hipMemset(c->fix.p, 0, kFixHeader * 4) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
        e |= MYYUV_E_HIP;
    }
  }
  return e ? MYYUV_E_HIP : 0;
}

namespace {

uint32_t next_epoch(myyuv_hip_ctx* c) {
  c->epoch = (c->epoch + 1) & kEpochMask;
  if (c->epoch == 0) c->epoch = 1;  // status words start zeroed: epoch 0 is never current
  return c->epoch;
}

// K2: fast pass over all tiles (grid (tiles, frames)), then the overflow pass
// over the blocks with more than 8 distinct symbols (worklist filled on the
// device; no host sync): wave-per-block for lists of at most kWaveEncodeLimit
// blocks, lane-per-block for longer ones; both kernels are queued and each
// returns at once outside its regime.  A batch (nf > 1) takes the
// lane-per-block pass only: its list is long, and the wave pass's per-block
// SALU cost would crowd the other launch groups in flight (tools/kskip.py).
// A list longer than one resident round of the lane pass (kR16Gate; a
// single frame's: two rounds of the wave pass, kR16GateSingle) goes
// through the CAP-16 register tier first (k_huff_encode_r16), and the two
// passes then take what it leaves (more than 16 symbols: work[1] blocks from
// word 64 + nblk).  work[0] is zeroed by K1 (or the host), work[1] here.
int launch_overflow(myyuv_hip_ctx* c, const FrameGeom& G, hipStream_t s) {
  const uint32_t nf = G.nframes, nblk = G.cum[3] * nf;
  uint32_t* count = c->work.as<uint32_t>();
  uint32_t* list = count + 64;
  uint32_t* count2 = count + 1;
  uint32_t* list2 = list + nblk;
  const uint32_t limit = nf > 1 ? kBatchWaveLimit : kWaveEncodeLimit;
  int e = 0;
  const uint32_t g16 = nf == 1 ? kR16GateSingle : kR16Gate;
  const uint32_t gate = (nf == 1 || MYYUV_R16_BATCH) && nblk > g16 ? g16 : ~0u;
  // (launched whenever such a list is possible; with 8-frame launch groups,
  // whose lists stay below the gate, the empty launch cost 3.4 % of the
  // bench, profiles/r3zw_*; the bench's 24-frame groups take the tier)
  if (gate != ~0u) {
    // work[1], the tier's count (its own node: a store in K1's prologue
    // shifted K1's loop and cost it 5 %, profiles/r3zx_*)
    e |= hipMemsetAsync(count2, 0, 4, s) != hipSuccess;
    const uint32_t r16 = ceil_div(nblk, kWave) < kR16Grid ? ceil_div(nblk, kWave) : kR16Grid;
    e |= launch(c, MYYUV_K_HUFF_R16, k_huff_encode_r16, dim3(r16), dim3(kWave), s, c->coef.as<const uint4>(),
                c->rmask.as<const uint8_t>(), c->zq.as<const uint4>(), G, c->oslots.as<uint32_t>(),
                c->sizes.as<uint8_t>(), c->tinfo.as<uint32_t>(), (const uint32_t*)list, (const uint32_t*)count,
                list2, count2, gate);
  }
  if (limit > 0)
    e |= launch(c, MYYUV_K_HUFF_WAVE, k_huff_encode_wave, dim3(kWaveEncodeGrid), dim3(kWave), s,
                c->coef.as<const uint4>(), c->rmask.as<const uint8_t>(), G, c->oslots.as<uint32_t>(),
                c->sizes.as<uint8_t>(), c->tinfo.as<uint32_t>(), (const uint32_t*)list, (const uint32_t*)count,
                (const uint32_t*)list2, (const uint32_t*)count2, gate, limit);
  const uint32_t wide = ceil_div(nblk, kWideLanes) < kWideGrid ? ceil_div(nblk, kWideLanes) : kWideGrid;
  e |= launch(c, MYYUV_K_HUFF_WIDE, k_huff_encode_wide, dim3(wide), dim3(kWideLanes), s,
              c->coef.as<const uint4>(), c->rmask.as<const uint8_t>(), c->zq.as<const uint4>(), G,
              c->oslots.as<uint32_t>(), c->sizes.as<uint8_t>(), c->tinfo.as<uint32_t>(), (const uint32_t*)list,
              (const uint32_t*)count, (const uint32_t*)list2, (const uint32_t*)count2, gate, limit);
  return e;
}

}  // namespace

int launch_huff_encode(myyuv_hip_ctx* c, const FrameGeom& G, hipStream_t s) {
  const uint32_t nf = G.nframes;
  uint32_t* count = c->work.as<uint32_t>();
  uint32_t* list = count + 64;
  // (*count was zeroed by K1, just before in the stream: k_fdct_quant's k2ctl)
  // (the window size of the launch, k2_win: K4 uses the same)
  const uint32_t W = k2_win(nf * G.tcum[3]);
  const int e = launch(c, MYYUV_K_HUFF_ENC, W == kWinTilesBig ? k_huff_encode<kWinTilesBig> : k_huff_encode<kWinTiles>,
                       dim3(ceil_div(nf * G.tcum[3], W)), dim3(kK2Group), s,
               c->coef.as<const uint4>(), c->binfo.as<const uint32_t>(), c->zq.as<const uint4>(), G,
               c->stage.as<uint32_t>(), c->tinfo.as<uint32_t>(), c->sizes.as<uint8_t>(),
               c->srcoff.as<uint32_t>(), list, count);
  return e | launch_overflow(c, G, s);
}

// K1, then its exact path for the units it listed (k_fdct_fix).  The list
// is on the device, so the fix grid cannot follow its length: the resident
// count (the fast path fails for 0.07 % of the bench frame's units at q50,
// 18 % at q90, 48 % at q100, more on noise: tools/diag/fast_dct_sim.py);
// workgroups past the list return at once.  MYYUV_FIX_GRID=n caps it at n
// workgroups for qualities up to MYYUV_FIX_QMAX (a test of the grid-stride
// walk).  k2ctl: K2's overflow count, zeroed by K1
// (nullptr: none).
int launch_fdct(myyuv_hip_ctx* c, const FrameGeom& G, const uint8_t* in, const QTables* qt, uint32_t* k2ctl,
                hipStream_t s) {
  const uint32_t par = c->fix_par;
  c->fix_par ^= 1u;
  int e = launch(c, MYYUV_K_FDCT, k_fdct_quant, xf_grid(G, c->xf_resident[0]), dim3(256), s, in, G, qt,
                 c->coef.as<uint4>(), c->rmask.as<uint8_t>(), c->binfo.as<uint32_t>(), c->sink.as<uint4>(), k2ctl,
                 c->fix.as<uint32_t>(), par);
  uint32_t qmax = 0;
  for (int p = 0; p < 3; p++) qmax = std::max(qmax, (uint32_t)c->q_cached[p]);
  const uint32_t want =
      (c->fix_grid == 0 || !c->q_valid || qmax > c->fix_qmax) ? c->fix_resident : c->fix_grid;
  // (a multiple of kFixLists waves: wave w takes list w % kFixLists)
  const uint32_t per = kFixLists / kFixWaves;
  const uint32_t grid = std::max(per, (want * 4 / kFixWaves) / per * per);
  e |= launch(c, MYYUV_K_FDCT_FIX, k_fdct_fix, dim3(grid), dim3(64 * kFixWaves), s, in, G, qt, c->coef.as<uint4>(),
              c->rmask.as<uint8_t>(), c->binfo.as<uint32_t>(), c->sink.as<uint4>(), c->fix.as<uint32_t>(), par);
  // the fix kernel zeroes the next launch's counts; without it (a diagnostic
  // skip, or a failed launch) the host does
  if (e || ((c->skip >> MYYUV_K_FDCT_FIX) & 1u))
    e |= hipMemsetAsync(fix_count(c->fix.as<uint32_t>(), par ^ 1u, 0), 0, kFixLists * 32 * 4, s) != hipSuccess;
  return e;
}

namespace {

// One batch of G.nframes frames (frame f at d_in + f * fbytes), payload f at
// d_out + f * cap, its size at d_size[f].
int launch_compress(myyuv_hip_ctx* c, const FrameGeom& G, const void* d_in, void* d_out,
                    uint32_t cap, uint32_t* d_size, hipStream_t s, unsigned long long* err = nullptr) {
  const uint32_t nf = G.nframes;
  const QTables* qt = c->qtd.as<const QTables>();
  if (!err) err = c->err.as<unsigned long long>();
  int e = 0;
  if (c->fused) {
    // fused single-pass encoder (K1 + K2 per tile), then the overflow passes
    uint32_t* count = c->work.as<uint32_t>();
    e |= hipMemsetAsync(count, 0, 4, s) != hipSuccess;
    e |= launch(c, MYYUV_K_ENCODE_TILE, k_encode_tile, dim3(G.tcum[3], nf), dim3(kK2Group), s,
                static_cast<const uint8_t*>(d_in), G, qt, c->coef.as<uint4>(), c->rmask.as<uint8_t>(),
                c->stage.as<uint32_t>(), c->tinfo.as<uint32_t>(), c->sizes.as<uint8_t>(), c->srcoff.as<uint32_t>(),
                count + 64, count);
    e |= launch_overflow(c, G, s);
  } else {
    e |= launch_fdct(c, G, static_cast<const uint8_t*>(d_in), qt, c->work.as<uint32_t>(), s);
    if ((c->skip >> MYYUV_K_FDCT) & 1u)  // diagnostic skip: keep K1's reset of the overflow count
      e |= hipMemsetAsync(c->work.p, 0, 4, s) != hipSuccess;
    e |= launch_huff_encode(c, G, s);
  }
  e |= launch(c, MYYUV_K_SCAN, k_tile_scan, dim3(nf), dim3(256), s, c->tinfo.as<uint32_t>(), G,
              static_cast<uint8_t*>(d_out), cap, d_size, err);
  // K4 reads the stage in K2's windows (k2_win; the fused encoder's: kWinTiles)
  const uint32_t W = c->fused ? kWinTiles : k2_win(nf * G.tcum[3]);
  e |= launch(c, MYYUV_K_COMPACT, k_stream_out, dim3(ceil_div(G.tcum[3] * nf, 8 * W) * 8 * W), dim3(256), s,
              c->stage.as<const uint32_t>(), c->tinfo.as<const uint32_t>(), c->sizes.as<const uint8_t>(),
              c->srcoff.as<const uint32_t>(), c->oslots.as<const uint32_t>(), G, static_cast<uint8_t*>(d_out),
              cap, W);
  return e ? MYYUV_E_HIP : 0;
}

// The mirror: payload f at d_in + f * cap (size d_size[f]) -> frame f at
// d_out + f * fbytes.
int launch_decompress(myyuv_hip_ctx* c, const FrameGeom& G, const void* d_in,
                      const uint32_t* d_size, uint32_t cap, void* d_out, hipStream_t s,
                      unsigned long long* err = nullptr) {
  const uint32_t nf = G.nframes;
  const uint32_t nblk = G.cum[3];
  const uint32_t ntiles = ceil_div(nblk, kScanTile);
  const QTables* qt = c->qtd.as<const QTables>();
  if (!err) err = c->err.as<unsigned long long>();
  StreamDesc* desc = c->desc.as<StreamDesc>();
  const uint8_t* in = static_cast<const uint8_t*>(d_in);
  int e = 0;
  ScanSrc S;
  for (int i = 0; i < 4; i++) S.cum[i] = G.cum[i];
  for (int p = 0; p < 3; p++) S.pos[p] = 0;
  e |= launch(c, MYYUV_K_SCAN, k_scan_chain, dim3(ntiles, nf), dim3(256), s, in, cap, S, d_size, cap,
              G, desc, c->loff.as<uint32_t>(), c->tiles.as<uint32_t>(), ntiles,
              c->status.as<unsigned long long>(), next_epoch(c), err);
  const uint32_t t0 = ceil_div(G.cum[1] - G.cum[0], kWave),
                 t1 = ceil_div(G.cum[2] - G.cum[1], kWave),
                 t2 = ceil_div(G.cum[3] - G.cum[2], kWave);
  if (c->fused_dec) {  // K5 + K6 in one pass, the coefficients kept on chip
    if ((uint64_t)(t0 + t1 + t2) * nf >= c->dec_span_min) {  // a wave per span (same kernel id)
      const uint32_t s0 = ceil_div(G.cum[1] - G.cum[0], kDecSpan), s1 = ceil_div(G.cum[2] - G.cum[1], kDecSpan),
                     s2 = ceil_div(G.cum[3] - G.cum[2], kDecSpan);
      e |= launch(c, MYYUV_K_HUFF_DEC, k_decode_span, dim3(s0 + s1 + s2, nf), dim3(kWave), s, in, d_size, cap,
                  (const StreamDesc*)desc, c->loff.as<const uint32_t>(), c->tiles.as<const uint32_t>(), G, s0, s1,
                  qt, c->coef.as<uint4>(), static_cast<uint8_t*>(d_out), err);
      return e ? MYYUV_E_HIP : 0;
    }
    e |= launch(c, MYYUV_K_HUFF_DEC, k_decode_idct, dim3(t0 + t1 + t2, nf), dim3(kWave), s, in, d_size, cap,
                (const StreamDesc*)desc, c->loff.as<const uint32_t>(), c->tiles.as<const uint32_t>(), G, t0, t1,
                qt, c->coef.as<uint4>(), static_cast<uint8_t*>(d_out), err);
    return e ? MYYUV_E_HIP : 0;
  }
  e |= launch(c, MYYUV_K_HUFF_DEC, k_huff_decode, dim3(t0 + t1 + t2, nf), dim3(kWave), s, in, d_size,
              cap, (const StreamDesc*)desc, c->loff.as<const uint32_t>(),
              c->tiles.as<const uint32_t>(), G, t0, t1, c->coef.as<uint4>(), c->rmask.as<uint8_t>(), err);
  e |= launch(c, MYYUV_K_IDCT, k_dequant_idct, xf_grid(G, c->xf_resident[1]), dim3(256), s,
              c->coef.as<const uint4>(), c->rmask.as<const uint8_t>(), c->zq.as<const uint4>(), G, qt,
              static_cast<uint8_t*>(d_out), c->sink.as<uint4>());
  return e ? MYYUV_E_HIP : 0;
}

// The region (rx, ry, rw, rh) of a w x h frame: multiples of 16 (whole blocks
// in every plane, and the result a compressible frame), not empty, inside
// the frame (sums in 64 bits).  R: the output frame's geometry, S: the
// rectangle's place in the source planes and its segments.
int make_region(uint32_t w, uint32_t h, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh, FrameGeom& R,
                RegionSegs& S) {
  if (((rx | ry | rw | rh) & 15u) || rw == 0 || rh == 0) return MYYUV_E_ARG;
  if ((uint64_t)rx + rw > w || (uint64_t)ry + rh > h) return MYYUV_E_ARG;
  if (make_geom(rw, rh, R)) return MYYUV_E_ARG;
  S.scum[0] = 0;
  for (int p = 0; p < 3; p++) {
    const uint32_t sh = p ? 4 : 3;  // log2 of the plane's block size in luma pixels
    S.bx[p] = rx >> sh;
    S.by[p] = ry >> sh;
    S.spr[p] = ceil_div(R.bw[p], kWave);
    S.scum[p + 1] = S.scum[p] + S.spr[p] * (R.ph[p] / 8);
  }
  return 0;
}

// Region decode: payload f at d_in + f * cap -> the region's frame f at d_out +
// f * R.fbytes.  The size table of the whole frame is scanned as
// launch_decompress does; k_decode_region then reads the region's chunks
// only, whatever MYYUV_DECODER says (there is no split form).
int launch_decompress_region(myyuv_hip_ctx* c, const FrameGeom& G, const FrameGeom& R, const RegionSegs& S,
                             const void* d_in, const uint32_t* d_size, uint32_t cap, void* d_out, hipStream_t s) {
  const uint32_t nf = G.nframes;
  const uint32_t ntiles = ceil_div(G.cum[3], kScanTile);
  unsigned long long* err = c->err.as<unsigned long long>();
  StreamDesc* desc = c->desc.as<StreamDesc>();
  const uint8_t* in = static_cast<const uint8_t*>(d_in);
  int e = 0;
  ScanSrc SS;
  for (int i = 0; i < 4; i++) SS.cum[i] = G.cum[i];
  for (int p = 0; p < 3; p++) SS.pos[p] = 0;
  e |= launch(c, MYYUV_K_SCAN, k_scan_chain, dim3(ntiles, nf), dim3(256), s, in, cap, SS, d_size, cap, G, desc,
              c->loff.as<uint32_t>(), c->tiles.as<uint32_t>(), ntiles, c->status.as<unsigned long long>(),
              next_epoch(c), err);
  e |= launch(c, MYYUV_K_REGION, k_decode_region, dim3(S.scum[3], nf), dim3(kWave), s, in, d_size, cap,
              (const StreamDesc*)desc, c->loff.as<const uint32_t>(), c->tiles.as<const uint32_t>(), G, R, S,
              c->qtd.as<const QTables>(), static_cast<uint8_t*>(d_out), err);
  return e ? MYYUV_E_HIP : 0;
}

// Scaled decode (denom 2, 4 or 8): payload f at d_in + f * cap -> the scaled
// frame f at d_out + f * G.fbytes / denom^2.  The scan as launch_decompress
// runs it, then k_decode_scaled<8 / denom> on k_decode_idct's grid, whatever
// MYYUV_DECODER says (there is no split form).  Workspace: reserve_scaled.
int reserve_scaled(myyuv_hip_ctx* c, const FrameGeom& G) {
  const uint32_t nwaves = ceil_div(G.cum[3] * G.nframes, kWave);
  if (c->coef.grow((size_t)nwaves * kCoefQuadsPerWave * 16)) return MYYUV_E_HIP;  // (decode_general's blocks)
  return reserve_scan(c, G);
}

int launch_decompress_scaled(myyuv_hip_ctx* c, const FrameGeom& G, uint32_t denom, const void* d_in,
                             const uint32_t* d_size, uint32_t cap, void* d_out, hipStream_t s) {
  const uint32_t nf = G.nframes;
  const uint32_t ntiles = ceil_div(G.cum[3], kScanTile);
  unsigned long long* err = c->err.as<unsigned long long>();
  StreamDesc* desc = c->desc.as<StreamDesc>();
  const uint8_t* in = static_cast<const uint8_t*>(d_in);
  int e = 0;
  ScanSrc SS;
  for (int i = 0; i < 4; i++) SS.cum[i] = G.cum[i];
  for (int p = 0; p < 3; p++) SS.pos[p] = 0;
  e |= launch(c, MYYUV_K_SCAN, k_scan_chain, dim3(ntiles, nf), dim3(256), s, in, cap, SS, d_size, cap, G, desc,
              c->loff.as<uint32_t>(), c->tiles.as<uint32_t>(), ntiles, c->status.as<unsigned long long>(),
              next_epoch(c), err);
  const uint32_t t0 = ceil_div(G.cum[1] - G.cum[0], kWave), t1 = ceil_div(G.cum[2] - G.cum[1], kWave),
                 t2 = ceil_div(G.cum[3] - G.cum[2], kWave);
  auto* k = denom == 2 ? k_decode_scaled<4> : (denom == 4 ? k_decode_scaled<2> : k_decode_scaled<1>);
  e |= launch(c, MYYUV_K_SCALED, k, dim3(t0 + t1 + t2, nf), dim3(kWave), s, in, d_size, cap,
              (const StreamDesc*)desc, c->loff.as<const uint32_t>(), c->tiles.as<const uint32_t>(), G, t0, t1,
              c->qtd.as<const QTables>(), c->coef.as<uint4>(), static_cast<uint8_t*>(d_out), err);
  return e ? MYYUV_E_HIP : 0;
}

bool denom_ok(uint32_t denom) { return denom == 2 || denom == 4 || denom == 8; }

// The requantiser's tables for (q_src, q_dst), on the device in stream order;
// cached by the six quality bytes as set_qtables caches its triple.  The
// compress / decompress tables (qt, qtd, q_cached, q_valid) are not touched.
// swap (the transform's transposing operations): qs is held as the transposed
// block reads it, qs[8u' + v'] = Qs[8v' + u'] (coef_xform.h xf_source_table).
int set_requant_tables(myyuv_hip_ctx* c, const uint8_t qs[3], const uint8_t qd[3], hipStream_t s,
                       bool swap = false) {
  uint8_t key[6];
  std::memcpy(key, qs, 3);
  std::memcpy(key + 3, qd, 3);
  if (c->rq_valid && std::memcmp(c->rq_cached, key, 6) == 0 && c->rq_swap == swap && c->rq_stream == s)
    return 0;
  c->rq_valid = false;  // (until the new tables are queued)
  c->rq_eq = 0;
  for (int p = 0; p < 3; p++) {
    float t[64];
    make_qtable(qs[p], p != 0, t);
    myyuv_xform::xf_source_table(swap ? myyuv_xform::kSwap : 0u, t, c->rq.qs[p]);
    make_qtable(qd[p], p != 0, c->rq.qd[p]);
    if (std::memcmp(c->rq.qs[p], c->rq.qd[p], sizeof(t)) == 0) c->rq_eq |= 1u << p;
  }
  c->rq_swap = swap;
  if (c->rqt.grow(sizeof(RequantTables))) return MYYUV_E_HIP;
  // kernels queued on another stream may still read the old tables
  if (c->rq_stream && c->rq_stream != s && hipStreamSynchronize(c->rq_stream) != hipSuccess) return MYYUV_E_HIP;
  if (hipMemcpyAsync(c->rqt.p, &c->rq, sizeof(RequantTables), hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  c->rq_stream = s;
  std::memcpy(c->rq_cached, key, 6);
  c->rq_valid = true;
  return 0;
}

// The encoder from K2 on, over K1's hand-off (coefficient quads, row masks,
// block words) of Gd's batch: K2, the tile scan and the stream writer, as
// launch_compress runs them after K1.  Shared by requantise, transform,
// downscale and the JPEG import; the caller has zeroed work[0].
int launch_encode_tail(myyuv_hip_ctx* c, const FrameGeom& Gd, void* d_out, uint32_t cap_out, uint32_t* d_size_out,
                       hipStream_t s) {
  const uint32_t nf = Gd.nframes;
  unsigned long long* err = c->err.as<unsigned long long>();
  int e = 0;
  e |= launch_huff_encode(c, Gd, s);
  e |= launch(c, MYYUV_K_SCAN, k_tile_scan, dim3(nf), dim3(256), s, c->tinfo.as<uint32_t>(), Gd,
              static_cast<uint8_t*>(d_out), cap_out, d_size_out, err);
  const uint32_t W = k2_win(nf * Gd.tcum[3]);  // (K2's windows, as launch_compress)
  e |= launch(c, MYYUV_K_COMPACT, k_stream_out, dim3(ceil_div(Gd.tcum[3] * nf, 8 * W) * 8 * W), dim3(256), s,
              c->stage.as<const uint32_t>(), c->tinfo.as<const uint32_t>(), c->sizes.as<const uint8_t>(),
              c->srcoff.as<const uint32_t>(), c->oslots.as<const uint32_t>(), Gd, static_cast<uint8_t*>(d_out),
              cap_out, W);
  return e ? MYYUV_E_HIP : 0;
}

// Requantise and transform (include/myyuv_hip.h): stream f at d_in + f * cap_in
// (its size at d_size_in[f]) -> stream f at d_out + f * cap_out, its size at
// d_size_out[f].  The scan as launch_decompress runs it; k_requant (op < 0) or
// k_coef_xform decodes every block, rescales (and moves) it and leaves K1's
// hand-off (coefficient quads, row masks, block words); then the encoder from
// K2 on, as launch_compress runs it after K1.  work[0], K2's overflow count, is
// zeroed here as K1 would have.  No K1, no fix kernel, no K6.  Workspace:
// reserve (the compress calls'), and for the transform reserve_xform.
// G is the source frame's geometry (the scan and the decode), Gd the
// destination's (the encoder and the writer): the same batch, and the same
// block, tile and unit counts per plane; they differ after a swap, in the
// planes' widths.
int launch_recode(myyuv_hip_ctx* c, const FrameGeom& G, const FrameGeom& Gd, int op, const void* d_in,
                  const uint32_t* d_size_in, uint32_t cap_in, void* d_out, uint32_t cap_out, uint32_t* d_size_out,
                  hipStream_t s) {
  const uint32_t nf = G.nframes;
  const uint32_t ntiles = ceil_div(G.cum[3], kScanTile);
  unsigned long long* err = c->err.as<unsigned long long>();
  StreamDesc* desc = c->desc.as<StreamDesc>();
  const uint8_t* in = static_cast<const uint8_t*>(d_in);
  int e = 0;
  ScanSrc SS;
  for (int i = 0; i < 4; i++) SS.cum[i] = G.cum[i];
  for (int p = 0; p < 3; p++) SS.pos[p] = 0;
  e |= launch(c, MYYUV_K_SCAN, k_scan_chain, dim3(ntiles, nf), dim3(256), s, in, cap_in, SS, d_size_in, cap_in, G,
              desc, c->loff.as<uint32_t>(), c->tiles.as<uint32_t>(), ntiles, c->status.as<unsigned long long>(),
              next_epoch(c), err);
  e |= hipMemsetAsync(c->work.p, 0, 4, s) != hipSuccess;
  const uint32_t t0 = ceil_div(G.cum[1] - G.cum[0], kWave), t1 = ceil_div(G.cum[2] - G.cum[1], kWave),
                 t2 = ceil_div(G.cum[3] - G.cum[2], kWave);
  if (op < 0)
    e |= launch(c, MYYUV_K_REQUANT, k_requant, dim3(t0 + t1 + t2, nf), dim3(kWave), s, in, d_size_in, cap_in,
                (const StreamDesc*)desc, c->loff.as<const uint32_t>(), c->tiles.as<const uint32_t>(), G, t0, t1,
                c->rqt.as<const RequantTables>(), c->coef.as<uint4>(), c->rmask.as<uint8_t>(),
                c->binfo.as<uint32_t>(), err);
  else
    e |= launch(c, MYYUV_K_COEF_XF, k_coef_xform, dim3(t0 + t1 + t2, nf), dim3(kWave), s, in, d_size_in, cap_in,
                (const StreamDesc*)desc, c->loff.as<const uint32_t>(), c->tiles.as<const uint32_t>(), G, t0, t1,
                c->rqt.as<const RequantTables>(), (uint32_t)op, c->rq_eq, c->xfgen.as<uint4>(), c->coef.as<uint4>(),
                c->rmask.as<uint8_t>(), c->binfo.as<uint32_t>(), err);
  e |= launch_encode_tail(c, Gd, d_out, cap_out, d_size_out, s);
  return e ? MYYUV_E_HIP : 0;
}

int launch_requant(myyuv_hip_ctx* c, const FrameGeom& G, const void* d_in, const uint32_t* d_size_in,
                   uint32_t cap_in, void* d_out, uint32_t cap_out, uint32_t* d_size_out, hipStream_t s) {
  return launch_recode(c, G, G, -1, d_in, d_size_in, cap_in, d_out, cap_out, d_size_out, s);
}

// Transform (include/myyuv_hip.h): op is MYYUV_XF_*, Gd the geometry of the
// H x W frame after a swap (G itself otherwise), with G's batch.
int launch_coef_xform(myyuv_hip_ctx* c, const FrameGeom& G, const FrameGeom& Gd, uint32_t op, const void* d_in,
                      const uint32_t* d_size_in, uint32_t cap_in, void* d_out, uint32_t cap_out,
                      uint32_t* d_size_out, hipStream_t s) {
  return launch_recode(c, G, Gd, (int)op, d_in, d_size_in, cap_in, d_out, cap_out, d_size_out, s);
}

// The downscaler's tables for (q_src, q_dst), on the device in stream order;
// cached by the six quality bytes as set_requant_tables caches its pair.  The
// other calls' tables (qt / qtd, rq / rqt) and their caches are not touched.
int set_downscale_tables(myyuv_hip_ctx* c, const uint8_t qs[3], const uint8_t qd[3], hipStream_t s) {
  uint8_t key[6];
  std::memcpy(key, qs, 3);
  std::memcpy(key + 3, qd, 3);
  if (c->ds_valid && std::memcmp(c->ds_cached, key, 6) == 0 && c->ds_stream == s) return 0;
  c->ds_valid = false;  // (until the new tables are queued)
  for (int p = 0; p < 3; p++) {
    make_qtable(qs[p], p != 0, c->ds.qs[p]);
    make_qtable(qd[p], p != 0, c->ds.d.q[p]);
  }
  finish_qtables(c->ds.d, 3);
  if (c->dst.grow(sizeof(DownscaleTables))) return MYYUV_E_HIP;
  // kernels queued on another stream may still read the old tables
  if (c->ds_stream && c->ds_stream != s && hipStreamSynchronize(c->ds_stream) != hipSuccess) return MYYUV_E_HIP;
  if (hipMemcpyAsync(c->dst.p, &c->ds, sizeof(DownscaleTables), hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  c->ds_stream = s;
  std::memcpy(c->ds_cached, key, 6);
  c->ds_valid = true;
  return 0;
}

// Downscale (include/myyuv_hip.h): stream f of G's frames at d_in + f * cap_in
// -> the stream of the 1/denom-size frame (geometry Gd, the same batch) at
// d_out + f * cap_out.  The scan as launch_decompress runs it on the source;
// k_downscale<8 / denom> decodes every block, builds the scaled pixels in LDS
// and leaves K1's hand-off for the destination's blocks; then the encoder from
// K2 on with Gd, as launch_recode runs it.  work[0] is zeroed here as K1 would
// have.  No scaled frame, no K1, no fix kernel.  Workspace: reserve_downscale.
int reserve_downscale(myyuv_hip_ctx* c, const FrameGeom& G, const FrameGeom& Gd) {
  if (int e = reserve_scan(c, G)) return e;  // (the source's; reserve's own, for Gd, is smaller)
  return reserve(c, Gd);
}

int launch_downscale(myyuv_hip_ctx* c, const FrameGeom& G, const FrameGeom& Gd, uint32_t denom, const void* d_in,
                     const uint32_t* d_size_in, uint32_t cap_in, void* d_out, uint32_t cap_out,
                     uint32_t* d_size_out, hipStream_t s) {
  const uint32_t nf = G.nframes;
  const uint32_t ntiles = ceil_div(G.cum[3], kScanTile);
  unsigned long long* err = c->err.as<unsigned long long>();
  StreamDesc* desc = c->desc.as<StreamDesc>();
  const uint8_t* in = static_cast<const uint8_t*>(d_in);
  int e = 0;
  ScanSrc SS;
  for (int i = 0; i < 4; i++) SS.cum[i] = G.cum[i];
  for (int p = 0; p < 3; p++) SS.pos[p] = 0;
  e |= launch(c, MYYUV_K_SCAN, k_scan_chain, dim3(ntiles, nf), dim3(256), s, in, cap_in, SS, d_size_in, cap_in, G,
              desc, c->loff.as<uint32_t>(), c->tiles.as<uint32_t>(), ntiles, c->status.as<unsigned long long>(),
              next_epoch(c), err);
  e |= hipMemsetAsync(c->work.p, 0, 4, s) != hipSuccess;
  const myyuv_downscale::Map M = myyuv_downscale::make_map(G.pw[0], G.ph[0], denom);
  auto* k = denom == 2 ? k_downscale<4> : (denom == 4 ? k_downscale<2> : k_downscale<1>);
  e |= launch(c, MYYUV_K_DOWNSCALE, k, dim3(M.wcum[3], nf), dim3(kWave), s, in, d_size_in, cap_in,
              (const StreamDesc*)desc, c->loff.as<const uint32_t>(), c->tiles.as<const uint32_t>(), G, Gd, M,
              c->dst.as<const DownscaleTables>(), c->coef.as<uint4>(), c->rmask.as<uint8_t>(),
              c->binfo.as<uint32_t>(), err);
  e |= launch_encode_tail(c, Gd, d_out, cap_out, d_size_out, s);
  return e ? MYYUV_E_HIP : 0;
}

// The transform's scratch coefficient image (decode_general's blocks, in
// source order: the hand-off image is written in destination order by other
// waves meanwhile), sized as reserve sizes the hand-off image.
int reserve_xform(myyuv_hip_ctx* c, const FrameGeom& G) {
  const uint32_t nwaves = ceil_div(G.cum[3] * G.nframes, kWave);
  return c->xfgen.grow((size_t)nwaves * kCoefQuadsPerWave * 16) ? MYYUV_E_HIP : 0;
}

// The destination geometry of `op` on a w x h frame whose geometry is G, with
// G's batch and launch base.
int xform_geom(const FrameGeom& G, uint32_t w, uint32_t h, uint32_t op, FrameGeom& Gd) {
  Gd = G;
  if (!MYYUV_XF_SWAPS(op)) return 0;
  const int e = make_geom(h, w, Gd);
  if (e) return e;
  Gd.nframes = G.nframes;
  Gd.fbase = G.fbase;
  return 0;
}

// Host <-> device copies of the host-buffer entry points: direct async copies
// from / into the caller's pageable buffers.  On this stack they run at the
// PCIe link rate whatever the buffer's alignment or age (tools/ubench/
// pcie_copy.cpp, profiles/r3b_pcie_copy.txt: 18 MB in 0.33-0.43 ms, a fresh
// or 1-byte-misaligned buffer included), faster than staging through pinned
// chunks with a CPU copy (0.47-0.59 ms H2D, 1.1-2.7 ms D2H).
int h2d(void* dst, const void* src, size_t n, hipStream_t s) {
  return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s) == hipSuccess ? 0 : MYYUV_E_HIP;
}

// (synchronous: returns when dst holds the bytes)
int d2h(void* dst, const void* src, size_t n, hipStream_t s) {
  return hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess
             ? 0
             : MYYUV_E_HIP;
}

int reset_err(myyuv_hip_ctx* c, hipStream_t s) {
  return hipMemsetAsync(c->err.p, 0xFF, 8, s) == hipSuccess ? 0 : MYYUV_E_HIP;
}

int read_err(myyuv_hip_ctx* c, hipStream_t s, int64_t* bad_block) {
  unsigned long long v = ~0ull;
  if (hipMemcpyAsync(&v, c->err.p, 8, hipMemcpyDeviceToHost, s) != hipSuccess) return MYYUV_E_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return MYYUV_E_HIP;
  if (bad_block) *bad_block = -1;
  return chunk_err(v, 0, 0, bad_block);
}

// Host mirror of the stream header checks (parse_stream, k_chain.hpp; same order), for host buffers.
int host_parse_headers(const uint8_t* in, uint32_t size) {
  auto rd32 = [&](uint64_t a) {
    uint32_t v;
    std::memcpy(&v, in + a, 4);
    return v;
  };
  if (size <= 12) return MYYUV_E_DCTYUV_SIZE;
  const uint32_t ps[3] = {rd32(0), rd32(4), rd32(8)};
  if (12ull + ps[0] + ps[1] + ps[2] > size) return MYYUV_E_DCTYUV_SIZE;
  uint64_t off = 12;
  for (int p = 0; p < 3; p++) {
    if (ps[p] <= 8) return MYYUV_E_PLANE_SIZE;
    const uint32_t hn = rd32(off), hc = rd32(off + 4);
    if (hn == 0) return MYYUV_E_PLANE_NBLK;
    if (hc == 0) return MYYUV_E_PLANE_CONTENT;
    if (8ull + hn + hc > ps[p]) return MYYUV_E_PLANE_SIZE;
    off += ps[p];
  }
  return 0;
}

bool hip_ok() {
  static int ok = -1;
  if (ok < 0) {
    int n = 0;
    ok = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0;
  }
  return ok == 1;
}

// The device-resident codec calls, both directions (compress: frames ->
// payloads; frame f at d_frames + f * fbytes, payload f at d_payloads +
// f * cap, its size at d_sizes[f]).  Nothing synchronises.
int batch_device(bool compress, myyuv_hip_ctx* c, void* d_frames, void* d_payloads, uint32_t* d_sizes,
                 uint32_t cap, uint32_t nframes, uint32_t w, uint32_t h, const uint8_t q[3], void* stream) {
  if (!c || !d_frames || !d_payloads || !d_sizes || !q) return MYYUV_E_ARG;
  if (((uintptr_t)d_payloads & 3) || ((uintptr_t)d_frames & 7) || (nframes > 1 && (cap & 3)))
    return MYYUV_E_ARG;
  FrameGeom G;
  int e = check_q(q);
  if (e || (e = make_geom(w, h, G)) || (e = set_batch(G, nframes))) return e;
  Entry en(c, stream);
  // (as several launches when the batch's coefficient image would reach 4 GiB)
  const uint32_t per = launch_frames(G, c->launch_blocks);
  FrameGeom GL = G;
  if ((e = set_batch(GL, std::min(nframes, per))) || (e = reserve(c, GL)) || (e = set_qtables(c, q, en.s))) return e;
  for (uint32_t f0 = 0; f0 < nframes; f0 += per) {
    GL = G;
    GL.fbase = f0;
    if ((e = set_batch(GL, std::min(per, nframes - f0)))) return e;
    uint8_t* fr = static_cast<uint8_t*>(d_frames) + (size_t)f0 * G.fbytes;
    uint8_t* pay = static_cast<uint8_t*>(d_payloads) + (size_t)f0 * cap;
    if ((e = compress ? launch_compress(c, GL, fr, pay, cap, d_sizes + f0, en.s)
                      : launch_decompress(c, GL, pay, d_sizes + f0, cap, fr, en.s)))
      return e;
  }
  return 0;
}

}  // namespace

extern "C" {

const char* myyuv_hip_strerror(int code) {
  switch (code) {
    case MYYUV_OK: return "Success";
    case MYYUV_E_ARG: return "Invalid argument";
    case MYYUV_E_QUALITY: return "Level of quality must be between 1 and 100";
    case MYYUV_E_WIDTH: return "Error. width % 8 must be 0";
    case MYYUV_E_HEIGHT: return "Error. height % 8 must be 0";
    case MYYUV_E_CAPACITY: return "Output buffer too small for the compressed stream";
    case MYYUV_E_DCTYUV_SIZE: return "DCTYUV load bad size";
    case MYYUV_E_PLANE_SIZE: return "DCTYUVPlane load bad size";
    case MYYUV_E_PLANE_NBLK: return "DCTYUVPlane load chunks_sizes_size bad size";
    case MYYUV_E_PLANE_CONTENT: return "DCTYUVPlane load content_size bad size";
    case MYYUV_E_BAD_CODE: return "Huffman bad code";
    case MYYUV_E_UNKNOWN_SYMBOL: return "Huffman unknown symbol";
    case MYYUV_E_BAD_CHUNK: return "Huffman bad chunk";
    case MYYUV_E_HIP: return "HIP runtime error";
    case MYYUV_E_NO_DEVICE: return "No HIP device available";
    case MYYUV_E_BMP_INVALID: return "BMP is invalid";
    case MYYUV_E_BMP_SIGN: return "Unaccounted width and height sign";
    case MYYUV_E_BMP_UNSUPPORTED: return "BMP to IYUV needs 24 or 32 bits per pixel and even height";
    default: return "Unknown error";
  }
}

const char* myyuv_hip_error_message(int code) {
  if (code == MYYUV_E_TARGET) return "target not reachable";
  if (code == MYYUV_E_JPEG_DIM) return "JPEG width and height must not exceed 65535";
  if (code == MYYUV_E_JPEG_UNSUPPORTED) return "JPEG file is not a baseline 4:2:0 picture the container can hold";
  if (code == MYYUV_E_JPEG_SYNTAX) return "JPEG file is damaged";
  if (code == MYYUV_E_JPEG_DATA) return "JPEG entropy data is damaged";
  if (code == MYYUV_E_JPEG_TABLES) return "the file's tables are not the codec's: name a quality";
  return myyuv_hip_strerror(code);
}

uint64_t myyuv_jpeg_bound(uint32_t w, uint32_t h) { return myyuv_jpeg::file_bound(w, h); }

uint32_t myyuv_dct_payload_bound(uint32_t w, uint32_t h) {
  const uint64_t nb = (uint64_t)(w / 8) * (h / 8) + 2ull * (uint64_t)(w / 16) * (h / 16);
  const uint64_t b = 12 + 24 + nb + nb * kMaxChunk;
  return b > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)((b + 3) & ~3ull);
}

int myyuv_hip_create(int device, myyuv_hip_handle* out) {
  if (!out) return MYYUV_E_ARG;
  *out = nullptr;
  if (!hip_ok()) return MYYUV_E_NO_DEVICE;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return MYYUV_E_NO_DEVICE;
  DeviceGuard g(device);  // (declared before c: it outlives the context on a failure)
  auto c = std::make_unique<myyuv_hip_ctx>();
  c->device = device;
  if (hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->done.h, hipEventDisableTiming) != hipSuccess)
    return MYYUV_E_HIP;
  {
    int cus = 0, n1 = 0, n6 = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&n1, k_fdct_quant, 256, 0) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&n6, k_dequant_idct, 256, 0) == hipSuccess &&
        cus > 0 && n1 > 0 && n6 > 0) {
      c->xf_resident[0] = (uint32_t)(cus * n1);
      c->xf_resident[1] = (uint32_t)(cus * n6);
      int ncc = 0;
      c->xf_resident[2] = c->xf_resident[1];
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&ncc, k_coef_compare, 256, 0) == hipSuccess && ncc > 0)
        c->xf_resident[2] = (uint32_t)(cus * ncc);
      int nfix = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nfix, k_fdct_fix, 64 * kFixWaves, 0) == hipSuccess &&
          nfix > 0)
        c->fix_resident = (uint32_t)(cus * nfix) * kFixWaves / 4;  // (in 4-wave workgroups)
      if (const char* v = std::getenv("MYYUV_FIX_GRID")) c->fix_grid = (uint32_t)std::atoi(v);
      if (const char* v = std::getenv("MYYUV_FIX_QMAX")) c->fix_qmax = (uint32_t)std::atoi(v);
      if (const char* v = std::getenv("MYYUV_LAUNCH_BLOCKS"))
        c->launch_blocks = std::max(1u, std::min(kMaxLaunchBlocks, (uint32_t)std::strtoul(v, nullptr, 10)));
      {
        const char* v = std::getenv("MYYUV_ENCODER");
        c->fused = v && std::strcmp(v, "fused") == 0;
        const char* d = std::getenv("MYYUV_DECODER");
        c->fused_dec = !(d && std::strcmp(d, "split") == 0);
        // fused (or unset): spans from dec_span_min groups on; span / group: always / never
        if (const char* m = std::getenv("MYYUV_DEC_SPAN_MIN"))
          c->dec_span_min = (uint32_t)std::strtoul(m, nullptr, 10);
        if (d && std::strcmp(d, "span") == 0) c->dec_span_min = 0;
        if (d && std::strcmp(d, "group") == 0) c->dec_span_min = ~0u;
      }
      // tuning knobs (diagnostic; default 100): K1 / K6 grids as a percentage
      // of the resident workgroups, leaving wave slots to other launch groups
      for (int k = 0; k < 2; k++) {
        const char* v = std::getenv(k == 0 ? "MYYUV_K1_GRID_PCT" : "MYYUV_K6_GRID_PCT");
        const int pct = v ? std::atoi(v) : 100;
        if (pct > 0 && pct < 100) c->xf_resident[k] = std::max(1u, c->xf_resident[k] * (uint32_t)pct / 100u);
      }
    }
  }
  if (c->err.grow(8) || c->psize.grow(4) || c->desc.grow(sizeof(StreamDesc)) ||
      hipMemset(c->err.p, 0xFF, 8) != hipSuccess)
    return MYYUV_E_HIP;
  *out = c.release();
  return 0;
}

void myyuv_hip_destroy(myyuv_hip_handle c) {
  if (!c) return;
  DeviceGuard g(c->device);
  delete c;
}

int myyuv_hip_reserve(myyuv_hip_handle c, uint32_t w, uint32_t h) { return myyuv_hip_reserve_batch(c, w, h, 1); }

int myyuv_gpu_dct_compress_batch_device(myyuv_hip_handle c, const void* d_in, uint32_t nframes,
                                        uint32_t w, uint32_t h, const uint8_t q[3], void* d_out,
                                        uint32_t cap, uint32_t* d_sizes, void* stream) {
  return batch_device(true, c, const_cast<void*>(d_in), d_out, d_sizes, cap, nframes, w, h, q, stream);
}

int myyuv_gpu_dct_decompress_batch_device(myyuv_hip_handle c, const void* d_in, const uint32_t* d_sizes,
                                          uint32_t cap, uint32_t nframes, uint32_t w, uint32_t h,
                                          const uint8_t q[3], void* d_out, void* stream) {
  return batch_device(false, c, d_out, const_cast<void*>(d_in), const_cast<uint32_t*>(d_sizes), cap, nframes, w, h,
                      q, stream);
}

int myyuv_gpu_dct_compress_device(myyuv_hip_handle c, const void* d_in, uint32_t w, uint32_t h,
                                  const uint8_t q[3], void* d_out, uint32_t cap,
                                  uint32_t* d_size, void* stream) {
  return myyuv_gpu_dct_compress_batch_device(c, d_in, 1, w, h, q, d_out, cap, d_size, stream);
}

int myyuv_gpu_dct_decompress_device(myyuv_hip_handle c, const void* d_in, const uint32_t* d_size,
                                    uint32_t cap, uint32_t w, uint32_t h, const uint8_t q[3],
                                    void* d_out, void* stream) {
  return myyuv_gpu_dct_decompress_batch_device(c, d_in, d_size, cap, 1, w, h, q, d_out, stream);
}

int myyuv_hip_reserve_batch(myyuv_hip_handle c, uint32_t w, uint32_t h, uint32_t nframes) {
  if (!c) return MYYUV_E_ARG;
  FrameGeom G;
  int e = make_geom(w, h, G);
  if (e || (e = set_batch(G, nframes))) return e;
  std::lock_guard<std::mutex> lk(c->mu);
  if ((e = set_batch(G, std::min(nframes, launch_frames(G, c->launch_blocks))))) return e;  // (the largest launch)
  DeviceGuard g(c->device);
  return reserve(c, G);
}

// ---- K7: BMP -> IYUV (myyuv_yuv.cpp:88-128 over myyuv_bmp.cpp:77-101) ----
namespace {

// The checks the conversion itself makes, in the reference's order:
// YUV::load's isValid (width % 4 of isValidHeader; bit_count > 0), then
// colorData's sign cases, then the bmp_to_yuv_map asserts (even size,
// 32 bpp — 24 bpp converts the same way and is accepted).
int bmp_check(int32_t width, int32_t height, uint16_t bit_count, uint32_t* W, uint32_t* H,
              uint32_t* orient) {
  const uint32_t aw = width < 0 ? 0u - (uint32_t)width : (uint32_t)width;
  const uint32_t ah = height < 0 ? 0u - (uint32_t)height : (uint32_t)height;
  if (aw % 4 != 0 || bit_count == 0) return MYYUV_E_BMP_INVALID;
  if (width > 0 && height < 0)
    *orient = 0;
  else if (width < 0 && height > 0)
    *orient = 1;
  else if (width > 0 && height > 0)
    *orient = 2;
  else
    return MYYUV_E_BMP_SIGN;
  if ((bit_count != 24 && bit_count != 32) || ah % 2 != 0) return MYYUV_E_BMP_UNSUPPORTED;
  if ((uint64_t)aw * ah * 4 > 0xFFFFFFFFull) return MYYUV_E_ARG;  // imageSize() is a u32
  *W = aw;
  *H = ah;
  return 0;
}

int launch_bmp(myyuv_hip_ctx* c, const void* src, uint32_t W, uint32_t H, uint32_t orient,
               uint16_t bits, void* dst, hipStream_t s) {
  const uint32_t tiles = (W / 4) * (H / 2);
  if (tiles == 0) return 0;
  const uint32_t grid = std::min(ceil_div(tiles, 256), 8192u);
  const uint8_t* in = static_cast<const uint8_t*>(src);
  uint8_t* out = static_cast<uint8_t*>(dst);
  return bits == 32 ? launch(c, MYYUV_K_BMP, k_bmp_to_iyuv<4>, dim3(grid), dim3(256), s, in, W, H, orient, out)
                    : launch(c, MYYUV_K_BMP, k_bmp_to_iyuv<3>, dim3(grid), dim3(256), s, in, W, H, orient, out);
}

}  // namespace

int myyuv_gpu_bmp_to_iyuv_device(myyuv_hip_handle c, const void* d_bmp, int32_t width, int32_t height,
                                 uint16_t bit_count, void* d_iyuv, void* stream) {
  if (!c || !d_bmp || !d_iyuv) return MYYUV_E_ARG;
  uint32_t W = 0, H = 0, orient = 0;
  int e = bmp_check(width, height, bit_count, &W, &H, &orient);
  if (e) return e;
  Entry en(c, stream);
  hipStream_t s = en.s;
  return launch_bmp(c, d_bmp, W, H, orient, bit_count, d_iyuv, s);
}

int myyuv_gpu_bmp_to_iyuv(myyuv_hip_handle c, const uint8_t* bmp_data, int32_t width, int32_t height,
                          uint16_t bit_count, uint8_t* iyuv) {
  if (!c || !bmp_data || !iyuv) return MYYUV_E_ARG;
  uint32_t W = 0, H = 0, orient = 0;
  int e = bmp_check(width, height, bit_count, &W, &H, &orient);
  if (e) return e;
  Entry en(c);
  hipStream_t s = en.s;
  const size_t in_bytes = (size_t)W * H * (bit_count / 8), out_bytes = (size_t)W * H * 3 / 2;
  if (in_bytes == 0) return 0;
  if (c->bmp.grow(in_bytes) || c->frame.grow(out_bytes)) return MYYUV_E_HIP;
  if (h2d(c->bmp.p, bmp_data, in_bytes, s)) return MYYUV_E_HIP;
  if ((e = launch_bmp(c, c->bmp.p, W, H, orient, bit_count, c->frame.p, s))) return e;
  if (d2h(iyuv, c->frame.p, out_bytes, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

// ---- K8: IYUV -> BMP (the viewers' conversion; defined in myyuv_hip.h) ----
namespace {

// nf frames (frame f at src + f * W*H*3/2 -> dst + f * W*H*bits/8).  Four tile
// rows per workgroup, at most about 8192 workgroups striding over tile rows
// and frames.
int launch_to_bmp(myyuv_hip_ctx* c, const void* src, uint32_t W, uint32_t H, uint32_t nf, uint32_t orient,
                  uint16_t bits, uint32_t chroma, void* dst, hipStream_t s) {
  if (W == 0 || H == 0 || nf == 0) return 0;
  const uint32_t gx = ceil_div(W / 4, 64);
  const uint32_t gy = std::min(ceil_div(H / 2, 4), std::max(1u, 8192u / gx));
  const uint32_t gz = std::min(nf, std::max(1u, 8192u / (gx * gy)));
  const uint8_t* in = static_cast<const uint8_t*>(src);
  uint8_t* out = static_cast<uint8_t*>(dst);
  const dim3 grid(gx, gy, gz), block(64, 4);
  auto* k = bits == 32 ? (chroma ? k_iyuv_to_bmp<4, 1> : k_iyuv_to_bmp<4, 0>)
                       : (chroma ? k_iyuv_to_bmp<3, 1> : k_iyuv_to_bmp<3, 0>);
  return launch(c, MYYUV_K_IYUV_BMP, k, grid, block, s, in, W, H, nf, orient, out);
}

bool chroma_ok(uint32_t chroma) { return chroma == MYYUV_CHROMA_NEAREST || chroma == MYYUV_CHROMA_LINEAR; }

}  // namespace

int myyuv_gpu_iyuv_to_bmp_device(myyuv_hip_handle c, const void* d_iyuv, uint32_t nframes, int32_t width,
                                 int32_t height, uint16_t bit_count, uint32_t chroma, void* d_bmp, void* stream) {
  if (!d_iyuv || !d_bmp || nframes == 0 || !chroma_ok(chroma)) return MYYUV_E_ARG;
  uint32_t W = 0, H = 0, orient = 0;
  int e = bmp_check(width, height, bit_count, &W, &H, &orient);
  if (e) return e;
  // the kernel's dword luma loads and its 16-B / dword stores
  if (((uintptr_t)d_iyuv & 3) || ((uintptr_t)d_bmp & (bit_count == 32 ? 15 : 3))) return MYYUV_E_ARG;
  if (!c) return MYYUV_E_ARG;  // (last: the argument checks above need no context)
  Entry en(c, stream);
  return launch_to_bmp(c, d_iyuv, W, H, nframes, orient, bit_count, chroma, d_bmp, en.s);
}

int myyuv_gpu_iyuv_to_bmp(myyuv_hip_handle c, const uint8_t* iyuv, int32_t width, int32_t height,
                          uint16_t bit_count, uint32_t chroma, uint8_t* bmp_data) {
  if (!iyuv || !bmp_data || !chroma_ok(chroma)) return MYYUV_E_ARG;
  uint32_t W = 0, H = 0, orient = 0;
  int e = bmp_check(width, height, bit_count, &W, &H, &orient);
  if (e) return e;
  if (!c) return MYYUV_E_ARG;  // (last: the argument checks above need no context)
  Entry en(c);
  hipStream_t s = en.s;
  const size_t in_bytes = (size_t)W * H * 3 / 2, out_bytes = (size_t)W * H * (bit_count / 8);
  if (in_bytes == 0) return 0;
  if (c->frame.grow(in_bytes) || c->bmp.grow(out_bytes)) return MYYUV_E_HIP;
  if (h2d(c->frame.p, iyuv, in_bytes, s)) return MYYUV_E_HIP;
  if ((e = launch_to_bmp(c, c->frame.p, W, H, 1, orient, bit_count, chroma, c->bmp.p, s))) return e;
  if (d2h(bmp_data, c->bmp.p, out_bytes, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

int myyuv_hip_sync_status(myyuv_hip_handle c, void* stream, int64_t* bad_block) {
  if (!c) return MYYUV_E_ARG;
  Entry en(c, stream);
  hipStream_t s = en.s;
  int code = read_err(c, s, bad_block);
  if (reset_err(c, s) || hipStreamSynchronize(s) != hipSuccess) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return code;
}

int myyuv_gpu_dct_compress(myyuv_hip_handle c, const uint8_t* iyuv, uint32_t w, uint32_t h,
                           const uint8_t q[3], uint8_t* payload, uint32_t cap,
                           uint32_t* payload_size) {
  if (!c || !iyuv || !payload || !payload_size || !q) return MYYUV_E_ARG;
  FrameGeom G;
  int e = check_q(q);
  if (e || (e = make_geom(w, h, G))) return e;
  Entry en(c);
  hipStream_t s = en.s;
  const size_t fbytes = (size_t)w * h * 3 / 2;
  const uint32_t bound = myyuv_dct_payload_bound(w, h);
  if ((e = reserve(c, G)) || (e = set_qtables(c, q, s))) return e;
  if (c->frame.grow(fbytes) || c->payload.grow(bound)) return MYYUV_E_HIP;
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (h2d(c->frame.p, iyuv, fbytes, s)) return MYYUV_E_HIP;
  if ((e = launch_compress(c, G, c->frame.p, c->payload.p, bound, c->psize.as<uint32_t>(), s)))
    return e;
  uint32_t size = 0;
  if (hipMemcpyAsync(&size, c->psize.p, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return MYYUV_E_HIP;
  int64_t bad = -1;
  if ((e = read_err(c, s, &bad))) {
    (void)reset_err(c, s);
    return e;
  }
  *payload_size = size;
  if (size > cap) return MYYUV_E_CAPACITY;
  if (d2h(payload, c->payload.p, size, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

// ---- compress from BMP (include/myyuv_hip.h) ----
namespace {

// G.nframes pixel arrays (array f at d_bmp + f * W * H * bits / 8) -> payload f
// at d_out + f * cap.  k_bmp_fdct leaves K1's hand-off (quads, row masks, info
// words) for every block of the batch; then the encoder from K2 on, as
// launch_downscale runs it.  work[0] is zeroed here as K1 would have.  No IYUV
// frame, no K7, no K1, no fix kernel (K1's fix lists and their parity are not
// touched).  Workspace: reserve.
int launch_bmp_compress(myyuv_hip_ctx* c, const FrameGeom& G, const void* d_bmp, uint32_t orient, uint16_t bits,
                        void* d_out, uint32_t cap, uint32_t* d_size, hipStream_t s) {
  const uint32_t nf = G.nframes;
  const QTables* qt = c->qtd.as<const QTables>();
  unsigned long long* err = c->err.as<unsigned long long>();
  const myyuv_bmpfdct::Map M = myyuv_bmpfdct::make_map(G.pw[0], G.ph[0], orient);
  int e = 0;
  e |= hipMemsetAsync(c->work.p, 0, 4, s) != hipSuccess;
  e |= launch(c, MYYUV_K_BMP_FDCT, bits == 32 ? k_bmp_fdct<4> : k_bmp_fdct<3>, dim3(M.nstrips, nf), dim3(kWave), s,
              static_cast<const uint8_t*>(d_bmp), M, G, qt, c->coef.as<uint4>(), c->rmask.as<uint8_t>(),
              c->binfo.as<uint32_t>());
  e |= launch_huff_encode(c, G, s);
  e |= launch(c, MYYUV_K_SCAN, k_tile_scan, dim3(nf), dim3(256), s, c->tinfo.as<uint32_t>(), G,
              static_cast<uint8_t*>(d_out), cap, d_size, err);
  const uint32_t W = k2_win(nf * G.tcum[3]);  // (K2's windows, as launch_compress)
  e |= launch(c, MYYUV_K_COMPACT, k_stream_out, dim3(ceil_div(G.tcum[3] * nf, 8 * W) * 8 * W), dim3(256), s,
              c->stage.as<const uint32_t>(), c->tinfo.as<const uint32_t>(), c->sizes.as<const uint8_t>(),
              c->srcoff.as<const uint32_t>(), c->oslots.as<const uint32_t>(), G, static_cast<uint8_t*>(d_out), cap,
              W);
  return e ? MYYUV_E_HIP : 0;
}

}  // namespace

int myyuv_gpu_bmp_dct_compress(myyuv_hip_handle c, const uint8_t* bmp_data, int32_t width, int32_t height,
                               uint16_t bit_count, const uint8_t q[3], uint8_t* payload, uint32_t cap,
                               uint32_t* payload_size) {
  if (!c || !bmp_data || !payload || !payload_size || !q) return MYYUV_E_ARG;
  uint32_t w = 0, h = 0, orient = 0;
  FrameGeom G;
  int e = bmp_check(width, height, bit_count, &w, &h, &orient);
  if (e || (e = check_q(q)) || (e = make_geom(w, h, G))) return e;
  Entry en(c);
  hipStream_t s = en.s;
  const size_t in_bytes = (size_t)w * h * (bit_count / 8);
  const uint32_t bound = myyuv_dct_payload_bound(w, h);
  if ((e = reserve(c, G)) || (e = set_qtables(c, q, s))) return e;
  if (c->bmp.grow(in_bytes) || c->payload.grow(bound)) return MYYUV_E_HIP;
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (h2d(c->bmp.p, bmp_data, in_bytes, s)) return MYYUV_E_HIP;
  if ((e = launch_bmp_compress(c, G, c->bmp.p, orient, bit_count, c->payload.p, bound, c->psize.as<uint32_t>(), s)))
    return e;
  uint32_t size = 0;
  if (hipMemcpyAsync(&size, c->psize.p, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return MYYUV_E_HIP;
  int64_t bad = -1;
  if ((e = read_err(c, s, &bad))) {
    (void)reset_err(c, s);
    return e;
  }
  *payload_size = size;
  if (size > cap) return MYYUV_E_CAPACITY;
  if (d2h(payload, c->payload.p, size, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

int myyuv_gpu_bmp_dct_compress_device(myyuv_hip_handle c, const void* d_bmp, uint32_t nframes, int32_t width,
                                      int32_t height, uint16_t bit_count, const uint8_t q[3], void* d_payload,
                                      uint32_t cap, uint32_t* d_sizes, void* stream) {
  if (!c || !d_bmp || !d_payload || !d_sizes || !q) return MYYUV_E_ARG;
  uint32_t w = 0, h = 0, orient = 0;
  int e = bmp_check(width, height, bit_count, &w, &h, &orient);
  if (e) return e;
  // the kernel's 16-B / dword pixel loads; the stream writer's dword stores
  if (nframes == 0 || ((uintptr_t)d_bmp & (bit_count == 32 ? 15 : 3)) || ((uintptr_t)d_payload & 3) ||
      (nframes > 1 && (cap & 3)))
    return MYYUV_E_ARG;
  FrameGeom G;
  if ((e = check_q(q)) || (e = make_geom(w, h, G)) || (e = set_batch(G, nframes))) return e;
  Entry en(c, stream);
  // (as several launches when the batch's coefficient image would reach 4 GiB)
  const uint32_t per = launch_frames(G, c->launch_blocks);
  FrameGeom GL = G;
  if ((e = set_batch(GL, std::min(nframes, per))) || (e = reserve(c, GL)) || (e = set_qtables(c, q, en.s))) return e;
  const size_t in_bytes = (size_t)w * h * (bit_count / 8);
  for (uint32_t f0 = 0; f0 < nframes; f0 += per) {
    GL = G;
    GL.fbase = f0;
    if ((e = set_batch(GL, std::min(per, nframes - f0)))) return e;
    const uint8_t* px = static_cast<const uint8_t*>(d_bmp) + (size_t)f0 * in_bytes;
    uint8_t* pay = static_cast<uint8_t*>(d_payload) + (size_t)f0 * cap;
    if ((e = launch_bmp_compress(c, GL, px, orient, bit_count, pay, cap, d_sizes + f0, en.s))) return e;
  }
  return 0;
}

int myyuv_gpu_dct_decompress(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, uint32_t w,
                             uint32_t h, const uint8_t q[3], uint8_t* iyuv, int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payload || !iyuv || !q) return MYYUV_E_ARG;
  int e = check_q(q);
  if (e) return e;
  // DCTYUV::load / DCTYUVPlane::load checks (DCT.cpp:454 -> :130-159, :39-62)
  // come before the dimension checks in the reference: validate the stream
  // header on the host (the device re-checks it in k_scan_chain).
  FrameGeom G;
  if ((e = host_parse_headers(payload, size)) || (e = make_geom(w, h, G))) return e;
  Entry en(c);
  hipStream_t s = en.s;
  const uint32_t cap = (size + 3) & ~3u;
  const size_t fbytes = (size_t)w * h * 3 / 2;
  if ((e = reserve(c, G)) || (e = set_qtables(c, q, s))) return e;
  if (c->frame.grow(fbytes) || c->payload.grow(cap)) return MYYUV_E_HIP;
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (hipMemsetAsync(static_cast<uint8_t*>(c->payload.p) + (cap - 4), 0, 4, s) != hipSuccess ||
      h2d(c->payload.p, payload, size, s) ||
      hipMemcpyAsync(c->psize.p, &size, 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  if ((e = launch_decompress(c, G, c->payload.p, c->psize.as<const uint32_t>(), cap, c->frame.p, s)))
    return e;
  if ((e = read_err(c, s, bad_block))) {
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  if (d2h(iyuv, c->frame.p, fbytes, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

// myyuv_gpu_dct_decompress with K8 behind the decoder: the frame goes from
// the decoder to the conversion in the context's `frame` buffer.
int myyuv_gpu_dct_decompress_to_bmp(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, int32_t width,
                                    int32_t height, const uint8_t q[3], uint16_t bit_count, uint32_t chroma,
                                    uint8_t* bmp_data, int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payload || !bmp_data || !q || !chroma_ok(chroma)) return MYYUV_E_ARG;
  int e = check_q(q);
  if (e) return e;
  FrameGeom G;
  uint32_t w = 0, h = 0, orient = 0;
  if ((e = host_parse_headers(payload, size)) || (e = bmp_check(width, height, bit_count, &w, &h, &orient)) ||
      (e = make_geom(w, h, G)))
    return e;
  Entry en(c);
  hipStream_t s = en.s;
  const uint32_t cap = (size + 3) & ~3u;
  const size_t fbytes = (size_t)w * h * 3 / 2, out_bytes = (size_t)w * h * (bit_count / 8);
  if ((e = reserve(c, G)) || (e = set_qtables(c, q, s))) return e;
  if (c->frame.grow(fbytes) || c->payload.grow(cap) || c->bmp.grow(out_bytes)) return MYYUV_E_HIP;
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (hipMemsetAsync(static_cast<uint8_t*>(c->payload.p) + (cap - 4), 0, 4, s) != hipSuccess ||
      h2d(c->payload.p, payload, size, s) ||
      hipMemcpyAsync(c->psize.p, &size, 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  if ((e = launch_decompress(c, G, c->payload.p, c->psize.as<const uint32_t>(), cap, c->frame.p, s)) ||
      (e = launch_to_bmp(c, c->frame.p, w, h, 1, orient, bit_count, chroma, c->bmp.p, s)))
    return e;
  if ((e = read_err(c, s, bad_block))) {
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  if (d2h(bmp_data, c->bmp.p, out_bytes, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

// ---- region decode (defined in myyuv_hip.h) --------------------------------
namespace {

// The host-buffer region calls' device part: the whole stream goes up (the
// host cannot know the region's byte ranges), the region's frame is left in
// the context's `frame` buffer.
int region_to_frame(myyuv_hip_ctx* c, const uint8_t* payload, uint32_t size, const FrameGeom& G, const FrameGeom& R,
                    const RegionSegs& S, const uint8_t q[3], hipStream_t s) {
  int e;
  const uint32_t cap = (size + 3) & ~3u;
  if ((e = reserve_scan(c, G)) || (e = set_qtables(c, q, s))) return e;
  if (c->frame.grow(R.fbytes) || c->payload.grow(cap)) return MYYUV_E_HIP;
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (hipMemsetAsync(static_cast<uint8_t*>(c->payload.p) + (cap - 4), 0, 4, s) != hipSuccess ||
      h2d(c->payload.p, payload, size, s) ||
      hipMemcpyAsync(c->psize.p, &size, 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  return launch_decompress_region(c, G, R, S, c->payload.p, c->psize.as<const uint32_t>(), cap, c->frame.p, s);
}

}  // namespace

int myyuv_gpu_dct_decompress_region(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, uint32_t w,
                                    uint32_t h, const uint8_t q[3], uint32_t rx, uint32_t ry, uint32_t rw,
                                    uint32_t rh, uint8_t* iyuv, int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payload || !iyuv || !q) return MYYUV_E_ARG;
  int e = check_q(q);
  if (e) return e;
  FrameGeom G, R;
  RegionSegs S;
  if ((e = host_parse_headers(payload, size)) || (e = make_geom(w, h, G)) ||
      (e = make_region(w, h, rx, ry, rw, rh, R, S)))
    return e;
  Entry en(c);
  hipStream_t s = en.s;
  if ((e = region_to_frame(c, payload, size, G, R, S, q, s))) return e;
  if ((e = read_err(c, s, bad_block))) {
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  if (d2h(iyuv, c->frame.p, R.fbytes, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

int myyuv_gpu_dct_decompress_region_device(myyuv_hip_handle c, const void* d_payload, const uint32_t* d_sizes,
                                           uint32_t cap, uint32_t nframes, uint32_t w, uint32_t h,
                                           const uint8_t q[3], uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh,
                                           void* d_iyuv, void* stream) {
  if (!c || !d_payload || !d_sizes || !d_iyuv || !q) return MYYUV_E_ARG;
  if (((uintptr_t)d_payload & 3) || ((uintptr_t)d_iyuv & 7) || (nframes > 1 && (cap & 3))) return MYYUV_E_ARG;
  FrameGeom G, R;
  RegionSegs S;
  int e = check_q(q);
  if (e || (e = make_geom(w, h, G)) || (e = set_batch(G, nframes)) || (e = make_region(w, h, rx, ry, rw, rh, R, S)))
    return e;
  Entry en(c, stream);
  // (as several launches past the kernels' 32-bit block numbers or the grid's 65,535 frames)
  const uint32_t per = std::min(launch_frames(G, c->launch_blocks), 65535u);
  FrameGeom GL = G;
  if ((e = set_batch(GL, std::min(nframes, per))) || (e = reserve_scan(c, GL)) || (e = set_qtables(c, q, en.s)))
    return e;
  for (uint32_t f0 = 0; f0 < nframes; f0 += per) {
    GL = G;
    GL.fbase = f0;
    if ((e = set_batch(GL, std::min(per, nframes - f0)))) return e;
    const uint8_t* pay = static_cast<const uint8_t*>(d_payload) + (size_t)f0 * cap;
    uint8_t* fr = static_cast<uint8_t*>(d_iyuv) + (size_t)f0 * R.fbytes;
    if ((e = launch_decompress_region(c, GL, R, S, pay, d_sizes + f0, cap, fr, en.s))) return e;
  }
  return 0;
}

int myyuv_gpu_dct_decompress_region_to_bmp(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, int32_t width,
                                           int32_t height, const uint8_t q[3], uint32_t rx, uint32_t ry,
                                           uint32_t rw, uint32_t rh, uint16_t bit_count, uint32_t chroma,
                                           uint8_t* bmp_data, int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payload || !bmp_data || !q || !chroma_ok(chroma)) return MYYUV_E_ARG;
  int e = check_q(q);
  if (e) return e;
  FrameGeom G, R;
  RegionSegs S;
  uint32_t w = 0, h = 0, orient = 0;
  if ((e = host_parse_headers(payload, size)) || (e = bmp_check(width, height, bit_count, &w, &h, &orient)) ||
      (e = make_geom(w, h, G)) || (e = make_region(w, h, rx, ry, rw, rh, R, S)))
    return e;
  Entry en(c);
  hipStream_t s = en.s;
  const size_t out_bytes = (size_t)rw * rh * (bit_count / 8);
  if (c->bmp.grow(out_bytes)) return MYYUV_E_HIP;
  if ((e = region_to_frame(c, payload, size, G, R, S, q, s)) ||
      (e = launch_to_bmp(c, c->frame.p, rw, rh, 1, orient, bit_count, chroma, c->bmp.p, s)))
    return e;
  if ((e = read_err(c, s, bad_block))) {
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  if (d2h(bmp_data, c->bmp.p, out_bytes, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

// ---- scaled decode (defined in myyuv_hip.h) ---------------------------------
namespace {

// The host-buffer scaled calls' device part: the stream goes up, the scaled
// frame (G.fbytes / denom^2 bytes) is left in the context's `frame` buffer.
int scaled_to_frame(myyuv_hip_ctx* c, const uint8_t* payload, uint32_t size, const FrameGeom& G, uint32_t denom,
                    const uint8_t q[3], hipStream_t s) {
  int e;
  const uint32_t cap = (size + 3) & ~3u;
  if ((e = reserve_scaled(c, G)) || (e = set_qtables(c, q, s))) return e;
  if (c->frame.grow(G.fbytes / (denom * denom)) || c->payload.grow(cap)) return MYYUV_E_HIP;
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (hipMemsetAsync(static_cast<uint8_t*>(c->payload.p) + (cap - 4), 0, 4, s) != hipSuccess ||
      h2d(c->payload.p, payload, size, s) ||
      hipMemcpyAsync(c->psize.p, &size, 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  return launch_decompress_scaled(c, G, denom, c->payload.p, c->psize.as<const uint32_t>(), cap, c->frame.p, s);
}

}  // namespace

int myyuv_gpu_dct_decompress_scaled(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, uint32_t w,
                                    uint32_t h, const uint8_t q[3], uint32_t denom, uint8_t* iyuv,
                                    int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payload || !iyuv || !q) return MYYUV_E_ARG;
  int e = check_q(q);
  if (e) return e;
  FrameGeom G;
  if ((e = host_parse_headers(payload, size)) || (e = make_geom(w, h, G))) return e;
  if (!denom_ok(denom)) return MYYUV_E_ARG;
  Entry en(c);
  hipStream_t s = en.s;
  if ((e = scaled_to_frame(c, payload, size, G, denom, q, s))) return e;
  if ((e = read_err(c, s, bad_block))) {
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  if (d2h(iyuv, c->frame.p, G.fbytes / (denom * denom), s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

int myyuv_gpu_dct_decompress_scaled_device(myyuv_hip_handle c, const void* d_payload, const uint32_t* d_sizes,
                                           uint32_t cap, uint32_t nframes, uint32_t w, uint32_t h,
                                           const uint8_t q[3], uint32_t denom, void* d_iyuv, void* stream) {
  if (!c || !d_payload || !d_sizes || !d_iyuv || !q) return MYYUV_E_ARG;
  // (d_iyuv: the kernel's 2- and 4-byte row stores)
  if (((uintptr_t)d_payload & 3) || ((uintptr_t)d_iyuv & 3) || (nframes > 1 && (cap & 3))) return MYYUV_E_ARG;
  FrameGeom G;
  int e = check_q(q);
  if (e || (e = make_geom(w, h, G)) || (e = set_batch(G, nframes))) return e;
  if (!denom_ok(denom)) return MYYUV_E_ARG;
  Entry en(c, stream);
  // (as several launches past the kernels' 32-bit block numbers or the grid's 65,535 frames)
  const uint32_t per = std::min(launch_frames(G, c->launch_blocks), 65535u);
  FrameGeom GL = G;
  if ((e = set_batch(GL, std::min(nframes, per))) || (e = reserve_scaled(c, GL)) || (e = set_qtables(c, q, en.s)))
    return e;
  const size_t sbytes = G.fbytes / (denom * denom);
  for (uint32_t f0 = 0; f0 < nframes; f0 += per) {
    GL = G;
    GL.fbase = f0;
    if ((e = set_batch(GL, std::min(per, nframes - f0)))) return e;
    const uint8_t* pay = static_cast<const uint8_t*>(d_payload) + (size_t)f0 * cap;
    uint8_t* fr = static_cast<uint8_t*>(d_iyuv) + (size_t)f0 * sbytes;
    if ((e = launch_decompress_scaled(c, GL, denom, pay, d_sizes + f0, cap, fr, en.s))) return e;
  }
  return 0;
}

int myyuv_gpu_dct_decompress_scaled_to_bmp(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, int32_t width,
                                           int32_t height, const uint8_t q[3], uint32_t denom, uint16_t bit_count,
                                           uint32_t chroma, uint8_t* bmp_data, int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payload || !bmp_data || !q || !chroma_ok(chroma)) return MYYUV_E_ARG;
  int e = check_q(q);
  if (e) return e;
  FrameGeom G;
  const uint32_t w = width < 0 ? 0u - (uint32_t)width : (uint32_t)width;
  const uint32_t h = height < 0 ? 0u - (uint32_t)height : (uint32_t)height;
  if ((e = host_parse_headers(payload, size)) || (e = make_geom(w, h, G))) return e;
  if (!denom_ok(denom)) return MYYUV_E_ARG;
  // K8's checks on the scaled frame's signed header fields (exact: |width|
  // and |height| are multiples of 16)
  uint32_t sw = 0, sh = 0, orient = 0;
  if ((e = bmp_check(width / (int32_t)denom, height / (int32_t)denom, bit_count, &sw, &sh, &orient))) return e;
  Entry en(c);
  hipStream_t s = en.s;
  const size_t out_bytes = (size_t)sw * sh * (bit_count / 8);
  if (c->bmp.grow(out_bytes)) return MYYUV_E_HIP;
  if ((e = scaled_to_frame(c, payload, size, G, denom, q, s)) ||
      (e = launch_to_bmp(c, c->frame.p, sw, sh, 1, orient, bit_count, chroma, c->bmp.p, s)))
    return e;
  if ((e = read_err(c, s, bad_block))) {
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  if (d2h(bmp_data, c->bmp.p, out_bytes, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

// ---- compare (defined in myyuv_hip.h) ----------------------------------------
namespace {

void group_tiles(const FrameGeom& G, uint32_t& t0, uint32_t& t1, uint32_t& t2) {
  t0 = ceil_div(G.cum[1] - G.cum[0], kWave);
  t1 = ceil_div(G.cum[2] - G.cum[1], kWave);
  t2 = ceil_div(G.cum[3] - G.cum[2], kWave);
}

// The waves' totals of a launch of G.nframes frames (16 B per 64-block group).
int reserve_metric(myyuv_hip_ctx* c, const FrameGeom& G) {
  uint32_t t0, t1, t2;
  group_tiles(G, t0, t1, t2);
  return c->mpart.grow((size_t)G.nframes * (t0 + t1 + t2) * sizeof(uint4)) ? MYYUV_E_HIP : 0;
}

// The records from the waves' totals.  Every wave of the compare kernels
// writes its slot and k_metric_reduce writes every record whole: there is no
// accumulator that a call could find stale, and nothing to clear.
int launch_metric_reduce(myyuv_hip_ctx* c, const FrameGeom& G, myyuv_frame_metric* d_out, hipStream_t s) {
  uint32_t t0, t1, t2;
  group_tiles(G, t0, t1, t2);
  return launch(c, MYYUV_K_METRIC_SUM, k_metric_reduce, dim3(3, G.nframes), dim3(256), s,
                c->mpart.as<const uint4>(), t0, t1, t2, d_out);
}

// Two raw frames: test frame f at d_test + f * fbytes against reference frame
// f (ref_fbytes = fbytes) or frame 0 (ref_fbytes = 0) of d_ref.
int launch_frame_compare(myyuv_hip_ctx* c, const FrameGeom& G, const void* d_ref, uint32_t ref_fbytes,
                         const void* d_test, myyuv_frame_metric* d_out, myyuv_block_metric* d_map, hipStream_t s) {
  const uint32_t nf = G.nframes;
  uint32_t t0, t1, t2;
  group_tiles(G, t0, t1, t2);
  if (reserve_metric(c, G)) return MYYUV_E_HIP;
  int e = launch(c, MYYUV_K_FRAME_CMP, k_frame_compare, dim3(t0 + t1 + t2, nf), dim3(kWave), s,
              static_cast<const uint8_t*>(d_ref), ref_fbytes, static_cast<const uint8_t*>(d_test), G, t0, t1,
              c->mpart.as<uint4>(), d_map);
  e |= launch_metric_reduce(c, G, d_out, s);
  return e ? MYYUV_E_HIP : 0;
}

// A stream against a raw frame: the scan as launch_decompress runs it, then
// k_decode_compare on k_decode_idct's grid, whatever MYYUV_DECODER says (the
// split arrangement runs the same kernel).  Workspace: reserve_scaled.
int launch_dct_compare(myyuv_hip_ctx* c, const FrameGeom& G, const void* d_in, const uint32_t* d_size, uint32_t cap,
                       const void* d_ref, uint32_t ref_fbytes, myyuv_frame_metric* d_out, myyuv_block_metric* d_map,
                       hipStream_t s) {
  const uint32_t nf = G.nframes;
  const uint32_t ntiles = ceil_div(G.cum[3], kScanTile);
  unsigned long long* err = c->err.as<unsigned long long>();
  StreamDesc* desc = c->desc.as<StreamDesc>();
  const uint8_t* in = static_cast<const uint8_t*>(d_in);
  if (reserve_metric(c, G)) return MYYUV_E_HIP;
  int e = 0;
  ScanSrc SS;
  for (int i = 0; i < 4; i++) SS.cum[i] = G.cum[i];
  for (int p = 0; p < 3; p++) SS.pos[p] = 0;
  e |= launch(c, MYYUV_K_SCAN, k_scan_chain, dim3(ntiles, nf), dim3(256), s, in, cap, SS, d_size, cap, G, desc,
              c->loff.as<uint32_t>(), c->tiles.as<uint32_t>(), ntiles, c->status.as<unsigned long long>(),
              next_epoch(c), err);
  uint32_t t0, t1, t2;
  group_tiles(G, t0, t1, t2);
  e |= launch(c, MYYUV_K_COMPARE, k_decode_compare, dim3(t0 + t1 + t2, nf), dim3(kWave), s, in, d_size, cap,
              (const StreamDesc*)desc, c->loff.as<const uint32_t>(), c->tiles.as<const uint32_t>(), G, t0, t1,
              c->qtd.as<const QTables>(), c->coef.as<uint4>(), static_cast<const uint8_t*>(d_ref), ref_fbytes,
              c->mpart.as<uint4>(), d_map, err);
  e |= launch_metric_reduce(c, G, d_out, s);
  return e ? MYYUV_E_HIP : 0;
}

// The host-buffer calls' last step: the records (and the map) come back.
int compare_fetch(myyuv_hip_ctx* c, const FrameGeom& G, myyuv_frame_metric* out, myyuv_block_metric* map,
                  hipStream_t s) {
  myyuv_frame_metric m;
  if (map && hipMemcpyAsync(map, c->mmap.p, (size_t)G.cum[3] * sizeof(myyuv_block_metric), hipMemcpyDeviceToHost,
                            s) != hipSuccess)
    return MYYUV_E_HIP;
  if (d2h(&m, c->mrec.p, sizeof(m), s)) return MYYUV_E_HIP;
  *out = m;
  if (c->prof) drain_profile(c);
  return 0;
}

}  // namespace

double myyuv_metric_psnr(uint64_t sse, uint64_t nsamples) {
  if (sse == 0) return HUGE_VAL;
  return 10.0 * std::log10(65025.0 * (double)nsamples / (double)sse);
}

double myyuv_metric_ssim(int64_t ssim_sum, uint64_t nblocks) {
  return (double)ssim_sum / ((double)nblocks * 16777216.0);
}

int myyuv_gpu_iyuv_compare(myyuv_hip_handle c, const uint8_t* ref, const uint8_t* test, uint32_t w, uint32_t h,
                           myyuv_frame_metric* out, myyuv_block_metric* map) {
  if (out) std::memset(out, 0, sizeof(*out));
  if (!c || !ref || !test || !out) return MYYUV_E_ARG;
  FrameGeom G;
  int e = make_geom(w, h, G);
  if (e) return e;
  Entry en(c);
  hipStream_t s = en.s;
  if (c->frame.grow(G.fbytes) || c->mtest.grow(G.fbytes) || c->mrec.grow(sizeof(myyuv_frame_metric)) ||
      (map && c->mmap.grow((size_t)G.cum[3] * sizeof(myyuv_block_metric))))
    return MYYUV_E_HIP;
  if (h2d(c->frame.p, ref, G.fbytes, s) || h2d(c->mtest.p, test, G.fbytes, s)) return MYYUV_E_HIP;
  if ((e = launch_frame_compare(c, G, c->frame.p, 0, c->mtest.p, c->mrec.as<myyuv_frame_metric>(),
                                map ? c->mmap.as<myyuv_block_metric>() : nullptr, s)))
    return e;
  return compare_fetch(c, G, out, map, s);
}

int myyuv_gpu_iyuv_compare_device(myyuv_hip_handle c, const void* d_ref, const void* d_test, uint32_t nframes,
                                  uint32_t ref_frames, uint32_t w, uint32_t h, myyuv_frame_metric* d_out,
                                  myyuv_block_metric* d_map, void* stream) {
  if (!c || !d_ref || !d_test || !d_out || nframes == 0 || (ref_frames != 1 && ref_frames != nframes))
    return MYYUV_E_ARG;
  if (((uintptr_t)d_ref & 7) || ((uintptr_t)d_test & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_map & 7))
    return MYYUV_E_ARG;
  FrameGeom G;
  int e;
  if ((e = make_geom(w, h, G)) || (e = set_batch(G, nframes))) return e;
  Entry en(c, stream);
  // (the grid's 65,535 frames)
  const uint32_t per = 65535u;
  for (uint32_t f0 = 0; f0 < nframes; f0 += per) {
    FrameGeom GL = G;
    if ((e = set_batch(GL, std::min(per, nframes - f0)))) return e;
    const uint32_t rfb = ref_frames == 1 ? 0u : G.fbytes;
    const uint8_t* rf = static_cast<const uint8_t*>(d_ref) + (size_t)f0 * rfb;
    const uint8_t* tf = static_cast<const uint8_t*>(d_test) + (size_t)f0 * G.fbytes;
    if ((e = launch_frame_compare(c, GL, rf, rfb, tf, d_out + f0, d_map ? d_map + (size_t)f0 * G.cum[3] : nullptr,
                                  en.s)))
      return e;
  }
  return 0;
}

int myyuv_gpu_dct_compare(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, uint32_t w, uint32_t h,
                          const uint8_t q[3], const uint8_t* ref_iyuv, myyuv_frame_metric* out,
                          myyuv_block_metric* map, int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (out) std::memset(out, 0, sizeof(*out));
  if (!c || !payload || !ref_iyuv || !out || !q) return MYYUV_E_ARG;
  int e = check_q(q);
  if (e) return e;
  FrameGeom G;
  if ((e = host_parse_headers(payload, size)) || (e = make_geom(w, h, G))) return e;
  Entry en(c);
  hipStream_t s = en.s;
  const uint32_t cap = (size + 3) & ~3u;
  if ((e = reserve_scaled(c, G)) || (e = set_qtables(c, q, s))) return e;
  if (c->frame.grow(G.fbytes) || c->payload.grow(cap) || c->psize.grow(4) ||
      c->mrec.grow(sizeof(myyuv_frame_metric)) ||
      (map && c->mmap.grow((size_t)G.cum[3] * sizeof(myyuv_block_metric))))
    return MYYUV_E_HIP;
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (hipMemsetAsync(static_cast<uint8_t*>(c->payload.p) + (cap - 4), 0, 4, s) != hipSuccess ||
      h2d(c->payload.p, payload, size, s) || h2d(c->frame.p, ref_iyuv, G.fbytes, s) ||
      hipMemcpyAsync(c->psize.p, &size, 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  if ((e = launch_dct_compare(c, G, c->payload.p, c->psize.as<const uint32_t>(), cap, c->frame.p, 0,
                              c->mrec.as<myyuv_frame_metric>(), map ? c->mmap.as<myyuv_block_metric>() : nullptr,
                              s)))
    return e;
  if ((e = read_err(c, s, bad_block))) {
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  return compare_fetch(c, G, out, map, s);
}

int myyuv_gpu_dct_compare_device(myyuv_hip_handle c, const void* d_payload, const uint32_t* d_sizes, uint32_t cap,
                                 uint32_t nframes, uint32_t w, uint32_t h, const uint8_t q[3], const void* d_ref,
                                 uint32_t ref_frames, myyuv_frame_metric* d_out, myyuv_block_metric* d_map,
                                 void* stream) {
  if (!c || !d_payload || !d_sizes || !d_ref || !d_out || !q || (ref_frames != 1 && ref_frames != nframes))
    return MYYUV_E_ARG;
  if (((uintptr_t)d_payload & 3) || ((uintptr_t)d_ref & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_map & 7) ||
      (nframes > 1 && (cap & 3)))
    return MYYUV_E_ARG;
  FrameGeom G;
  int e = check_q(q);
  if (e || (e = make_geom(w, h, G)) || (e = set_batch(G, nframes))) return e;
  Entry en(c, stream);
  // (as several launches past the kernels' 32-bit block numbers or the grid's 65,535 frames)
  const uint32_t per = std::min(launch_frames(G, c->launch_blocks), 65535u);
  FrameGeom GL = G;
  if ((e = set_batch(GL, std::min(nframes, per))) || (e = reserve_scaled(c, GL)) || (e = set_qtables(c, q, en.s)))
    return e;
  const uint32_t rfb = ref_frames == 1 ? 0u : G.fbytes;
  for (uint32_t f0 = 0; f0 < nframes; f0 += per) {
    GL = G;
    GL.fbase = f0;
    if ((e = set_batch(GL, std::min(per, nframes - f0)))) return e;
    const uint8_t* pay = static_cast<const uint8_t*>(d_payload) + (size_t)f0 * cap;
    const uint8_t* rf = static_cast<const uint8_t*>(d_ref) + (size_t)f0 * rfb;
    if ((e = launch_dct_compare(c, GL, pay, d_sizes + f0, cap, rf, rfb, d_out + f0,
                                d_map ? d_map + (size_t)f0 * G.cum[3] : nullptr, en.s)))
      return e;
  }
  return 0;
}

// ---- probe and encode to a target (defined in myyuv_hip.h) -------------------
namespace {

bool what_ok(uint32_t what) { return what >= 1 && what <= (MYYUV_PROBE_SIZE | MYYUV_PROBE_METRIC); }

// The probe's scratch for a launch of nf frames: 12 head bytes per frame, the
// payload sizes, the scan's error word (8-byte aligned).
size_t probe_sizes_at(uint32_t nf) { return (size_t)nf * 12; }
size_t probe_err_at(uint32_t nf) { return ((size_t)nf * 16 + 7) & ~(size_t)7; }

// Workspace of a probe of G.nframes frames: the compress calls', the units'
// totals (16 B per 16-block unit) and the plane records.
int reserve_probe(myyuv_hip_ctx* c, const FrameGeom& G, uint32_t what) {
  const uint32_t nf = G.nframes;
  int e = reserve(c, G);
  e |= c->pbsz.grow(probe_err_at(nf) + 8);
  if (what & MYYUV_PROBE_METRIC) {
    e |= c->mpart.grow((size_t)nf * G.ucum[3] * sizeof(uint4));
    e |= c->mrec.grow((size_t)nf * sizeof(myyuv_frame_metric));
  }
  return e ? MYYUV_E_HIP : 0;
}

// One launch group of a probe: frame f at d_in + f * fbytes -> d_out[f] (and
// its part of the map).  Size: the encoder as launch_compress runs it, up to
// the tile scan, which is given a 12-byte "stream" per frame (it writes the
// three plane sizes there, skips the plane headers, and reports the size; its
// capacity overflow goes to an error word of the probe's own).  Metric: K1
// (once, when the split encoder's size part ran it already), k_coef_compare
// on K6's grid, k_metric_reduce over the planes' unit counts.
int launch_probe(myyuv_hip_ctx* c, const FrameGeom& G, const void* d_in, uint32_t what, myyuv_probe* d_out,
                 myyuv_block_metric* d_map, hipStream_t s) {
  const uint32_t nf = G.nframes;
  const QTables* qt = c->qtd.as<const QTables>();
  const uint8_t* in = static_cast<const uint8_t*>(d_in);
  uint8_t* heads = c->pbsz.as<uint8_t>();
  uint32_t* sizes = reinterpret_cast<uint32_t*>(heads + probe_sizes_at(nf));
  unsigned long long* scan_err = reinterpret_cast<unsigned long long*>(heads + probe_err_at(nf));
  int e = 0;
  bool have_coef = false;
  if (what & MYYUV_PROBE_SIZE) {
    if (c->fused) {
      uint32_t* count = c->work.as<uint32_t>();
      e |= hipMemsetAsync(count, 0, 4, s) != hipSuccess;
      e |= launch(c, MYYUV_K_ENCODE_TILE, k_encode_tile, dim3(G.tcum[3], nf), dim3(kK2Group), s, in, G, qt,
                  c->coef.as<uint4>(), c->rmask.as<uint8_t>(), c->stage.as<uint32_t>(), c->tinfo.as<uint32_t>(),
                  c->sizes.as<uint8_t>(), c->srcoff.as<uint32_t>(), count + 64, count);
      e |= launch_overflow(c, G, s);
    } else {
      e |= launch_fdct(c, G, in, qt, c->work.as<uint32_t>(), s);
      if ((c->skip >> MYYUV_K_FDCT) & 1u) e |= hipMemsetAsync(c->work.p, 0, 4, s) != hipSuccess;  // (see launch_compress)
      e |= launch_huff_encode(c, G, s);
      have_coef = true;
    }
    e |= launch(c, MYYUV_K_SCAN, k_tile_scan, dim3(nf), dim3(256), s, c->tinfo.as<uint32_t>(), G, heads, 12u, sizes,
                scan_err);
  }
  if (what & MYYUV_PROBE_METRIC) {
    if (!have_coef) e |= launch_fdct(c, G, in, qt, nullptr, s);
    e |= launch(c, MYYUV_K_COEF_CMP, k_coef_compare, xf_grid(G, c->xf_resident[2]), dim3(256), s,
                c->coef.as<const uint4>(), c->rmask.as<const uint8_t>(), c->zq.as<const uint4>(), G, qt, in,
                c->mpart.as<uint4>(), d_map, c->sink.as<uint4>());
    e |= launch(c, MYYUV_K_METRIC_SUM, k_metric_reduce, dim3(3, nf), dim3(256), s, c->mpart.as<const uint4>(),
                G.ucum[1] - G.ucum[0], G.ucum[2] - G.ucum[1], G.ucum[3] - G.ucum[2], c->mrec.as<myyuv_frame_metric>());
  }
  e |= launch(c, MYYUV_K_PROBE_OUT, k_probe_out, dim3(ceil_div(nf, 64)), dim3(64), s,
              reinterpret_cast<const uint32_t*>(heads), (const uint32_t*)sizes,
              c->mrec.as<const myyuv_frame_metric>(), what, nf, d_out);
  return e ? MYYUV_E_HIP : 0;
}

// One frame on the device at quality q: the record read back (the search's
// step; synchronous).  Workspace: reserve_probe, c->prec.
int probe_once(myyuv_hip_ctx* c, const FrameGeom& G, const void* d_frame, const uint8_t q[3], uint32_t what,
               myyuv_block_metric* d_map, hipStream_t s, myyuv_probe* out) {
  int e;
  if ((e = set_qtables(c, q, s)) || (e = launch_probe(c, G, d_frame, what, c->prec.as<myyuv_probe>(), d_map, s)))
    return e;
  return d2h(out, c->prec.p, sizeof(*out), s);
}

// The search over probes of the frame at d_frame, then (unless the target is
// out of reach) the ordinary compress at the chosen qualities into d_payload.
// Synchronous up to the compress launch.
int target_search(myyuv_hip_ctx* c, const FrameGeom& G, const void* d_frame, myyuv_rate::Search& S, void* d_payload,
                  uint32_t cap, uint32_t* d_size, myyuv_target_result* result, hipStream_t s) {
  int e;
  if ((e = reserve_probe(c, G, MYYUV_PROBE_SIZE | MYYUV_PROBE_METRIC)) || c->prec.grow(sizeof(myyuv_probe)))
    return e ? e : MYYUV_E_HIP;
  // What the search's probes said, by quality: the sizes of (q, q, q) in size
  // mode, plane p's record at its quality q in distortion mode (a plane's
  // figures depend on its own quality alone).  The result's qualities were
  // all probed (each is 1, 100, or a mid that became lo or hi), so `at` takes
  // that part from here and the other part from one launch after the search.
  std::vector<myyuv_probe> seen(101);
  uint8_t q[3];
  myyuv_probe pr;
  while (S.next(q)) {
    if ((e = probe_once(c, G, d_frame, q, S.size_mode ? MYYUV_PROBE_SIZE : MYYUV_PROBE_METRIC, nullptr, s, &pr)))
      return e;
    const uint64_t sse[3] = {pr.metric.plane[0].sse, pr.metric.plane[1].sse, pr.metric.plane[2].sse};
    if (S.size_mode) {
      std::memcpy(seen[q[0]].plane_bytes, pr.plane_bytes, sizeof(pr.plane_bytes));
      seen[q[0]].payload_bytes = pr.payload_bytes;
    } else {
      for (int p = 0; p < 3; p++) seen[q[p]].metric.plane[p] = pr.metric.plane[p];
    }
    S.answer(pr.payload_bytes, sse);
  }
  std::memcpy(result->quality, S.quality, 3);
  result->failed_planes = S.failed_planes;
  result->probes = S.probes;
  if ((e = probe_once(c, G, d_frame, S.quality, S.size_mode ? MYYUV_PROBE_METRIC : MYYUV_PROBE_SIZE, nullptr, s,
                      &result->at)))
    return e;
  if (S.size_mode) {
    std::memcpy(result->at.plane_bytes, seen[S.quality[0]].plane_bytes, sizeof(pr.plane_bytes));
    result->at.payload_bytes = seen[S.quality[0]].payload_bytes;
  } else {
    for (int p = 0; p < 3; p++) result->at.metric.plane[p] = seen[S.quality[p]].metric.plane[p];
  }
  if (S.failed) return MYYUV_E_TARGET;
  if ((e = set_qtables(c, S.quality, s))) return e;
  return launch_compress(c, G, d_frame, d_payload, cap, d_size, s);
}

int target_host(myyuv_hip_ctx* c, const uint8_t* iyuv, uint32_t w, uint32_t h, myyuv_rate::Search& S,
                uint8_t* payload, uint32_t cap, uint32_t* payload_size, myyuv_target_result* result) {
  if (result) std::memset(result, 0, sizeof(*result));
  if (!c || !iyuv || !payload || !payload_size || !result) return MYYUV_E_ARG;
  FrameGeom G;
  int e = make_geom(w, h, G);
  if (e) return e;
  Entry en(c);
  hipStream_t s = en.s;
  const uint32_t bound = myyuv_dct_payload_bound(w, h);
  if (c->frame.grow(G.fbytes) || c->payload.grow(bound)) return MYYUV_E_HIP;
  if (reset_err(c, s) || h2d(c->frame.p, iyuv, G.fbytes, s)) return MYYUV_E_HIP;
  e = target_search(c, G, c->frame.p, S, c->payload.p, bound, c->psize.as<uint32_t>(), result, s);
  if (e) {
    if (c->prof) drain_profile(c);
    return e;
  }
  uint32_t size = 0;
  if (d2h(&size, c->psize.p, 4, s)) return MYYUV_E_HIP;
  if ((e = read_err(c, s, nullptr))) {
    (void)reset_err(c, s);
    return e;
  }
  *payload_size = size;
  if (size > cap) return MYYUV_E_CAPACITY;
  if (d2h(payload, c->payload.p, size, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

int target_device(myyuv_hip_ctx* c, const void* d_iyuv, uint32_t w, uint32_t h, myyuv_rate::Search& S,
                  void* d_payload, uint32_t cap, uint32_t* d_payload_size, myyuv_target_result* result,
                  void* stream) {
  if (result) std::memset(result, 0, sizeof(*result));
  if (!c || !d_iyuv || !d_payload || !d_payload_size || !result) return MYYUV_E_ARG;
  if (((uintptr_t)d_payload & 3) || ((uintptr_t)d_iyuv & 7)) return MYYUV_E_ARG;
  FrameGeom G;
  int e = make_geom(w, h, G);
  if (e) return e;
  Entry en(c, stream);
  if ((e = target_search(c, G, d_iyuv, S, d_payload, cap, d_payload_size, result, en.s))) return e;
  if (hipStreamSynchronize(en.s) != hipSuccess) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

}  // namespace

uint64_t myyuv_metric_sse_for_psnr(double db, uint64_t nsamples) {
  return myyuv_rate::sse_for_psnr(db, nsamples, myyuv_metric_psnr);
}

int myyuv_gpu_dct_probe(myyuv_hip_handle c, const uint8_t* iyuv, uint32_t w, uint32_t h, const uint8_t q[3],
                        uint32_t what, myyuv_probe* out, myyuv_block_metric* map) {
  if (out) std::memset(out, 0, sizeof(*out));
  if (!c || !iyuv || !out || !q) return MYYUV_E_ARG;
  FrameGeom G;
  int e = check_q(q);
  if (e || (e = make_geom(w, h, G))) return e;
  if (!what_ok(what)) return MYYUV_E_ARG;
  Entry en(c);
  hipStream_t s = en.s;
  const bool with_map = map && (what & MYYUV_PROBE_METRIC);
  if ((e = reserve_probe(c, G, what))) return e;
  if (c->frame.grow(G.fbytes) || c->prec.grow(sizeof(myyuv_probe)) ||
      (with_map && c->mmap.grow((size_t)G.cum[3] * sizeof(myyuv_block_metric))))
    return MYYUV_E_HIP;
  if (h2d(c->frame.p, iyuv, G.fbytes, s)) return MYYUV_E_HIP;
  myyuv_probe r;
  if ((e = set_qtables(c, q, s)) ||
      (e = launch_probe(c, G, c->frame.p, what, c->prec.as<myyuv_probe>(),
                        with_map ? c->mmap.as<myyuv_block_metric>() : nullptr, s)))
    return e;
  if (with_map && hipMemcpyAsync(map, c->mmap.p, (size_t)G.cum[3] * sizeof(myyuv_block_metric),
                                 hipMemcpyDeviceToHost, s) != hipSuccess)
    return MYYUV_E_HIP;
  if (d2h(&r, c->prec.p, sizeof(r), s)) return MYYUV_E_HIP;
  *out = r;
  if (c->prof) drain_profile(c);
  return 0;
}

int myyuv_gpu_dct_probe_device(myyuv_hip_handle c, const void* d_iyuv, uint32_t nframes, uint32_t w, uint32_t h,
                               const uint8_t q[3], uint32_t what, myyuv_probe* d_out, myyuv_block_metric* d_map,
                               void* stream) {
  if (!c || !d_iyuv || !d_out || !q) return MYYUV_E_ARG;
  if (((uintptr_t)d_iyuv & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_map & 7)) return MYYUV_E_ARG;
  FrameGeom G;
  int e = check_q(q);
  if (e || (e = make_geom(w, h, G)) || (e = set_batch(G, nframes))) return e;
  if (!what_ok(what)) return MYYUV_E_ARG;
  Entry en(c, stream);
  // (as several launches when the batch's coefficient image would reach 4 GiB; k_metric_reduce's grid: 65,535 frames)
  const uint32_t per = std::min(launch_frames(G, c->launch_blocks), 65535u);
  FrameGeom GL = G;
  if ((e = set_batch(GL, std::min(nframes, per))) || (e = reserve_probe(c, GL, what)) ||
      (e = set_qtables(c, q, en.s)))
    return e;
  if (!(what & MYYUV_PROBE_METRIC)) d_map = nullptr;
  for (uint32_t f0 = 0; f0 < nframes; f0 += per) {
    GL = G;
    GL.fbase = f0;
    if ((e = set_batch(GL, std::min(per, nframes - f0)))) return e;
    const uint8_t* fr = static_cast<const uint8_t*>(d_iyuv) + (size_t)f0 * G.fbytes;
    if ((e = launch_probe(c, GL, fr, what, d_out + f0, d_map ? d_map + (size_t)f0 * G.cum[3] : nullptr, en.s)))
      return e;
  }
  return 0;
}

int myyuv_gpu_dct_compress_to_size(myyuv_hip_handle c, const uint8_t* iyuv, uint32_t w, uint32_t h,
                                   uint32_t max_payload_bytes, uint8_t* payload, uint32_t cap,
                                   uint32_t* payload_size, myyuv_target_result* result) {
  myyuv_rate::Search S = myyuv_rate::Search::size(max_payload_bytes);
  return target_host(c, iyuv, w, h, S, payload, cap, payload_size, result);
}

int myyuv_gpu_dct_compress_to_sse(myyuv_hip_handle c, const uint8_t* iyuv, uint32_t w, uint32_t h,
                                  const uint64_t max_sse[3], uint8_t* payload, uint32_t cap, uint32_t* payload_size,
                                  myyuv_target_result* result) {
  if (result) std::memset(result, 0, sizeof(*result));
  if (!max_sse) return MYYUV_E_ARG;
  myyuv_rate::Search S = myyuv_rate::Search::sse(max_sse);
  return target_host(c, iyuv, w, h, S, payload, cap, payload_size, result);
}

int myyuv_gpu_dct_compress_to_size_device(myyuv_hip_handle c, const void* d_iyuv, uint32_t w, uint32_t h,
                                          uint32_t max_payload_bytes, void* d_payload, uint32_t cap,
                                          uint32_t* d_payload_size, myyuv_target_result* result, void* stream) {
  myyuv_rate::Search S = myyuv_rate::Search::size(max_payload_bytes);
  return target_device(c, d_iyuv, w, h, S, d_payload, cap, d_payload_size, result, stream);
}

int myyuv_gpu_dct_compress_to_sse_device(myyuv_hip_handle c, const void* d_iyuv, uint32_t w, uint32_t h,
                                         const uint64_t max_sse[3], void* d_payload, uint32_t cap,
                                         uint32_t* d_payload_size, myyuv_target_result* result, void* stream) {
  if (result) std::memset(result, 0, sizeof(*result));
  if (!max_sse) return MYYUV_E_ARG;
  myyuv_rate::Search S = myyuv_rate::Search::sse(max_sse);
  return target_device(c, d_iyuv, w, h, S, d_payload, cap, d_payload_size, result, stream);
}

// ---- requantise and transform (defined in myyuv_hip.h) ----------------------
namespace {

// Both host-buffer calls; op < 0: requantise.
int recode_host(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, uint32_t w, uint32_t h,
                const uint8_t q_src[3], int op, const uint8_t q_dst[3], uint8_t* out, uint32_t cap,
                uint32_t* out_size, int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payload || !out || !out_size || !q_src || !q_dst || op > 7) return MYYUV_E_ARG;
  int e = check_q(q_src);
  if (e) return e;
  FrameGeom G, Gd;
  if ((e = host_parse_headers(payload, size)) || (e = make_geom(w, h, G)) || (e = check_q(q_dst))) return e;
  if (op >= 0 && (e = xform_geom(G, w, h, (uint32_t)op, Gd))) return e;
  Entry en(c);
  hipStream_t s = en.s;
  const uint32_t cap_in = (size + 3) & ~3u;
  // the device writes into a buffer of the bound's size, so a result larger
  // than the caller's `cap` is known by its size alone (as compress)
  const uint32_t bound = myyuv_dct_payload_bound(w, h);
  if ((e = reserve(c, G)) || (op >= 0 && (e = reserve_xform(c, G))) ||
      (e = set_requant_tables(c, q_src, q_dst, s, op >= 0 && MYYUV_XF_SWAPS(op))))
    return e;
  if (c->rqsrc.grow(cap_in) || c->payload.grow(bound) || c->psize.grow(8)) return MYYUV_E_HIP;
  uint32_t* psz = c->psize.as<uint32_t>();  // [0] the source's size, [1] the result's
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (hipMemsetAsync(static_cast<uint8_t*>(c->rqsrc.p) + (cap_in - 4), 0, 4, s) != hipSuccess ||
      h2d(c->rqsrc.p, payload, size, s) || hipMemcpyAsync(psz, &size, 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  e = op < 0 ? launch_requant(c, G, c->rqsrc.p, psz, cap_in, c->payload.p, bound, psz + 1, s)
             : launch_coef_xform(c, G, Gd, (uint32_t)op, c->rqsrc.p, psz, cap_in, c->payload.p, bound, psz + 1, s);
  if (e) return e;
  uint32_t nout = 0;
  if (hipMemcpyAsync(&nout, psz + 1, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return MYYUV_E_HIP;
  if ((e = read_err(c, s, bad_block))) {  // (synchronises)
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  *out_size = nout;
  if (nout > cap) return MYYUV_E_CAPACITY;
  if (d2h(out, c->payload.p, nout, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

// Both device-resident batches; op < 0: requantise.
int recode_device(myyuv_hip_handle c, const void* d_payload, const uint32_t* d_payload_sizes, uint32_t cap_in,
                  uint32_t nframes, uint32_t w, uint32_t h, const uint8_t q_src[3], int op, const uint8_t q_dst[3],
                  void* d_out, uint32_t cap_out, uint32_t* d_out_sizes, void* stream) {
  if (!c || !d_payload || !d_payload_sizes || !d_out || !d_out_sizes || !q_src || !q_dst || op > 7)
    return MYYUV_E_ARG;
  FrameGeom G;
  int e = check_q(q_src);
  if (e || (e = make_geom(w, h, G)) || (e = set_batch(G, nframes)) || (e = check_q(q_dst))) return e;
  if (((uintptr_t)d_payload & 3) || ((uintptr_t)d_out & 3) || (nframes > 1 && ((cap_in | cap_out) & 3)))
    return MYYUV_E_ARG;
  {  // the two stream arrays must not overlap: K4 writes frame f while later frames are still being read
    const uintptr_t a = (uintptr_t)d_payload, b = (uintptr_t)d_out;
    const uint64_t na = (uint64_t)cap_in * nframes, nb = (uint64_t)cap_out * nframes;
    if (a < b + nb && b < a + na) return MYYUV_E_ARG;
  }
  Entry en(c, stream);
  // (as several launches past the kernels' 32-bit block numbers or the grid's 65,535 frames)
  const uint32_t per = std::min(launch_frames(G, c->launch_blocks), 65535u);
  FrameGeom GL = G, GD;
  if ((e = set_batch(GL, std::min(nframes, per))) || (e = reserve(c, GL)) ||
      (op >= 0 && (e = reserve_xform(c, GL))) ||
      (e = set_requant_tables(c, q_src, q_dst, en.s, op >= 0 && MYYUV_XF_SWAPS(op))))
    return e;
  for (uint32_t f0 = 0; f0 < nframes; f0 += per) {
    GL = G;
    GL.fbase = f0;
    if ((e = set_batch(GL, std::min(per, nframes - f0)))) return e;
    const uint8_t* src = static_cast<const uint8_t*>(d_payload) + (size_t)f0 * cap_in;
    uint8_t* dst = static_cast<uint8_t*>(d_out) + (size_t)f0 * cap_out;
    if (op < 0)
      e = launch_requant(c, GL, src, d_payload_sizes + f0, cap_in, dst, cap_out, d_out_sizes + f0, en.s);
    else if (!(e = xform_geom(GL, w, h, (uint32_t)op, GD)))
      e = launch_coef_xform(c, GL, GD, (uint32_t)op, src, d_payload_sizes + f0, cap_in, dst, cap_out,
                            d_out_sizes + f0, en.s);
    if (e) return e;
  }
  return 0;
}

}  // namespace

int myyuv_gpu_dct_requantize(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, uint32_t w, uint32_t h,
                             const uint8_t q_src[3], const uint8_t q_dst[3], uint8_t* out, uint32_t cap,
                             uint32_t* out_size, int64_t* bad_block) {
  return recode_host(c, payload, size, w, h, q_src, -1, q_dst, out, cap, out_size, bad_block);
}

int myyuv_gpu_dct_requantize_device(myyuv_hip_handle c, const void* d_payload, const uint32_t* d_payload_sizes,
                                    uint32_t cap_in, uint32_t nframes, uint32_t w, uint32_t h,
                                    const uint8_t q_src[3], const uint8_t q_dst[3], void* d_out, uint32_t cap_out,
                                    uint32_t* d_out_sizes, void* stream) {
  return recode_device(c, d_payload, d_payload_sizes, cap_in, nframes, w, h, q_src, -1, q_dst, d_out, cap_out,
                       d_out_sizes, stream);
}

int myyuv_gpu_dct_transform(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, uint32_t w, uint32_t h,
                            const uint8_t q_src[3], uint32_t op, const uint8_t q_dst[3], uint8_t* out, uint32_t cap,
                            uint32_t* out_size, int64_t* bad_block) {
  if (op > 7) op = 8;  // (any larger code: MYYUV_E_ARG below, whatever its low bits)
  return recode_host(c, payload, size, w, h, q_src, (int)op, q_dst, out, cap, out_size, bad_block);
}

int myyuv_gpu_dct_transform_device(myyuv_hip_handle c, const void* d_payload, const uint32_t* d_payload_sizes,
                                   uint32_t cap_in, uint32_t nframes, uint32_t w, uint32_t h,
                                   const uint8_t q_src[3], uint32_t op, const uint8_t q_dst[3], void* d_out,
                                   uint32_t cap_out, uint32_t* d_out_sizes, void* stream) {
  if (op > 7) op = 8;
  return recode_device(c, d_payload, d_payload_sizes, cap_in, nframes, w, h, q_src, (int)op, q_dst, d_out, cap_out,
                       d_out_sizes, stream);
}

// ---- export to JPEG (defined in myyuv_hip.h) --------------------------------
namespace {

// Two launches of one kernel with a scan between them ("Export
// to JPEG"): the sizing launch leaves every group's interval size, k_jpeg_place
// turns the sizes into file offsets and writes the header and the markers, the
// writing launch stores the intervals.  Workspace: the decoder's coefficient
// image and scan, and two words per 64-block group.
int reserve_jpeg(myyuv_hip_ctx* c, const FrameGeom& G, uint32_t ntg) {
  const uint32_t nwaves = ceil_div(G.cum[3] * G.nframes, kWave);
  int e = c->coef.grow((size_t)nwaves * kCoefQuadsPerWave * 16);
  e |= reserve_scan(c, G);
  e |= c->psize.grow(8);
  e |= c->jsz.grow((size_t)ntg * G.nframes * 4);
  e |= c->joff.grow((size_t)ntg * G.nframes * 4);
  return e ? MYYUV_E_HIP : 0;
}

struct JpegTiles {
  uint32_t t0, t1, t2;
  explicit JpegTiles(const FrameGeom& G)
      : t0(ceil_div(G.cum[1] - G.cum[0], kWave)),
        t1(ceil_div(G.cum[2] - G.cum[1], kWave)),
        t2(ceil_div(G.cum[3] - G.cum[2], kWave)) {}
  uint32_t n() const { return t0 + t1 + t2; }
};

int launch_jpeg_export(bool write, myyuv_hip_ctx* c, const FrameGeom& G, const uint8_t* in,
                       const uint32_t* d_size_in, uint32_t cap_in, const uint32_t* d_size_out, uint8_t* d_out,
                       uint32_t cap_out, hipStream_t s) {
  const JpegTiles T(G);
  return launch(c, MYYUV_K_JPEG, write ? k_jpeg_export<true> : k_jpeg_export<false>, dim3(T.n(), G.nframes), dim3(kWave), s, in, d_size_in,
                cap_in, (const StreamDesc*)c->desc.as<StreamDesc>(), c->loff.as<const uint32_t>(),
                c->tiles.as<const uint32_t>(), G, T.t0, T.t1, c->coef.as<uint4>(), c->jsz.as<uint32_t>(),
                c->joff.as<const uint32_t>(), d_size_out, d_out, cap_out, c->err.as<unsigned long long>());
}

// The scan and the sizing launch.
int launch_jpeg_size(myyuv_hip_ctx* c, const FrameGeom& G, const uint8_t* in, const uint32_t* d_size_in,
                     uint32_t cap_in, hipStream_t s) {
  const uint32_t ntiles = ceil_div(G.cum[3], kScanTile);
  unsigned long long* err = c->err.as<unsigned long long>();
  ScanSrc SS;
  for (int i = 0; i < 4; i++) SS.cum[i] = G.cum[i];
  for (int p = 0; p < 3; p++) SS.pos[p] = 0;
  int e = launch(c, MYYUV_K_SCAN, k_scan_chain, dim3(ntiles, G.nframes), dim3(256), s, in, cap_in, SS, d_size_in,
                 cap_in, G, c->desc.as<StreamDesc>(), c->loff.as<uint32_t>(), c->tiles.as<uint32_t>(), ntiles,
                 c->status.as<unsigned long long>(), next_epoch(c), err);
  e |= launch_jpeg_export(false, c, G, in, d_size_in, cap_in, nullptr, nullptr, 0, s);
  return e ? MYYUV_E_HIP : 0;
}

// d_out == nullptr: the files' sizes only.
int launch_jpeg_place(myyuv_hip_ctx* c, const FrameGeom& G, const myyuv_jpeg::Head& H, uint8_t* d_out,
                      uint32_t cap_out, uint32_t* d_size_out, hipStream_t s) {
  const JpegTiles T(G);
  return launch(c, MYYUV_K_JPEG_PLACE, k_jpeg_place, dim3(G.nframes), dim3(256), s, c->jsz.as<const uint32_t>(),
                c->joff.as<uint32_t>(), T.t0, T.t1, T.t2, H, d_out, cap_out, d_size_out,
                c->err.as<unsigned long long>())
             ? MYYUV_E_HIP
             : 0;
}

void jpeg_head(uint32_t w, uint32_t h, const uint8_t q[3], myyuv_jpeg::Head& H) {
  uint8_t qt[3][64];
  for (int p = 0; p < 3; p++) {
    float t[64];
    make_qtable(q[p], p != 0, t);
    for (int i = 0; i < 64; i++) qt[p][i] = (uint8_t)t[i];  // integers 1..255
  }
  (void)myyuv_jpeg::write_header(H.b, w, h, qt);
}

int jpeg_dim(uint32_t w, uint32_t h) {
  return w > myyuv_jpeg::kMaxDim || h > myyuv_jpeg::kMaxDim ? MYYUV_E_JPEG_DIM : 0;
}

// The host-buffer calls, from the stream on the device (`src`, its size at
// psize[0], queued on `s`) to the file in `out`.  The file's size comes first
// (no capacity on the device: the host compares), then a device buffer of
// that size: none is sized by the bound.
int jpeg_to_host(myyuv_hip_ctx* c, const FrameGeom& G, uint32_t w, uint32_t h, const uint8_t q[3], const uint8_t* src,
                 uint32_t cap_in, uint8_t* out, uint32_t cap, uint32_t* out_size, int64_t* bad_block,
                 hipStream_t s) {
  myyuv_jpeg::Head H;
  jpeg_head(w, h, q, H);
  uint32_t* psz = c->psize.as<uint32_t>();  // [0] the stream's size, [1] the file's
  int e;
  if ((e = launch_jpeg_size(c, G, src, psz, cap_in, s)) ||
      (e = launch_jpeg_place(c, G, H, nullptr, 0xFFFFFFFFu, psz + 1, s)))
    return e;
  uint32_t nout = 0;
  if (hipMemcpyAsync(&nout, psz + 1, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return MYYUV_E_HIP;
  if ((e = read_err(c, s, bad_block))) {  // (synchronises)
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  *out_size = nout;
  if (nout > cap) return MYYUV_E_CAPACITY;
  if (c->jout.grow(((size_t)nout + 3) & ~(size_t)3)) return MYYUV_E_HIP;
  uint8_t* dst = c->jout.as<uint8_t>();
  if ((e = launch_jpeg_place(c, G, H, dst, nout, psz + 1, s)) ||
      (e = launch_jpeg_export(true, c, G, src, psz, cap_in, psz + 1, dst, nout, s)))
    return e;
  if (d2h(out, dst, nout, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

}  // namespace

int myyuv_gpu_dct_to_jpeg(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, uint32_t w, uint32_t h,
                          const uint8_t q[3], uint8_t* out, uint32_t cap, uint32_t* out_size, int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payload || !out || !out_size || !q) return MYYUV_E_ARG;
  int e = check_q(q);
  if (e) return e;
  FrameGeom G;
  if ((e = host_parse_headers(payload, size)) || (e = make_geom(w, h, G)) || (e = jpeg_dim(w, h))) return e;
  Entry en(c);
  hipStream_t s = en.s;
  const uint32_t cap_in = (size + 3) & ~3u;
  if ((e = reserve_jpeg(c, G, JpegTiles(G).n()))) return e;
  if (c->rqsrc.grow(cap_in)) return MYYUV_E_HIP;
  uint32_t* psz = c->psize.as<uint32_t>();  // [0] the stream's size, [1] the file's
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (hipMemsetAsync(static_cast<uint8_t*>(c->rqsrc.p) + (cap_in - 4), 0, 4, s) != hipSuccess ||
      h2d(c->rqsrc.p, payload, size, s) || hipMemcpyAsync(psz, &size, 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  return jpeg_to_host(c, G, w, h, q, c->rqsrc.as<const uint8_t>(), cap_in, out, cap, out_size, bad_block, s);
}

int myyuv_gpu_iyuv_to_jpeg(myyuv_hip_handle c, const uint8_t* iyuv, uint32_t w, uint32_t h, const uint8_t q[3],
                           uint8_t* out, uint32_t cap, uint32_t* out_size) {
  if (!c || !iyuv || !out || !out_size || !q) return MYYUV_E_ARG;
  FrameGeom G;
  int e = check_q(q);
  if (e || (e = make_geom(w, h, G)) || (e = jpeg_dim(w, h))) return e;
  Entry en(c);
  hipStream_t s = en.s;
  const size_t fbytes = (size_t)w * h * 3 / 2;
  const uint32_t bound = myyuv_dct_payload_bound(w, h);
  if ((e = reserve(c, G)) || (e = reserve_jpeg(c, G, JpegTiles(G).n())) || (e = set_qtables(c, q, s))) return e;
  if (c->frame.grow(fbytes) || c->payload.grow(bound)) return MYYUV_E_HIP;
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (h2d(c->frame.p, iyuv, fbytes, s)) return MYYUV_E_HIP;
  // the stream stays on the device: the encoder's payload buffer is the exporter's source
  if ((e = launch_compress(c, G, c->frame.p, c->payload.p, bound, c->psize.as<uint32_t>(), s))) return e;
  return jpeg_to_host(c, G, w, h, q, c->payload.as<const uint8_t>(), bound, out, cap, out_size, nullptr, s);
}

int myyuv_gpu_dct_to_jpeg_device(myyuv_hip_handle c, const void* d_payload, const uint32_t* d_payload_sizes,
                                 uint32_t cap_in, uint32_t nframes, uint32_t w, uint32_t h, const uint8_t q[3],
                                 void* d_out, uint32_t cap_out, uint32_t* d_out_sizes, void* stream) {
  if (!c || !d_payload || !d_payload_sizes || !d_out || !d_out_sizes || !q) return MYYUV_E_ARG;
  FrameGeom G;
  int e = check_q(q);
  if (e || (e = make_geom(w, h, G)) || (e = set_batch(G, nframes)) || (e = jpeg_dim(w, h))) return e;
  if (((uintptr_t)d_payload & 3) || (nframes > 1 && (cap_in & 3))) return MYYUV_E_ARG;
  {  // the two arrays must not overlap: a file is written while later streams are still being read
    const uintptr_t a = (uintptr_t)d_payload, b = (uintptr_t)d_out;
    const uint64_t na = (uint64_t)cap_in * nframes, nb = (uint64_t)cap_out * nframes;
    if (a < b + nb && b < a + na) return MYYUV_E_ARG;
  }
  myyuv_jpeg::Head H;
  jpeg_head(w, h, q, H);
  Entry en(c, stream);
  // (as several launches past the kernels' 32-bit block numbers or the grid's 65,535 frames)
  const uint32_t per = std::min(launch_frames(G, c->launch_blocks), 65535u);
  FrameGeom GL = G;
  if ((e = set_batch(GL, std::min(nframes, per))) || (e = reserve_jpeg(c, GL, JpegTiles(G).n()))) return e;
  for (uint32_t f0 = 0; f0 < nframes; f0 += per) {
    GL = G;
    GL.fbase = f0;
    if ((e = set_batch(GL, std::min(per, nframes - f0)))) return e;
    const uint8_t* src = static_cast<const uint8_t*>(d_payload) + (size_t)f0 * cap_in;
    uint8_t* dst = static_cast<uint8_t*>(d_out) + (size_t)f0 * cap_out;
    if ((e = launch_jpeg_size(c, GL, src, d_payload_sizes + f0, cap_in, en.s)) ||
        (e = launch_jpeg_place(c, GL, H, dst, cap_out, d_out_sizes + f0, en.s)) ||
        (e = launch_jpeg_export(true, c, GL, src, d_payload_sizes + f0, cap_in, d_out_sizes + f0, dst, cap_out,
                                      en.s)))
      return e;
  }
  return 0;
}

// ---- import from JPEG (defined in myyuv_hip.h) ------------------------------
static_assert(MYYUV_E_JPEG_UNSUPPORTED == myyuv_jpegin::kUnsupported && MYYUV_E_JPEG_SYNTAX == myyuv_jpegin::kSyntax &&
                  MYYUV_E_JPEG_DATA == myyuv_jpegin::kData && MYYUV_E_JPEG_TABLES == myyuv_jpegin::kTables &&
                  MYYUV_JPEG_SEGMENTS_MIN == myyuv_jpegin::kSegThreshold,
              "jpeg_import.h's codes are the header's");
namespace {

// The smallest q in 1..100 whose make_qtable is `t` (natural order), or 0.
uint8_t keep_quality(const uint8_t t[64], bool chroma) {
  for (int q = 1; q <= 100; q++) {
    float f[64];
    make_qtable(q, chroma, f);
    int i = 0;
    while (i < 64 && f[i] == (float)t[i]) i++;
    if (i == 64) return (uint8_t)q;
  }
  return 0;
}

// A parsed file: inspect's findings, the segment table, the qualities the
// stream is decoded with and the call's rescale tables (file -> destination).
struct JpegIn {
  myyuv_jpegin::Info I;
  std::vector<myyuv_jpegin::Seg> segs;
  uint8_t q[3];
  RequantTables rq;
  uint32_t rescale = 0;  // bit p: plane p's table is not the destination's
  bool on_gpu = false;
  FrameGeom G;
};

bool jpeg_on_gpu(const myyuv_jpegin::Info& I) {
  bool ri = true;
  for (uint32_t s = 0; s < I.plan.nscan; s++) ri = ri && I.plan.ri[s] != 0;
  return ri && I.nseg >= myyuv_jpegin::kSegThreshold;
}

// The checks that need no device, in the header's order.
int jpeg_parse(const uint8_t* file, uint32_t size, const uint8_t* quality, JpegIn& J) {
  // one walk over the file for all but the longest tables: room for 64 Ki intervals first
  J.segs.resize(1u << 16);
  int e = myyuv_jpegin::inspect(file, size, J.I, J.segs.data(), (uint32_t)J.segs.size());
  if (e) return e;
  const bool again = J.I.nseg > J.segs.size();
  J.segs.resize(J.I.nseg);
  if (again && (e = myyuv_jpegin::inspect(file, size, J.I, J.segs.data(), J.I.nseg))) return e;
  if (quality) {
    if ((e = check_q(quality))) return e;
    std::memcpy(J.q, quality, 3);
  } else {
    for (int p = 0; p < 3; p++)
      if (!(J.q[p] = keep_quality(J.I.qt[p], p != 0))) return MYYUV_E_JPEG_TABLES;
  }
  for (int p = 0; p < 3; p++) {
    for (int i = 0; i < 64; i++) J.rq.qs[p][i] = (float)J.I.qt[p][i];
    make_qtable(J.q[p], p != 0, J.rq.qd[p]);
    if (std::memcmp(J.rq.qs[p], J.rq.qd[p], sizeof(J.rq.qs[p])) != 0) J.rescale |= 1u << p;
  }
  J.on_gpu = jpeg_on_gpu(J.I);
  return make_geom(J.I.Wp, J.I.Hp, J.G);
}

// The rescale tables of this call, on the device in stream order (a buffer of
// their own: the requantiser's cache is keyed by qualities and stays valid).
int jpeg_tables(myyuv_hip_ctx* c, const JpegIn& J, hipStream_t s) {
  if (c->jrq.grow(sizeof(RequantTables))) return MYYUV_E_HIP;
  return h2d(c->jrq.p, &J.rq, sizeof(RequantTables), s);
}

// The restart-interval path: the file at d_file -> the stream at d_out.
int launch_jpeg_import(myyuv_hip_ctx* c, const JpegIn& J, const void* d_file, void* d_out, uint32_t cap_out,
                       uint32_t* d_size_out, hipStream_t s) {
  using namespace myyuv_jpegin;
  const Plan& P = J.I.plan;
  const uint32_t nseg = J.I.nseg, nblk = J.G.cum[3];
  if (c->jseg.grow((size_t)nseg * sizeof(Seg)) || c->jtab.grow(6 * sizeof(DecTab))) return MYYUV_E_HIP;
  DecTab tabs[6];
  for (int p = 0; p < 3; p++) {
    tabs[p] = J.I.dc[p];
    tabs[3 + p] = J.I.ac[p];
  }
  int e = h2d(c->jseg.p, J.segs.data(), (size_t)nseg * sizeof(Seg), s);
  e |= h2d(c->jtab.p, tabs, sizeof(tabs), s);
  e |= hipMemsetAsync(c->work.p, 0, 4, s) != hipSuccess;
  // blocks of the padded grid that no scan holds are all-zero blocks
  if (P.ns[0] == 1 && (P.cw[0] != P.bw[0] || P.ch[0] * 8 != J.I.Hp)) {
    e |= hipMemsetAsync(c->rmask.p, 0, nblk, s) != hipSuccess;
    e |= hipMemsetAsync(c->binfo.p, 0, (size_t)nblk * 4, s) != hipSuccess;
  }
  e |= launch(c, MYYUV_K_JPEG_IMPORT, k_jpeg_import, dim3(ceil_div(nseg, kWave)), dim3(kWave), s,
              static_cast<const uint32_t*>(d_file), c->jseg.as<const Seg>(), nseg, P, c->jtab.as<const DecTab>(),
              c->jrq.as<const RequantTables>(), J.rescale, c->coef.as<uint4>(), c->rmask.as<uint8_t>(),
              c->binfo.as<uint32_t>(), c->err.as<unsigned long long>());
  e |= launch_encode_tail(c, J.G, d_out, cap_out, d_size_out, s);
  return e ? MYYUV_E_HIP : 0;
}

// The coefficient-image path: img (int16 [blocks][64]) on the device -> the stream.
int launch_jpeg_import_coef(myyuv_hip_ctx* c, const JpegIn& J, const void* d_img, void* d_out, uint32_t cap_out,
                            uint32_t* d_size_out, hipStream_t s) {
  const FrameGeom& G = J.G;
  int e = hipMemsetAsync(c->work.p, 0, 4, s) != hipSuccess;
  e |= launch(c, MYYUV_K_JPEG_IMPORT_COEF, k_jpeg_import_coef, dim3(ceil_div(G.cum[3], kWave)), dim3(kWave), s,
              static_cast<const uint4*>(d_img), G.cum[3], G.cum[1], G.cum[2], c->jrq.as<const RequantTables>(),
              J.rescale, c->coef.as<uint4>(), c->rmask.as<uint8_t>(), c->binfo.as<uint32_t>());
  e |= launch_encode_tail(c, G, d_out, cap_out, d_size_out, s);
  return e ? MYYUV_E_HIP : 0;
}

}  // namespace

int myyuv_jpeg_inspect(const uint8_t* file, uint32_t size, myyuv_jpeg_info* info) {
  if (!file || !info) return MYYUV_E_ARG;
  std::memset(info, 0, sizeof(*info));
  auto I = std::make_unique<myyuv_jpegin::Info>();
  if (int e = myyuv_jpegin::inspect(file, size, *I, nullptr, 0)) return e;
  info->width = I->W;
  info->height = I->H;
  info->padded_width = I->Wp;
  info->padded_height = I->Hp;
  info->scans = I->plan.nscan;
  for (uint32_t s = 0; s < I->plan.nscan; s++) info->restart_interval[s] = I->plan.ri[s];
  info->segments = I->nseg;
  info->on_gpu = jpeg_on_gpu(*I) ? 1u : 0u;
  FrameGeom G;
  info->payload_bound = make_geom(I->Wp, I->Hp, G) ? 0u : myyuv_dct_payload_bound(I->Wp, I->Hp);
  for (int p = 0; p < 3; p++) info->keep_quality[p] = keep_quality(I->qt[p], p != 0);
  return 0;
}

int myyuv_gpu_jpeg_to_dct(myyuv_hip_handle c, const uint8_t* file, uint32_t size, const uint8_t* quality,
                          uint8_t* out, uint32_t cap, uint32_t* out_size, uint32_t* width, uint32_t* height,
                          uint8_t q_out[3], int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !file || !out || !out_size || !width || !height || !q_out) return MYYUV_E_ARG;
  auto J = std::make_unique<JpegIn>();
  int e = jpeg_parse(file, size, quality, *J);
  if (e) return e;
  const FrameGeom& G = J->G;
  *width = J->I.Wp;
  *height = J->I.Hp;
  std::memcpy(q_out, J->q, 3);
  std::vector<int16_t> img;
  if (!J->on_gpu) {  // the host decode, by the kernel's own block decoder
    img.assign((size_t)G.cum[3] * 64, 0);
    int64_t bad = -1;
    if ((e = myyuv_jpegin::decode_scans(file, size, J->I, J->segs.data(), J->I.nseg, img.data(), &bad))) {
      if (bad_block) *bad_block = bad;
      return e;
    }
  }
  Entry en(c);
  hipStream_t s = en.s;
  // the device writes into a buffer of the bound's size, so a result larger
  // than the caller's `cap` is known by its size alone (as compress)
  const uint32_t bound = myyuv_dct_payload_bound(J->I.Wp, J->I.Hp);
  const size_t nin = J->on_gpu ? ((size_t)size + 3) & ~(size_t)3 : img.size() * 2;
  if ((e = reserve(c, G))) return e;
  if (c->jin.grow(nin) || c->payload.grow(bound) || c->psize.grow(8)) return MYYUV_E_HIP;
  uint32_t* psz = c->psize.as<uint32_t>();
  if (reset_err(c, s) || (e = jpeg_tables(c, *J, s))) return MYYUV_E_HIP;
  if (J->on_gpu) {
    if (hipMemsetAsync(static_cast<uint8_t*>(c->jin.p) + (nin - 4), 0, 4, s) != hipSuccess ||
        h2d(c->jin.p, file, size, s))
      return MYYUV_E_HIP;
    e = launch_jpeg_import(c, *J, c->jin.p, c->payload.p, bound, psz + 1, s);
  } else {
    if (h2d(c->jin.p, img.data(), nin, s)) return MYYUV_E_HIP;
    e = launch_jpeg_import_coef(c, *J, c->jin.p, c->payload.p, bound, psz + 1, s);
  }
  if (e) return e;
  uint32_t nout = 0;
  if (hipMemcpyAsync(&nout, psz + 1, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return MYYUV_E_HIP;
  if ((e = read_err(c, s, bad_block))) {  // (synchronises)
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  *out_size = nout;
  if (nout > cap) return MYYUV_E_CAPACITY;
  if (d2h(out, c->payload.p, nout, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

int myyuv_gpu_jpeg_to_dct_device(myyuv_hip_handle c, const void* d_file, const uint8_t* file, uint32_t size,
                                 const uint8_t* quality, void* d_out, uint32_t cap, uint32_t* d_out_size,
                                 uint32_t* width, uint32_t* height, uint8_t q_out[3], void* stream) {
  if (!c || !d_file || !file || !d_out || !d_out_size || !width || !height || !q_out) return MYYUV_E_ARG;
  if (((uintptr_t)d_file & 3) || ((uintptr_t)d_out & 3)) return MYYUV_E_ARG;
  auto J = std::make_unique<JpegIn>();
  int e = jpeg_parse(file, size, quality, *J);
  if (e) return e;
  if (!J->on_gpu) return MYYUV_E_JPEG_UNSUPPORTED;
  *width = J->I.Wp;
  *height = J->I.Hp;
  std::memcpy(q_out, J->q, 3);
  Entry en(c, stream);
  if ((e = reserve(c, J->G)) || (e = jpeg_tables(c, *J, en.s))) return e;
  return launch_jpeg_import(c, *J, d_file, d_out, cap, d_out_size, en.s);
}

// ---- downscale (defined in myyuv_hip.h) -------------------------------------
int myyuv_gpu_dct_downscale(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, uint32_t w, uint32_t h,
                            const uint8_t q_src[3], uint32_t denom, const uint8_t q_dst[3], uint8_t* out,
                            uint32_t cap, uint32_t* out_size, int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payload || !out || !out_size || !q_src || !q_dst) return MYYUV_E_ARG;
  int e = check_q(q_src);
  if (e) return e;
  FrameGeom G, Gd;
  if ((e = host_parse_headers(payload, size)) || (e = make_geom(w, h, G)) || (e = check_q(q_dst))) return e;
  if (!denom_ok(denom)) return MYYUV_E_ARG;
  if ((e = make_geom(w / denom, h / denom, Gd))) return e;
  Entry en(c);
  hipStream_t s = en.s;
  const uint32_t cap_in = (size + 3) & ~3u;
  // the device writes into a buffer of the bound's size, so a result larger
  // than the caller's `cap` is known by its size alone (as compress)
  const uint32_t bound = myyuv_dct_payload_bound(w / denom, h / denom);
  if ((e = reserve_downscale(c, G, Gd)) || (e = set_downscale_tables(c, q_src, q_dst, s))) return e;
  if (c->rqsrc.grow(cap_in) || c->payload.grow(bound) || c->psize.grow(8)) return MYYUV_E_HIP;
  uint32_t* psz = c->psize.as<uint32_t>();  // [0] the source's size, [1] the result's
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (hipMemsetAsync(static_cast<uint8_t*>(c->rqsrc.p) + (cap_in - 4), 0, 4, s) != hipSuccess ||
      h2d(c->rqsrc.p, payload, size, s) || hipMemcpyAsync(psz, &size, 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  if ((e = launch_downscale(c, G, Gd, denom, c->rqsrc.p, psz, cap_in, c->payload.p, bound, psz + 1, s))) return e;
  uint32_t nout = 0;
  if (hipMemcpyAsync(&nout, psz + 1, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return MYYUV_E_HIP;
  if ((e = read_err(c, s, bad_block))) {  // (synchronises)
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  *out_size = nout;
  if (nout > cap) return MYYUV_E_CAPACITY;
  if (d2h(out, c->payload.p, nout, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

int myyuv_gpu_dct_downscale_device(myyuv_hip_handle c, const void* d_payload, const uint32_t* d_payload_sizes,
                                   uint32_t cap_in, uint32_t nframes, uint32_t w, uint32_t h,
                                   const uint8_t q_src[3], uint32_t denom, const uint8_t q_dst[3], void* d_out,
                                   uint32_t cap_out, uint32_t* d_out_sizes, void* stream) {
  if (!c || !d_payload || !d_payload_sizes || !d_out || !d_out_sizes || !q_src || !q_dst) return MYYUV_E_ARG;
  FrameGeom G, Gd;
  int e = check_q(q_src);
  if (e || (e = make_geom(w, h, G)) || (e = set_batch(G, nframes)) || (e = check_q(q_dst))) return e;
  if (!denom_ok(denom)) return MYYUV_E_ARG;
  if ((e = make_geom(w / denom, h / denom, Gd))) return e;
  if (((uintptr_t)d_payload & 3) || ((uintptr_t)d_out & 3) || (nframes > 1 && ((cap_in | cap_out) & 3)))
    return MYYUV_E_ARG;
  {  // the two stream arrays must not overlap: K4 writes frame f while later frames are still being read
    const uintptr_t a = (uintptr_t)d_payload, b = (uintptr_t)d_out;
    const uint64_t na = (uint64_t)cap_in * nframes, nb = (uint64_t)cap_out * nframes;
    if (a < b + nb && b < a + na) return MYYUV_E_ARG;
  }
  Entry en(c, stream);
  // (as several launches past the kernels' 32-bit block numbers or the grid's 65,535 frames)
  const uint32_t per = std::min(launch_frames(G, c->launch_blocks), 65535u);
  FrameGeom GL = G, GD = Gd;
  if ((e = set_batch(GL, std::min(nframes, per))) || (e = set_batch(GD, std::min(nframes, per))) ||
      (e = reserve_downscale(c, GL, GD)) || (e = set_downscale_tables(c, q_src, q_dst, en.s)))
    return e;
  for (uint32_t f0 = 0; f0 < nframes; f0 += per) {
    GL = G;
    GD = Gd;
    GL.fbase = GD.fbase = f0;
    if ((e = set_batch(GL, std::min(per, nframes - f0))) || (e = set_batch(GD, std::min(per, nframes - f0))))
      return e;
    const uint8_t* src = static_cast<const uint8_t*>(d_payload) + (size_t)f0 * cap_in;
    uint8_t* dst = static_cast<uint8_t*>(d_out) + (size_t)f0 * cap_out;
    if ((e = launch_downscale(c, GL, GD, denom, src, d_payload_sizes + f0, cap_in, dst, cap_out, d_out_sizes + f0,
                              en.s)))
      return e;
  }
  return 0;
}

// ---- crop and join (defined in myyuv_hip.h) ---------------------------------
namespace {

using myyuv_gather::GatherMap;

// Workspace of a gather launch: the scan of the source streams (Gs: the source
// geometry, its batch the launch's source streams) and, for `nout` output
// frames of dblk blocks, the size-byte table (1 B per block) and the
// destination scan (4 B per block plus tile words).  Nothing of the 471 B per
// block the codec calls reserve.
int reserve_gather(myyuv_hip_ctx* c, const FrameGeom& Gs, uint32_t dblk, uint32_t nout) {
  if (int e = reserve_scan(c, Gs)) return e;
  const uint32_t dnt = ceil_div(dblk, kScanTile);
  int e = 0;
  e |= c->gsz.grow((size_t)nout * dblk);
  e |= c->gloff.grow((size_t)nout * dblk * 4);
  e |= c->gtiles.grow((size_t)nout * (dnt + 1) * 4);
  const size_t st_bytes = (size_t)nout * (dnt + 1) * 8;
  if (c->status.n < st_bytes) {  // (as reserve_scan: zeroed before any kernel reads it)
    e |= c->status.grow(st_bytes);
    if (!e && (hipMemset(c->status.p, 0, st_bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
      e |= MYYUV_E_HIP;
  }
  return e ? MYYUV_E_HIP : 0;
}

// One launch: output frame f (Gd.nframes of them, at d_out + f * cap_out, its
// size at d_size_out[f]) from the source streams f * nsub .. f * nsub + nsub - 1
// (nsub = M.cols * M.rows; stream k at d_in + k * cap_in, its size at
// d_size_in[k]).  Gs: the source geometry with the launch's nsub * nframes
// streams as its batch and fbase the first one's index in the caller's batch
// (of source streams: the error keys count in them).  report_cap: a frame
// larger than cap_out is MYYUV_E_CAPACITY in the error word (the device
// forms); the host-buffer forms pass their own bound and judge the size read
// back themselves (gather_host_finish).
int launch_gather(myyuv_hip_ctx* c, const FrameGeom& Gs, const FrameGeom& Gd, const GatherMap& M, const void* d_in,
                  const uint32_t* d_size_in, uint32_t cap_in, void* d_out, uint32_t cap_out, uint32_t* d_size_out,
                  bool report_cap, hipStream_t s) {
  const uint32_t nsrc = Gs.nframes, nout = Gd.nframes;
  const uint32_t snt = ceil_div(Gs.cum[3], kScanTile), dnt = ceil_div(Gd.cum[3], kScanTile);
  unsigned long long* err = c->err.as<unsigned long long>();
  StreamDesc* desc = c->desc.as<StreamDesc>();
  const uint8_t* in = static_cast<const uint8_t*>(d_in);
  uint8_t* out = static_cast<uint8_t*>(d_out);
  int e = 0;
  ScanSrc SS, SD;
  for (int i = 0; i < 4; i++) SS.cum[i] = Gs.cum[i], SD.cum[i] = Gd.cum[i];
  for (int p = 0; p < 3; p++) SS.pos[p] = 0, SD.pos[p] = Gd.cum[p];  // (the table holds the planes back to back)
  e |= launch(c, MYYUV_K_SCAN, k_scan_chain, dim3(snt, nsrc), dim3(256), s, in, cap_in, SS, d_size_in, cap_in, Gs, desc,
              c->loff.as<uint32_t>(), c->tiles.as<uint32_t>(), snt, c->status.as<unsigned long long>(), next_epoch(c),
              err);
  e |= launch(c, MYYUV_K_SCAN, k_gather_sizes, dim3(ceil_div(Gd.cum[3], 256), nout), dim3(256), s, in, cap_in,
              (const StreamDesc*)desc, M, c->gsz.as<uint8_t>());
  e |= launch(c, MYYUV_K_SCAN, k_scan_chain, dim3(dnt, nout), dim3(256), s, c->gsz.as<const uint8_t>(), Gd.cum[3], SD,
              (const uint32_t*)nullptr, 0u, Gd, (StreamDesc*)nullptr, c->gloff.as<uint32_t>(),
              c->gtiles.as<uint32_t>(), dnt, c->status.as<unsigned long long>(), next_epoch(c), err);
  e |= launch(c, MYYUV_K_SCAN, k_gather_heads, dim3(nout), dim3(kWave), s, c->gloff.as<const uint32_t>(),
              c->gtiles.as<const uint32_t>(), M, out, cap_out, report_cap ? 1u : 0u, d_size_out, err);
  e |= launch(c, MYYUV_K_GATHER, k_stream_gather, dim3(M.rcum[3], nout), dim3(kWave), s, in, cap_in,
              (const StreamDesc*)desc, c->loff.as<const uint32_t>(), c->tiles.as<const uint32_t>(),
              c->gsz.as<const uint8_t>(), c->gloff.as<const uint32_t>(), c->gtiles.as<const uint32_t>(), M,
              Gs.fbase, out, cap_out, err);
  return e ? MYYUV_E_HIP : 0;
}

// The join's grid: tiles of whole 16 x 16 units, at least one each way, no
// 32-bit wrap, an output frame the compressor accepts (Gd: its geometry) and
// at most 65,535 tiles (the scan's grid takes one row per tile).
int make_join(uint32_t cols, uint32_t rows, uint32_t tw, uint32_t th, FrameGeom& Gd) {
  if (cols == 0 || rows == 0 || tw == 0 || th == 0 || ((tw | th) & 15u)) return MYYUV_E_ARG;
  if ((uint64_t)cols * tw > 0xFFFFFFFFull || (uint64_t)rows * th > 0xFFFFFFFFull) return MYYUV_E_ARG;
  if ((uint64_t)cols * rows > 65535ull) return MYYUV_E_ARG;
  if (make_geom(cols * tw, rows * th, Gd)) return MYYUV_E_ARG;
  return 0;
}

// Upper bound of a gather's result: its headers and size bytes, and no more
// content than the sources hold.
uint32_t gather_bound(uint32_t dblk, uint64_t src_bytes) {
  const uint64_t b = 36ull + dblk + src_bytes;
  return b > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)((b + 3) & ~3ull);
}

// The host-buffer calls' device part and their epilogue: the streams are in
// c->rqsrc (stream k at k * cap_in), their sizes at psz[0 .. nsub), the
// result goes to c->payload and its size to psz[nsub].
int gather_host_finish(myyuv_hip_ctx* c, const FrameGeom& Gs, const FrameGeom& Gd, const GatherMap& M,
                       uint32_t cap_in, uint32_t bound, uint8_t* out, uint32_t cap, uint32_t* out_size,
                       int64_t* bad_block, hipStream_t s) {
  const uint32_t nsub = M.cols * M.rows;
  uint32_t* psz = c->psize.as<uint32_t>();
  int e = launch_gather(c, Gs, Gd, M, c->rqsrc.p, psz, cap_in, c->payload.p, bound, psz + nsub, false, s);
  if (e) return e;
  uint32_t nout = 0;
  if (hipMemcpyAsync(&nout, psz + nsub, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return MYYUV_E_HIP;
  e = read_err(c, s, bad_block);  // (synchronises)
  if (!e && nout > bound) {
    // `bound` holds every byte of the sources, so only a size table that
    // overruns its plane's declared content selects more: k_stream_gather
    // wrote and checked nothing, and the check runs on its own
    // (MYYUV_E_PLANE_CONTENT comes before the caller's capacity)
    if (launch(c, MYYUV_K_SCAN, k_gather_check, dim3(M.rcum[3], Gd.nframes), dim3(kWave), s,
               static_cast<const uint8_t*>(c->rqsrc.p), cap_in, c->desc.as<const StreamDesc>(),
               c->loff.as<const uint32_t>(), c->tiles.as<const uint32_t>(), M, Gs.fbase,
               c->err.as<unsigned long long>()))
      return MYYUV_E_HIP;
    if (!(e = read_err(c, s, bad_block))) e = MYYUV_E_HIP;  // (cannot be: see above)
  }
  if (e) {
    (void)reset_err(c, s);
    (void)hipStreamSynchronize(s);
    return e;
  }
  *out_size = nout;
  if (nout > cap) return MYYUV_E_CAPACITY;
  if (d2h(out, c->payload.p, nout, s)) return MYYUV_E_HIP;
  if (c->prof) drain_profile(c);
  return 0;
}

bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

}  // namespace

int myyuv_gpu_dct_crop(myyuv_hip_handle c, const uint8_t* payload, uint32_t size, uint32_t w, uint32_t h, uint32_t rx,
                       uint32_t ry, uint32_t rw, uint32_t rh, uint8_t* out, uint32_t cap, uint32_t* out_size,
                       int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payload || !out || !out_size) return MYYUV_E_ARG;
  FrameGeom G, R;
  RegionSegs S;
  int e;
  if ((e = host_parse_headers(payload, size)) || (e = make_geom(w, h, G)) ||
      (e = make_region(w, h, rx, ry, rw, rh, R, S)))
    return e;
  if (ranges_overlap(payload, size, out, cap)) return MYYUV_E_ARG;
  const GatherMap M = myyuv_gather::crop_map(w, h, rx, ry, rw, rh);
  Entry en(c);
  hipStream_t s = en.s;
  const uint32_t cap_in = (size + 3) & ~3u;
  const uint32_t bound = gather_bound(R.cum[3], size);
  if ((e = reserve_gather(c, G, R.cum[3], 1))) return e;
  if (c->rqsrc.grow(cap_in) || c->payload.grow(bound) || c->psize.grow(8)) return MYYUV_E_HIP;
  if (reset_err(c, s)) return MYYUV_E_HIP;
  if (hipMemsetAsync(static_cast<uint8_t*>(c->rqsrc.p) + (cap_in - 4), 0, 4, s) != hipSuccess ||
      h2d(c->rqsrc.p, payload, size, s) ||
      hipMemcpyAsync(c->psize.p, &size, 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return MYYUV_E_HIP;
  return gather_host_finish(c, G, R, M, cap_in, bound, out, cap, out_size, bad_block, s);
}

int myyuv_gpu_dct_crop_device(myyuv_hip_handle c, const void* d_payload, const uint32_t* d_payload_sizes,
                              uint32_t cap_in, uint32_t nframes, uint32_t w, uint32_t h, uint32_t rx, uint32_t ry,
                              uint32_t rw, uint32_t rh, void* d_out, uint32_t cap_out, uint32_t* d_out_sizes,
                              void* stream) {
  if (!c || !d_payload || !d_payload_sizes || !d_out || !d_out_sizes) return MYYUV_E_ARG;
  FrameGeom G, R;
  RegionSegs S;
  int e;
  if ((e = make_geom(w, h, G)) || (e = set_batch(G, nframes)) || (e = make_region(w, h, rx, ry, rw, rh, R, S)))
    return e;
  if (((uintptr_t)d_payload & 3) || ((uintptr_t)d_out & 3) || (nframes > 1 && ((cap_in | cap_out) & 3)))
    return MYYUV_E_ARG;
  if (ranges_overlap(d_payload, (uint64_t)cap_in * nframes, d_out, (uint64_t)cap_out * nframes)) return MYYUV_E_ARG;
  const GatherMap M = myyuv_gather::crop_map(w, h, rx, ry, rw, rh);
  Entry en(c, stream);
  // (as several launches past the kernels' 32-bit block numbers or the grid's 65,535 frames)
  const uint32_t per = std::min(launch_frames(G, c->launch_blocks), 65535u);
  FrameGeom GL = G, RL = R;
  if ((e = set_batch(GL, std::min(nframes, per))) || (e = reserve_gather(c, GL, R.cum[3], GL.nframes))) return e;
  for (uint32_t f0 = 0; f0 < nframes; f0 += per) {
    GL = G;
    GL.fbase = f0;
    if ((e = set_batch(GL, std::min(per, nframes - f0))) || (e = set_batch(RL, GL.nframes))) return e;
    const uint8_t* src = static_cast<const uint8_t*>(d_payload) + (size_t)f0 * cap_in;
    uint8_t* dst = static_cast<uint8_t*>(d_out) + (size_t)f0 * cap_out;
    if ((e = launch_gather(c, GL, RL, M, src, d_payload_sizes + f0, cap_in, dst, cap_out, d_out_sizes + f0, true,
                           en.s)))
      return e;
  }
  return 0;
}

int myyuv_gpu_dct_join(myyuv_hip_handle c, const uint8_t* const* payloads, const uint32_t* sizes, uint32_t cols,
                       uint32_t rows, uint32_t tw, uint32_t th, uint8_t* out, uint32_t cap, uint32_t* out_size,
                       int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payloads || !sizes || !out || !out_size) return MYYUV_E_ARG;
  // (the grid's counts first: they say how many streams there are to look at)
  if (cols == 0 || rows == 0 || (uint64_t)cols * rows > 65535ull) return MYYUV_E_ARG;
  const uint32_t nsub = cols * rows;
  FrameGeom G, Gd;
  int e = 0;
  uint64_t src_bytes = 0;
  uint32_t cap_in = 4;
  for (uint32_t t = 0; t < nsub; t++)
    if (!payloads[t]) return MYYUV_E_ARG;
  for (uint32_t t = 0; t < nsub; t++) {
    if ((e = host_parse_headers(payloads[t], sizes[t]))) {
      // tile t's first block, as the device batches report it (-1 for tile 0)
      const uint64_t tblk = (uint64_t)(tw / 8) * (th / 8) + 2ull * (tw / 16) * (th / 16);
      if (bad_block && t) *bad_block = (int64_t)(t * tblk);
      return e;
    }
    src_bytes += sizes[t];
    cap_in = std::max(cap_in, (sizes[t] + 3) & ~3u);
  }
  if ((e = make_geom(tw, th, G)) || (e = make_join(cols, rows, tw, th, Gd)) || (e = set_batch(G, nsub))) return e;
  for (uint32_t t = 0; t < nsub; t++)
    if (ranges_overlap(payloads[t], sizes[t], out, cap)) return MYYUV_E_ARG;
  const GatherMap M = myyuv_gather::join_map(cols, rows, tw, th);
  Entry en(c);
  hipStream_t s = en.s;
  const uint32_t bound = gather_bound(Gd.cum[3], src_bytes);
  if ((e = reserve_gather(c, G, Gd.cum[3], 1))) return e;
  if (c->rqsrc.grow((size_t)cap_in * nsub) || c->payload.grow(bound) || c->psize.grow((size_t)(nsub + 1) * 4))
    return MYYUV_E_HIP;
  if (reset_err(c, s)) return MYYUV_E_HIP;
  // (every slot's bytes past its stream are defined: the copy's loads are whole dwords)
  if (hipMemsetAsync(c->rqsrc.p, 0, (size_t)cap_in * nsub, s) != hipSuccess) return MYYUV_E_HIP;
  for (uint32_t t = 0; t < nsub; t++)
    if (h2d(static_cast<uint8_t*>(c->rqsrc.p) + (size_t)t * cap_in, payloads[t], sizes[t], s)) return MYYUV_E_HIP;
  if (hipMemcpyAsync(c->psize.p, sizes, (size_t)nsub * 4, hipMemcpyHostToDevice, s) != hipSuccess) return MYYUV_E_HIP;
  return gather_host_finish(c, G, Gd, M, cap_in, bound, out, cap, out_size, bad_block, s);
}

int myyuv_gpu_dct_join_device(myyuv_hip_handle c, const void* d_payload, const uint32_t* d_payload_sizes,
                              uint32_t cap_in, uint32_t cols, uint32_t rows, uint32_t tw, uint32_t th, void* d_out,
                              uint32_t cap_out, uint32_t* d_out_size, void* stream) {
  if (!c || !d_payload || !d_payload_sizes || !d_out || !d_out_size) return MYYUV_E_ARG;
  FrameGeom G, Gd;
  int e;
  if ((e = make_geom(tw, th, G)) || (e = make_join(cols, rows, tw, th, Gd))) return e;
  const uint32_t nsub = cols * rows;
  if ((e = set_batch(G, nsub))) return e;
  if (((uintptr_t)d_payload & 3) || ((uintptr_t)d_out & 3) || (nsub > 1 && (cap_in & 3))) return MYYUV_E_ARG;
  if (ranges_overlap(d_payload, (uint64_t)cap_in * nsub, d_out, cap_out)) return MYYUV_E_ARG;
  const GatherMap M = myyuv_gather::join_map(cols, rows, tw, th);
  Entry en(c, stream);
  if ((e = reserve_gather(c, G, Gd.cum[3], 1))) return e;
  return launch_gather(c, G, Gd, M, d_payload, d_payload_sizes, cap_in, d_out, cap_out, d_out_size, true, en.s);
}

// ---- host-buffer batches, pipelined ------------------
//
// The batch is cut into chunks of B frames, alternating between two device
// slots.  Chunk k's host -> device copies run on cin while chunk k-1's kernels
// run on the context's stream and chunk k-2's results go back on cout, so the
// PCIe transfers of both directions and the kernels overlap; the host waits
// only for a chunk's sizes and error word (pinned, copied behind its
// kernels) before it queues that chunk's device -> host copies.  Each copy
// goes straight between the caller's (pageable) buffers and the slot.
namespace {

// MYYUV_PIPE_TRACE=1: one stderr line per pipeline step (diagnostic)
bool pipe_trace() {
  static int t = -1;
  if (t < 0) t = std::getenv("MYYUV_PIPE_TRACE") ? 1 : 0;
  return t == 1;
}
#define PIPE_TRACE(...) (pipe_trace() ? (void)(std::fprintf(stderr, __VA_ARGS__), std::fflush(stderr)) : (void)0)
constexpr size_t kPipeSlotBytes = (size_t)2 << 30;  // per slot: chunk frames x (input + output) bytes

// frames per chunk: about 8 chunks per batch (the first chunk's upload and
// the last one's download are not overlapped), at most kPipeMaxChunk and
// within the slot budget
uint32_t pipe_chunk(uint32_t nf, size_t per_frame) {
  uint32_t b = std::max(1u, std::min(kPipeMaxChunk, nf / 8));
  while (b > 1 && (size_t)b * per_frame > kPipeSlotBytes) b--;
  return b;
}

// Builds the pipeline on first use.  The context gets it only when every
// piece exists: a failure leaves the context as it was, and the next call
// tries again.
int pipe_init(myyuv_hip_ctx* c) {
  if (c->pipe) return 0;
  auto p = std::make_unique<HostPipe>();
  if (hipStreamCreateWithFlags(&p->cin.h, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&p->cout.h, hipStreamNonBlocking) != hipSuccess)
    return MYYUV_E_HIP;
  int e = 0;
  for (auto& row : p->pev)
    for (auto& ev : row) e |= hipEventCreateWithFlags(&ev.h, hipEventDisableTiming) != hipSuccess;
  e |= hipHostMalloc(&p->hsz.h, 2 * kPipeMaxChunk * 4, hipHostMallocDefault) != hipSuccess;
  e |= hipHostMalloc(&p->herr.h, 2 * 8, hipHostMallocDefault) != hipSuccess;
  for (int k = 0; k < 2; k++) {
    e |= p->psz[k].grow(kPipeMaxChunk * 4);
    e |= p->perr[k].grow(8);
    if (!e) e |= hipMemset(p->perr[k].p, 0xFF, 8) != hipSuccess;
  }
  if (e) return MYYUV_E_HIP;
  c->pipe = std::move(p);
  return 0;
}

// Waits for every pipeline stream (an early return must not leave copies to
// or from the caller's buffers in flight).
struct PipeDrain {
  myyuv_hip_ctx* c;
  ~PipeDrain() {
    (void)hipStreamSynchronize(c->pipe->cin);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->pipe->cout);
  }
};

// The pipeline of both directions (tag: 'c' / 'd' in the trace).  A frame
// takes in_slot / out_slot bytes of a slot's input / output buffer, and
// mid_slot bytes (0: none) of c->dframes, a chunk's scratch between two of
// its kernels.  The
// direction's own steps, each for the n frames from f0 on in slot sl:
//   upload(P, sl, f0, n)       queues the chunk's host -> device copies on P.cin
//   run(P, GK, sl, perr, s)    launches its kernels on s (error word: perr)
//   download(P, sl, f0, n)     once they are done: queues the device -> host copies on P.cout
extern "C++" template <class Upload, class Run, class Download>
int pipe_frames(myyuv_hip_ctx* c, char tag, uint32_t nf, uint32_t w, uint32_t h, const uint8_t q[3],
                size_t in_slot, size_t out_slot, size_t mid_slot, int64_t* bad_block, Upload upload, Run run,
                Download download) {
  FrameGeom G;
  int e = make_geom(w, h, G);
  if (e) return e;
  const uint32_t B = std::min(pipe_chunk(nf, in_slot + out_slot), launch_frames(G, c->launch_blocks));
  FrameGeom GB = G;
  if ((e = set_batch(GB, B))) return e;
  Entry en(c);
  hipStream_t s = en.s;
  if ((e = pipe_init(c)) || (e = reserve(c, GB)) || (e = set_qtables(c, q, s))) return e;
  HostPipe& P = *c->pipe;
  for (int k = 0; k < 2; k++)
    if (P.pin[k].grow(in_slot * B) || P.pout[k].grow(out_slot * B)) return MYYUV_E_HIP;
  if (c->dframes.grow(mid_slot * B)) return MYYUV_E_HIP;  // (kernels run one chunk at a time: one slot)
  PipeDrain drain{c};
  const uint32_t nchunks = ceil_div(nf, B);
  // chunk k's sizes and error word are on the host: its results go back
  auto finish = [&](uint32_t k) -> int {
    const uint32_t sl = k & 1, f0 = k * B, n = std::min(B, nf - f0);
    PIPE_TRACE("pipe %c finish %u: wait kernels\n", tag, k);
    if (hipEventSynchronize(P.pev[1][sl]) != hipSuccess) return MYYUV_E_HIP;
    PIPE_TRACE("pipe %c finish %u: kernels done\n", tag, k);
    if (int ce = chunk_err(*P.err(sl), f0, G.cum[3], bad_block)) return ce;
    if (int de = download(P, sl, f0, n)) return de;
    PIPE_TRACE("pipe %c finish %u: downloads queued\n", tag, k);
    return hipEventRecord(P.pev[2][sl], P.cout) == hipSuccess ? 0 : MYYUV_E_HIP;
  };
  PIPE_TRACE("pipe %c: %u frames, chunks of %u\n", tag, nf, B);
  for (uint32_t k = 0; k < nchunks; k++) {
    const uint32_t sl = k & 1, f0 = k * B, n = std::min(B, nf - f0);
    FrameGeom GK = G;
    if ((e = set_batch(GK, n))) return e;
    PIPE_TRACE("pipe %c chunk %u: upload\n", tag, k);
    // upload (slot free once chunk k-2's kernels have read it)
    if (k >= 2 && hipStreamWaitEvent(P.cin, P.pev[1][sl], 0) != hipSuccess) return MYYUV_E_HIP;
    if ((e = upload(P, sl, f0, n))) return e;
    if (hipEventRecord(P.pev[0][sl], P.cin) != hipSuccess) return MYYUV_E_HIP;
    PIPE_TRACE("pipe %c chunk %u: uploads queued\n", tag, k);
    // kernels (output slot free once chunk k-2's results are back)
    if (hipStreamWaitEvent(s, P.pev[0][sl], 0) != hipSuccess ||
        (k >= 2 && hipStreamWaitEvent(s, P.pev[2][sl], 0) != hipSuccess))
      return MYYUV_E_HIP;
    unsigned long long* perr = P.perr[sl].as<unsigned long long>();
    if ((e = run(P, GK, sl, perr, s))) return e;
    if (hipMemcpyAsync(P.err(sl), perr, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemsetAsync(perr, 0xFF, 8, s) != hipSuccess || hipEventRecord(P.pev[1][sl], s) != hipSuccess)
      return MYYUV_E_HIP;
    if (k >= 1 && (e = finish(k - 1))) return e;
  }
  if ((e = finish(nchunks - 1))) return e;
  PIPE_TRACE("pipe %c: wait downloads\n", tag);
  if (hipStreamSynchronize(P.cout) != hipSuccess) return MYYUV_E_HIP;
  PIPE_TRACE("pipe %c: done\n", tag);
  if (c->prof) drain_profile(c);
  return 0;
}

int compress_frames(myyuv_hip_ctx* c, const uint8_t* const* frames, uint32_t nf, uint32_t w, uint32_t h,
                    const uint8_t q[3], myyuv_payload_alloc_fn alloc, void* user, uint32_t* sizes) {
  const size_t fb = (size_t)w * h * 3 / 2;
  const uint32_t dcap = (myyuv_dct_payload_bound(w, h) + 3) & ~3u;  // device slot per frame
  return pipe_frames(
      c, 'c', nf, w, h, q, fb, dcap, 0, nullptr,
      [&](HostPipe& P, uint32_t sl, uint32_t f0, uint32_t n) {
        int e = 0;
        for (uint32_t i = 0; i < n && !e; i++)
          e = h2d(P.pin[sl].as<uint8_t>() + i * fb, frames[f0 + i], fb, P.cin);
        return e;
      },
      [&](HostPipe& P, const FrameGeom& GK, uint32_t sl, unsigned long long* perr, hipStream_t s) {
        if (int e = launch_compress(c, GK, P.pin[sl].p, P.pout[sl].p, dcap, P.psz[sl].as<uint32_t>(), s, perr))
          return e;
        return hipMemcpyAsync(P.sizes(sl), P.psz[sl].p, (size_t)GK.nframes * 4, hipMemcpyDeviceToHost, s) == hipSuccess
                   ? 0
                   : MYYUV_E_HIP;
      },
      [&](HostPipe& P, uint32_t sl, uint32_t f0, uint32_t n) {
        for (uint32_t i = 0; i < n; i++) {
          const uint32_t size = P.sizes(sl)[i];
          sizes[f0 + i] = size;
          uint8_t* dst = alloc(user, f0 + i, size);
          if (!dst) return MYYUV_E_CAPACITY;
          if (hipMemcpyAsync(dst, P.pout[sl].as<uint8_t>() + (size_t)i * dcap, size, hipMemcpyDeviceToHost, P.cout) !=
              hipSuccess)
            return MYYUV_E_HIP;
        }
        return 0;
      });
}

// K8 behind the decoder (decompress_to_bmp_frames): how the frames leave
struct ToBmp {
  uint32_t orient, chroma;
  uint16_t bits;
};

// Streams -> frames[f]: the IYUV frame, or (bmp) its BMP pixel array, which
// K8 writes into the output slot from the chunk's frames in c->dframes.
int decompress_frames(myyuv_hip_ctx* c, const uint8_t* const* payloads, const uint32_t* psizes, uint32_t nf,
                      uint32_t w, uint32_t h, const uint8_t q[3], uint8_t* const* frames, int64_t* bad_block,
                      const ToBmp* bmp = nullptr) {
  const size_t fb = (size_t)w * h * 3 / 2;
  const size_t ob = bmp ? (size_t)w * h * (bmp->bits / 8) : fb;  // output bytes per frame
  uint32_t icap = 4;  // device slot per stream: the longest, 4-aligned
  for (uint32_t f = 0; f < nf; f++) icap = std::max(icap, (psizes[f] + 3u) & ~3u);
  return pipe_frames(
      c, 'd', nf, w, h, q, icap, ob, bmp ? fb : 0, bad_block,
      [&](HostPipe& P, uint32_t sl, uint32_t f0, uint32_t n) {
        uint8_t* slot = P.pin[sl].as<uint8_t>();
        for (uint32_t i = 0; i < n; i++) {
          const uint32_t sz = psizes[f0 + i], cap_i = (sz + 3u) & ~3u;
          // the stream's last word zero-padded (the scan reads whole words), then the bytes
          if ((cap_i >= 4 && hipMemsetAsync(slot + (size_t)i * icap + cap_i - 4, 0, 4, P.cin) != hipSuccess) ||
              h2d(slot + (size_t)i * icap, payloads[f0 + i], sz, P.cin))
            return MYYUV_E_HIP;
        }
        return h2d(P.psz[sl].p, psizes + f0, (size_t)n * 4, P.cin);
      },
      [&](HostPipe& P, const FrameGeom& GK, uint32_t sl, unsigned long long* perr, hipStream_t s) {
        if (!bmp)
          return launch_decompress(c, GK, P.pin[sl].p, P.psz[sl].as<const uint32_t>(), icap, P.pout[sl].p, s, perr);
        if (int e = launch_decompress(c, GK, P.pin[sl].p, P.psz[sl].as<const uint32_t>(), icap, c->dframes.p, s, perr))
          return e;
        return launch_to_bmp(c, c->dframes.p, w, h, GK.nframes, bmp->orient, bmp->bits, bmp->chroma, P.pout[sl].p, s);
      },
      [&](HostPipe& P, uint32_t sl, uint32_t f0, uint32_t n) {
        for (uint32_t i = 0; i < n; i++)
          if (hipMemcpyAsync(frames[f0 + i], P.pout[sl].as<uint8_t>() + i * ob, ob, hipMemcpyDeviceToHost, P.cout) !=
              hipSuccess)
            return MYYUV_E_HIP;
        return 0;
      });
}

struct SlotAlloc {
  uint8_t* base;
  uint32_t cap;
};
uint8_t* slot_alloc(void* user, uint32_t frame, uint32_t size) {
  const SlotAlloc* a = static_cast<const SlotAlloc*>(user);
  return size <= a->cap ? a->base + (size_t)frame * a->cap : nullptr;
}

}  // namespace

int myyuv_gpu_dct_compress_frames(myyuv_hip_handle c, const uint8_t* const* frames, uint32_t nframes, uint32_t w,
                                  uint32_t h, const uint8_t q[3], myyuv_payload_alloc_fn alloc, void* user,
                                  uint32_t* sizes) {
  if (!c || !frames || !alloc || !sizes || !q || nframes == 0) return MYYUV_E_ARG;
  for (uint32_t f = 0; f < nframes; f++)
    if (!frames[f]) return MYYUV_E_ARG;
  if (int e = check_q(q)) return e;
  return compress_frames(c, frames, nframes, w, h, q, alloc, user, sizes);
}

int myyuv_gpu_dct_compress_batch(myyuv_hip_handle c, const uint8_t* iyuv, uint32_t nframes, uint32_t w,
                                 uint32_t h, const uint8_t q[3], uint8_t* payloads, uint32_t cap,
                                 uint32_t* sizes) {
  if (!c || !iyuv || !payloads || !sizes || !q || nframes == 0) return MYYUV_E_ARG;
  if (int e = check_q(q)) return e;
  const size_t fb = (size_t)w * h * 3 / 2;
  std::vector<const uint8_t*> fr(nframes);
  for (uint32_t f = 0; f < nframes; f++) fr[f] = iyuv + f * fb;
  SlotAlloc a{payloads, cap};
  return compress_frames(c, fr.data(), nframes, w, h, q, slot_alloc, &a, sizes);
}

int myyuv_gpu_dct_decompress_frames(myyuv_hip_handle c, const uint8_t* const* payloads, const uint32_t* sizes,
                                    uint32_t nframes, uint32_t w, uint32_t h, const uint8_t q[3],
                                    uint8_t* const* frames, int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payloads || !sizes || !frames || !q || nframes == 0) return MYYUV_E_ARG;
  for (uint32_t f = 0; f < nframes; f++)
    if (!payloads[f] || !frames[f]) return MYYUV_E_ARG;
  if (int e = check_q(q)) return e;
  // every stream's DCTYUV::load checks first (DCT.cpp:454; the single-frame
  // call's order), frame by frame
  for (uint32_t f = 0; f < nframes; f++)
    if (int e = host_parse_headers(payloads[f], sizes[f])) return e;
  return decompress_frames(c, payloads, sizes, nframes, w, h, q, frames, bad_block);
}

int myyuv_gpu_dct_decompress_batch(myyuv_hip_handle c, const uint8_t* payloads, const uint32_t* sizes, uint32_t cap,
                                   uint32_t nframes, uint32_t w, uint32_t h, const uint8_t q[3], uint8_t* iyuv,
                                   int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payloads || !sizes || !iyuv || !q || nframes == 0) return MYYUV_E_ARG;
  for (uint32_t f = 0; f < nframes; f++)
    if (sizes[f] > cap) return MYYUV_E_ARG;
  const size_t fb = (size_t)w * h * 3 / 2;
  std::vector<const uint8_t*> in(nframes);
  std::vector<uint8_t*> out(nframes);
  for (uint32_t f = 0; f < nframes; f++) {
    in[f] = payloads + (size_t)f * cap;
    out[f] = iyuv + f * fb;
  }
  return myyuv_gpu_dct_decompress_frames(c, in.data(), sizes, nframes, w, h, q, out.data(), bad_block);
}

int myyuv_gpu_dct_decompress_to_bmp_frames(myyuv_hip_handle c, const uint8_t* const* payloads, const uint32_t* sizes,
                                           uint32_t nframes, int32_t width, int32_t height, const uint8_t q[3],
                                           uint16_t bit_count, uint32_t chroma, uint8_t* const* bmps,
                                           int64_t* bad_block) {
  if (bad_block) *bad_block = -1;
  if (!c || !payloads || !sizes || !bmps || !q || nframes == 0 || !chroma_ok(chroma)) return MYYUV_E_ARG;
  for (uint32_t f = 0; f < nframes; f++)
    if (!payloads[f] || !bmps[f]) return MYYUV_E_ARG;
  if (int e = check_q(q)) return e;
  for (uint32_t f = 0; f < nframes; f++)
    if (int e = host_parse_headers(payloads[f], sizes[f])) return e;
  uint32_t w = 0, h = 0;
  ToBmp t{0, chroma, bit_count};
  if (int e = bmp_check(width, height, bit_count, &w, &h, &t.orient)) return e;
  return decompress_frames(c, payloads, sizes, nframes, w, h, q, bmps, bad_block, &t);
}

int myyuv_hip_profile(myyuv_hip_handle c, int enable) {
  return myyuv_hip_profile_kernels(c, enable ? (1u << MYYUV_K_CEIL) - 1u : 0u);
}

int myyuv_hip_profile_kernels(myyuv_hip_handle c, uint32_t mask) {
  if (!c) return MYYUV_E_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  (void)hipStreamSynchronize(c->stream);
  drain_profile(c);
  c->prof = mask & ((1u << MYYUV_K_CEIL) - 1u);
  for (int k = 0; k < MYYUV_K_CEIL; k++) {
    c->ms[k] = 0;
    c->launches[k] = 0;
  }
  return 0;
}

int myyuv_hip_kernel_stats_n(myyuv_hip_handle c, uint32_t n, double* ms, int64_t* launches) {
  if (!c || !ms || !launches) return MYYUV_E_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  drain_profile(c);
  for (uint32_t k = 0; k < n; k++) {
    ms[k] = k < MYYUV_K_CEIL ? c->ms[k] : 0.0;
    launches[k] = k < MYYUV_K_CEIL ? c->launches[k] : 0;
  }
  return 0;
}

// (the first MYYUV_K_COUNT ids: the length its callers' arrays have)
int myyuv_hip_kernel_stats(myyuv_hip_handle c, double ms[MYYUV_K_COUNT],
                           int64_t launches[MYYUV_K_COUNT]) {
  return myyuv_hip_kernel_stats_n(c, MYYUV_K_COUNT, ms, launches);
}

}  // extern "C"

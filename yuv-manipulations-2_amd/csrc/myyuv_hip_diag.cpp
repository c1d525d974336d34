// myyuv_hip_diag.cpp — the diagnostic and known-answer entry points of the C
// ABI (include/myyuv_hip.h): myyuv_debug_*, and the block-level K1 / K2 calls.
// The product's host code is myyuv_hip.cpp; nothing here is on its path.
#include "host_ctx.hpp"

// READ_STAMPS(array, out, n, cap, elem, clear): the first n elements (at most
// cap) of elem bytes of a device stamp array, which is then zeroed when
// `clear` is set.  The arrays exist in diagnostic builds (-DMYYUV_STAMPS);
// MYYUV_E_ARG in normal builds.
#ifdef MYYUV_STAMPS
namespace myyuv_gpu {
extern __device__ unsigned long long g_k2_stamps[40];
extern __device__ uint32_t g_k2_wstamps[65536 * 8];
extern __device__ uint32_t g_k2_fstamps[8192 * 8];
extern __device__ uint32_t g_dec_wstamps[65536 * 8];
extern __device__ uint32_t g_k2_win[65536 * 8];
}  // namespace myyuv_gpu
static int read_stamps(const void* symbol, void* out, uint32_t n, uint32_t cap, size_t elem, bool clear) {
  const size_t bytes = (size_t)std::min(n, cap) * elem;
  if (hipMemcpyFromSymbol(out, symbol, bytes) != hipSuccess) return MYYUV_E_HIP;
  const std::vector<uint8_t> zero(bytes, 0);
  return !clear || hipMemcpyToSymbol(symbol, zero.data(), bytes) == hipSuccess ? 0 : MYYUV_E_HIP;
}
#define READ_STAMPS(sym, ...) read_stamps(HIP_SYMBOL(sym), __VA_ARGS__)
#else
#define READ_STAMPS(sym, ...) MYYUV_E_ARG
#endif

namespace {

constexpr uint8_t kZigzag[64] = MYYUV_ZIGZAG;

// The first n blocks of the context's coefficient image (the quad layout of
// codec_common.hpp) in natural order, as int16[n][64]; rows outside the row
// mask are not stored: zero.
int read_coef(myyuv_hip_ctx* c, uint32_t n, int16_t* out) {
  std::vector<uint4> img((size_t)ceil_div(n, kWave) * kCoefQuadsPerWave);
  std::vector<uint8_t> rm(n);
  if (hipStreamSynchronize(c->stream) != hipSuccess ||
      hipMemcpy(img.data(), c->coef.p, img.size() * 16, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(rm.data(), c->rmask.p, n, hipMemcpyDeviceToHost) != hipSuccess)
    return MYYUV_E_HIP;
  for (uint32_t b = 0; b < n; b++)
    for (uint32_t r = 0; r < 8; r++) {
      if ((rm[b] >> r) & 1u)
        std::memcpy(out + (size_t)b * 64 + r * 8, &img[coef_quad(b, r)], 16);
      else
        std::memset(out + (size_t)b * 64 + r * 8, 0, 16);
    }
  return 0;
}

// K2 and its overflow passes (launch_huff_encode) over nframes x nblocks
// coefficient blocks given in zig-zag order: a batch of nframes one-plane
// frames of nblocks blocks each (block_geom; nframes = 1: a single frame, with
// the single-frame gates).  chunks160 / sizes: per block, batch order.
// counts (may be null): work[0], the length of K2's overflow list; work[1],
// how many of them the CAP-16 tier listed again (0 when it did not run); and
// the chunk bytes the launch booked in its tiles' info words, which K4 places
// the chunks by: the overflow passes' (word 0; a block encoded by two passes
// is booked twice) and K2's dense runs' (words 1..4), each summed over the tiles.
int huff_encode_blocks(myyuv_hip_ctx* c, const int16_t* coef_zz, uint32_t nblocks, uint32_t nframes,
                       uint8_t* chunks160, uint8_t* sizes, uint32_t counts[4]) {
  if (!c || !coef_zz || !chunks160 || !sizes || nblocks == 0 || nframes == 0) return MYYUV_E_ARG;
  if ((uint64_t)nblocks * nframes > kMaxLaunchBlocks) return MYYUV_E_ARG;
  const uint32_t ntotal = nblocks * nframes;
  // the chunk format carries 11-bit symbols (pack11bit, Huffman.cpp:36-52);
  // K1 never produces others (DCT.cpp:276 asserts the range)
  for (size_t i = 0; i < (size_t)ntotal * 64; i++)
    if (coef_zz[i] < -1024 || coef_zz[i] > 1023) return MYYUV_E_ARG;
  Entry en(c);
  hipStream_t s = en.s;
  FrameGeom G = block_geom(nblocks);
  G.nframes = nframes;
  if (reserve(c, G)) return MYYUV_E_HIP;
  const uint32_t nwaves = ceil_div(ntotal, kWave);
  // host-side relayout into K1's output format: natural-order quads
  // and the per-block words K1 writes for K2's classification (binfo_word;
  // every row marked present)
  std::vector<uint32_t> words((size_t)nwaves * kCoefQuadsPerWave * 4, 0u), info(ntotal);
  for (uint32_t g = 0; g < ntotal; g++) {
    int16_t nat[64];
    uint32_t nnz = 0, msz = 0;
    for (int z = 0; z < 64; z++) {
      const int16_t v = coef_zz[(size_t)g * 64 + z];
      nat[kZigzag[z]] = v;
      if (v != 0) {
        nnz++;
        msz = (uint32_t)z + 1u;
      }
    }
    for (uint32_t c4 = 0; c4 < 8; c4++)
      std::memcpy(&words[(size_t)coef_quad(g, c4) * 4], nat + 8 * c4, 16);
    info[g] = binfo_word(0xFFu, msz, class_of(nnz, msz), (uint32_t)(uint16_t)nat[0]);
  }
  if (hipMemcpy(c->coef.p, words.data(), words.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->binfo.p, info.data(), (size_t)ntotal * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemsetAsync(c->rmask.p, 0xFF, ntotal, s) != hipSuccess ||  // every row present
      // work[0]: K1 zeroes it in the codec path; work[1]: launch_overflow
      // zeroes it when the tier runs, here also when it does not (`counts`)
      hipMemsetAsync(c->work.p, 0, 8, s) != hipSuccess)
    return MYYUV_E_HIP;
  if (launch_huff_encode(c, G, s)) return MYYUV_E_HIP;
  // K2's hand-off (codec_common.hpp): per tile the waves' dense runs, the
  // chunks of blocks with more than 8 symbols in their own slots
  const uint32_t ntile = nframes * G.tcum[3];
  std::vector<uint8_t> stage((size_t)win_tiles_alloc(ntile) * kTileCap), oslots((size_t)ntotal * kMaxChunk);
  std::vector<uint32_t> soff(ntotal);
  std::vector<uint32_t> ti((size_t)ntile * kTInfoWords);
  uint32_t cnt[4] = {0, 0, 0, 0};
  if (hipMemcpyAsync(stage.data(), c->stage.p, stage.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(oslots.data(), c->oslots.p, oslots.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(soff.data(), c->srcoff.p, (size_t)ntotal * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(sizes, c->sizes.p, ntotal, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(cnt, c->work.p, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(ti.data(), c->tinfo.p, ti.size() * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return MYYUV_E_HIP;
  for (uint32_t t = 0; t < ntile; t++) {
    cnt[2] += ti[(size_t)t * kTInfoWords];
    for (uint32_t w = 1; w <= kK2Group / kWave; w++) cnt[3] += ti[(size_t)t * kTInfoWords + w];
  }
  if (counts) std::memcpy(counts, cnt, sizeof(cnt));
  const uint32_t W = k2_win(ntile);
  for (uint32_t g = 0; g < ntotal; g++) {
    uint8_t* dst = chunks160 + (size_t)g * kMaxChunk;
    std::memset(dst, 0, kMaxChunk);
    if (src_is_single(soff[g])) {  // no stored chunk: the marker's closed form
      uint32_t w[2];
      single_chunk_words(soff[g], w[0], w[1]);
      std::memcpy(dst, w, std::min<uint32_t>(sizes[g], sizeof(w)));
      continue;
    }
    const uint8_t* src = soff[g] == kSrcOverflow
                             ? oslots.data() + (size_t)g * kMaxChunk
                             : stage.data() + (size_t)win_first_tile(tile_of_block(G, g), W) * kTileCap + soff[g];
    std::memcpy(dst, src, std::min<uint32_t>(sizes[g], kMaxChunk));  // (a size no pass wrote may hold anything)
  }
  return 0;
}

// K1 and its exact path (launch_fdct) over nblocks pixel blocks of one plane
// (block_geom), one Q table; the coefficients in zig-zag order.  listed /
// counts (may both be null): the launch's fix lists as K1 left them (its
// parity's counts; k_fdct_fix zeroes only the other parity's), read after
// the stream is synchronised.  listed[g] = 1 for each entry ua * 16 + b,
// counts[0] the number of entries, counts[1] the longest list.  An entry past
// the blocks, in another list than ua % kFixLists or listed twice, or a count
// above fix_list_cap, is kDiagFixList.
constexpr int kDiagFixList = 101;  // (diagnostic only: not a MYYUV_E_* code of include/myyuv_hip.h)
int fdct_blocks(myyuv_hip_ctx* c, const uint8_t* px, uint32_t nblocks, const float qtable[64], int16_t* coef_zz,
                uint8_t* listed, uint32_t counts[2]) {
  if (!c || !px || !qtable || !coef_zz || nblocks == 0) return MYYUV_E_ARG;
  Entry en(c);
  hipStream_t s = en.s;
  const FrameGeom G = block_geom(nblocks);
  QTables t;
  std::memset(&t, 0, sizeof(t));
  std::memcpy(t.q[0], qtable, 256);
  finish_qtables(t, 1);
  if (reserve(c, G) || c->frame.grow((size_t)nblocks * 64) || c->qtd.grow(sizeof(QTables)))
    return MYYUV_E_HIP;
  c->q_valid = false;
  if (hipStreamSynchronize(s) != hipSuccess ||
      hipMemcpy(c->qtd.p, &t, sizeof(t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->frame.p, px, (size_t)nblocks * 64, hipMemcpyHostToDevice) != hipSuccess)
    return MYYUV_E_HIP;
  const uint32_t par = c->fix_par;  // (launch_fdct uses it and flips it)
  if (launch_fdct(c, G, c->frame.as<const uint8_t>(), c->qtd.as<const QTables>(), nullptr, s))
    return MYYUV_E_HIP;
  if (hipGetLastError() != hipSuccess || read_coef(c, nblocks, coef_zz)) return MYYUV_E_HIP;
  for (uint32_t g = 0; g < nblocks; g++) {  // natural -> zigzag order
    int16_t nat[64];
    std::memcpy(nat, coef_zz + (size_t)g * 64, sizeof(nat));
    for (int z = 0; z < 64; z++) coef_zz[(size_t)g * 64 + z] = nat[kZigzag[z]];
  }
  if (!listed) return 0;
  const uint32_t units = G.ucum[3] * G.nframes, cap = fix_list_cap(units);
  std::vector<uint32_t> fix(fix_words(units));
  if (fix.size() * 4 > c->fix.n ||  // (read_coef synchronised the stream)
      hipMemcpy(fix.data(), c->fix.p, fix.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return MYYUV_E_HIP;
  std::memset(listed, 0, nblocks);
  counts[0] = counts[1] = 0;
  for (uint32_t l = 0; l < kFixLists; l++) {
    const uint32_t n = *fix_count(fix.data(), par, l);
    if (n > cap) return kDiagFixList;
    counts[0] += n;
    counts[1] = std::max(counts[1], n);
    const uint32_t* list = fix_list(fix.data(), G, l);
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t g = list[i];  // ua * 16 + b; one plane: the block's index
      if (g >= nblocks || g / kXfUnit % kFixLists != l || listed[g]) return kDiagFixList;
      listed[g] = 1;
    }
  }
  return 0;
}

}  // namespace

extern "C" {

// Per-wave stage cycles of the CAP=8 pass (n waves x 8 words).
int myyuv_debug_k2_fstamps(uint32_t* out, uint32_t n) { return READ_STAMPS(g_k2_fstamps, out, n, 8192, 32, false); }

// K2's per-wave window phases of the last launch, n waves x 8 words
// (k_huff_encode.hip g_k2_win; word 7 = 1 for a wave that ran), then zeroed.
int myyuv_debug_k2_win(uint32_t* out, uint32_t n) { return READ_STAMPS(g_k2_win, out, n, 65536, 32, true); }

// Per-block phase cycles of the wave encoder (n blocks x 8 words).
int myyuv_debug_k2_wstamps(uint32_t* out, uint32_t n) { return READ_STAMPS(g_k2_wstamps, out, n, 65536, 32, false); }

// The fused decoder's per-phase wave cycles of the last launch, n waves x 8
// words (k_huff_decode.hip g_dec_wstamps; word 7 = 1 for a wave that ran),
// then zeroed.
int myyuv_debug_dec_stamps(uint32_t* out, uint32_t n) { return READ_STAMPS(g_dec_wstamps, out, n, 65536, 32, true); }

// Summed per-stage wave cycles of K2 since the last call.
int myyuv_debug_k2_stamps(unsigned long long out[40]) { return READ_STAMPS(g_k2_stamps, out, 40, 40, 8, true); }

// Diagnostic: stop launching the kernels whose bit (1 << MYYUV_K_*) is set,
// to measure each kernel's share of a pipelined run.  The buffers keep what the
// last real launch wrote, so repeating identical frames still decodes.
int myyuv_debug_skip_kernels(myyuv_hip_handle c, uint32_t mask) {
  if (!c) return MYYUV_E_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  c->skip = mask;
  return 0;
}

// Diagnostic: the coefficient image of the last compress/decompress, n
// blocks, as int16[n][64] in natural order.
int myyuv_debug_coef(myyuv_hip_handle c, int16_t* out, uint32_t n) {
  if (!c || !out) return MYYUV_E_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if ((size_t)ceil_div(n, kWave) * kCoefQuadsPerWave * 16 > c->coef.n || n > c->rmask.n) return MYYUV_E_ARG;
  return read_coef(c, n, out);
}

// Diagnostic: the tile-info guard band.  arm != 0 fills the kWinTilesBig x
// kTInfoWords words after tile ntiles (the batch's last tile) with a canary;
// arm == 0 returns in *changed how many of them no longer hold it (a kernel
// wrote past the batch's tiles: the K2 window overrun of round 5's advice).
int myyuv_debug_tinfo_guard(myyuv_hip_handle c, uint32_t ntiles, int arm, uint32_t* changed) {
  if (!c) return MYYUV_E_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  constexpr uint32_t kGuardWords = kWinTilesBig * kTInfoWords;
  constexpr uint32_t kCanary = 0xA5C3E1F7u;
  const size_t off = (size_t)ntiles * kTInfoWords * 4;
  if (off + kGuardWords * 4 > c->tinfo.n) return MYYUV_E_ARG;
  std::vector<uint32_t> w(kGuardWords, kCanary);
  if (hipStreamSynchronize(c->stream) != hipSuccess) return MYYUV_E_HIP;
  uint8_t* p = static_cast<uint8_t*>(c->tinfo.p) + off;
  if (arm) return hipMemcpy(p, w.data(), kGuardWords * 4, hipMemcpyHostToDevice) == hipSuccess ? 0 : MYYUV_E_HIP;
  if (!changed) return MYYUV_E_ARG;
  if (hipMemcpy(w.data(), p, kGuardWords * 4, hipMemcpyDeviceToHost) != hipSuccess) return MYYUV_E_HIP;
  uint32_t n = 0;
  for (uint32_t v : w) n += v != kCanary;
  *changed = n;
  return 0;
}

// ---- block-level KAT entry points -----------------------------------------
int myyuv_gpu_fdct_blocks(myyuv_hip_handle c, const uint8_t* px, uint32_t nblocks,
                          const float qtable[64], int16_t* coef_zz) {
  return fdct_blocks(c, px, nblocks, qtable, coef_zz, nullptr, nullptr);
}

// Diagnostic: myyuv_gpu_fdct_blocks, and which blocks K1 listed for its exact
// path: listed[g] = 1 for each entry of the launch's lists, counts[0] the
// number of entries, counts[1] the longest list (fdct_blocks above).
// 101 (kDiagFixList) when the lists are not what K1 may write.
int myyuv_debug_fdct_blocks(myyuv_hip_handle c, const uint8_t* px, uint32_t nblocks, const float qtable[64],
                            int16_t* coef_zz, uint8_t* listed, uint32_t counts[2]) {
  if (!listed || !counts) return MYYUV_E_ARG;
  return fdct_blocks(c, px, nblocks, qtable, coef_zz, listed, counts);
}

int myyuv_gpu_huff_encode_blocks(myyuv_hip_handle c, const int16_t* coef_zz, uint32_t nblocks,
                                 uint8_t* chunks160, uint8_t* sizes) {
  return huff_encode_blocks(c, coef_zz, nblocks, 1, chunks160, sizes, nullptr);
}

// Diagnostic: myyuv_gpu_huff_encode_blocks over a batch of nframes frames of
// nblocks blocks each (coef_zz, chunks160, sizes: nframes x nblocks entries),
// returning the launch's two overflow list lengths and its booked overflow
// and dense chunk bytes in counts[0..3] (huff_encode_blocks above).
int myyuv_debug_huff_encode_blocks(myyuv_hip_handle c, const int16_t* coef_zz, uint32_t nblocks, uint32_t nframes,
                                   uint8_t* chunks160, uint8_t* sizes, uint32_t counts[4]) {
  if (!counts) return MYYUV_E_ARG;
  return huff_encode_blocks(c, coef_zz, nblocks, nframes, chunks160, sizes, counts);
}

// Diagnostic: the constants the overflow regimes switch on (codec_common.hpp),
// so that tests place list lengths at them without restating the values:
// kR16GateSingle, kR16Gate, kWaveEncodeLimit, kBatchWaveLimit, kK2Group, the
// blocks of one K2 window (kWinTiles tiles), and kOvfNub.
int myyuv_debug_k2_constants(uint32_t out[7]) {
  if (!out) return MYYUV_E_ARG;
  const uint32_t v[7] = {kR16GateSingle, kR16Gate, kWaveEncodeLimit, kBatchWaveLimit, kK2Group,
                         kWinTiles * kK2Group, kOvfNub};
  std::memcpy(out, v, sizeof(v));
  return 0;
}

}  // extern "C"

// host_ctx.hpp — what the two host translation units share: the kernels'
// declarations, the owners of HIP resources, the context, and the pieces every
// entry point is made of (myyuv_hip.cpp: the product; myyuv_hip_diag.cpp: the
// diagnostic and known-answer entry points).
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "bmp_fdct.h"
#include "codec_common.hpp"
#include "downscale.h"
#include "jpeg_export.h"
#include "jpeg_import.h"
#include "k_chain.hpp"
#include "k_stream.hpp"
#include "myyuv_hip.h"
#include "stream_gather.h"

namespace myyuv_gpu {
__global__ void k_fdct_quant(const uint8_t*, FrameGeom, const QTables*, uint4*, uint8_t*, uint32_t*, uint4*,
                             uint32_t*, uint32_t*, uint32_t);
__global__ void k_fdct_fix(const uint8_t*, FrameGeom, const QTables*, uint4*, uint8_t*, uint32_t*, uint4*,
                           uint32_t*, uint32_t);
__global__ void k_dequant_idct(const uint4*, const uint8_t*, const uint4*, FrameGeom, const QTables*, uint8_t*,
                               uint4*);
__global__ void k_decode_idct(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*, const uint32_t*,
                              const uint32_t*, FrameGeom, uint32_t, uint32_t, const QTables*, uint4*, uint8_t*,
                              unsigned long long*);
__global__ void k_decode_span(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*, const uint32_t*,
                              const uint32_t*, FrameGeom, uint32_t, uint32_t, const QTables*, uint4*, uint8_t*,
                              unsigned long long*);
__global__ void k_decode_region(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*, const uint32_t*,
                                const uint32_t*, FrameGeom, FrameGeom, RegionSegs, const QTables*, uint8_t*,
                                unsigned long long*);
template <int N>
__global__ void k_decode_scaled(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*, const uint32_t*,
                                const uint32_t*, FrameGeom, uint32_t, uint32_t, const QTables*, uint4*, uint8_t*,
                                unsigned long long*);
template <int N>
__global__ void k_downscale(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*, const uint32_t*,
                            const uint32_t*, FrameGeom, FrameGeom, myyuv_downscale::Map, const DownscaleTables*,
                            uint4*, uint8_t*, uint32_t*, unsigned long long*);
__global__ void k_requant(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*, const uint32_t*,
                          const uint32_t*, FrameGeom, uint32_t, uint32_t, const RequantTables*, uint4*, uint8_t*,
                          uint32_t*, unsigned long long*);
__global__ void k_coef_xform(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*, const uint32_t*,
                             const uint32_t*, FrameGeom, uint32_t, uint32_t, const RequantTables*, uint32_t, uint32_t,
                             uint4*, uint4*, uint8_t*, uint32_t*, unsigned long long*);
template <bool Write>
__global__ void k_jpeg_export(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*, const uint32_t*,
                              const uint32_t*, FrameGeom, uint32_t, uint32_t, uint4*, uint32_t*, const uint32_t*,
                              const uint32_t*, uint8_t*, uint32_t, unsigned long long*);
__global__ void k_jpeg_place(const uint32_t*, uint32_t*, uint32_t, uint32_t, uint32_t, myyuv_jpeg::Head, uint8_t*,
                             uint32_t, uint32_t*, unsigned long long*);
__global__ void k_jpeg_import(const uint32_t*, const myyuv_jpegin::Seg*, uint32_t, myyuv_jpegin::Plan,
                              const myyuv_jpegin::DecTab*, const RequantTables*, uint32_t, uint4*, uint8_t*, uint32_t*,
                              unsigned long long*);
__global__ void k_jpeg_import_coef(const uint4*, uint32_t, uint32_t, uint32_t, const RequantTables*, uint32_t, uint4*,
                                   uint8_t*, uint32_t*);
template <uint32_t W>
__global__ void k_huff_encode(const uint4*, const uint32_t*, const uint4*, FrameGeom, uint32_t*, uint32_t*,
                              uint8_t*, uint32_t*, uint32_t*, uint32_t*);
__global__ void k_huff_encode_wave(const uint4*, const uint8_t*, FrameGeom, uint32_t*, uint8_t*, uint32_t*,
                                   const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t,
                                   uint32_t);
__global__ void k_huff_encode_wide(const uint4*, const uint8_t*, const uint4*, FrameGeom, uint32_t*, uint8_t*,
                                   uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                                   uint32_t, uint32_t);
__global__ void k_huff_encode_r16(const uint4*, const uint8_t*, const uint4*, FrameGeom, uint32_t*, uint8_t*,
                                  uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t);
__global__ void k_encode_tile(const uint8_t*, FrameGeom, const QTables*, uint4*, uint8_t*, uint32_t*, uint32_t*,
                              uint8_t*, uint32_t*, uint32_t*, uint32_t*);
__global__ void k_tile_scan(uint32_t*, FrameGeom, uint8_t*, uint32_t, uint32_t*, unsigned long long*);
__global__ void k_scan_chain(const uint8_t*, uint32_t, ScanSrc, const uint32_t*, uint32_t, FrameGeom,
                             StreamDesc*, uint32_t*, uint32_t*, uint32_t, unsigned long long*,
                             uint32_t, unsigned long long*);
__global__ void k_stream_out(const uint32_t*, const uint32_t*, const uint8_t*, const uint32_t*,
                             const uint32_t*, FrameGeom, uint8_t*, uint32_t, uint32_t);
__global__ void k_huff_decode(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*,
                              const uint32_t*, const uint32_t*, FrameGeom, uint32_t, uint32_t,
                              uint4*, uint8_t*, unsigned long long*);
__global__ void k_gather_sizes(const uint8_t*, uint32_t, const StreamDesc*, myyuv_gather::GatherMap, uint8_t*);
__global__ void k_gather_heads(const uint32_t*, const uint32_t*, myyuv_gather::GatherMap, uint8_t*, uint32_t,
                               uint32_t, uint32_t*, unsigned long long*);
__global__ void k_gather_check(const uint8_t*, uint32_t, const StreamDesc*, const uint32_t*, const uint32_t*,
                               myyuv_gather::GatherMap, uint32_t, unsigned long long*);
__global__ void k_stream_gather(const uint8_t*, uint32_t, const StreamDesc*, const uint32_t*, const uint32_t*,
                                const uint8_t*, const uint32_t*, const uint32_t*, myyuv_gather::GatherMap, uint32_t,
                                uint8_t*, uint32_t, unsigned long long*);
__global__ void k_decode_compare(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*, const uint32_t*,
                                 const uint32_t*, FrameGeom, uint32_t, uint32_t, const QTables*, uint4*, const uint8_t*,
                                 uint32_t, uint4*, myyuv_block_metric*, unsigned long long*);
__global__ void k_frame_compare(const uint8_t*, uint32_t, const uint8_t*, FrameGeom, uint32_t, uint32_t, uint4*,
                                myyuv_block_metric*);
__global__ void k_metric_reduce(const uint4*, uint32_t, uint32_t, uint32_t, myyuv_frame_metric*);
__global__ void k_coef_compare(const uint4*, const uint8_t*, const uint4*, FrameGeom, const QTables*, const uint8_t*,
                               uint4*, myyuv_block_metric*, uint4*);
__global__ void k_probe_out(const uint32_t*, const uint32_t*, const myyuv_frame_metric*, uint32_t, uint32_t,
                            myyuv_probe*);
template <int BPP>
__global__ void k_bmp_to_iyuv(const uint8_t*, uint32_t, uint32_t, uint32_t, uint8_t*);
template <int BPP, int LINEAR>
__global__ void k_iyuv_to_bmp(const uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint8_t*);
template <int BPP>
__global__ void k_bmp_fdct(const uint8_t*, myyuv_bmpfdct::Map, FrameGeom, const QTables*, uint4*, uint8_t*, uint32_t*);
}  // namespace myyuv_gpu

using namespace myyuv_gpu;

// (nothing below is part of the library's ABI)
#pragma GCC visibility push(hidden)

// A HIP handle that is released with its owner (move-only).
template <class T, hipError_t (*Release)(T)>
struct Owned {
  T h = nullptr;
  Owned() = default;
  Owned(Owned&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Owned& operator=(Owned&& o) noexcept {
    std::swap(h, o.h);
    return *this;
  }
  ~Owned() {
    if (h) (void)Release(h);
  }
  operator T() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Pinned = Owned<void*, hipHostFree>;

// A device buffer that only grows (its content is lost when it does).
struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int grow(size_t want) {
    if (want <= n) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (hipMalloc(&p, want) != hipSuccess) return MYYUV_E_HIP;
    n = want;
    return 0;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

constexpr uint32_t kPipeMaxChunk = 8;

// The host-buffer batch pipeline (myyuv_hip.cpp, pipe_frames): H2D on cin,
// kernels on the context's stream, D2H on cout; two slots of up to
// kPipeMaxChunk frames.  (The streams first: they outlive what runs on them.)
struct HostPipe {
  Stream cin, cout;
  Event pev[3][2];  // [copied in, computed, copied out][slot]
  DevBuf pin[2], pout[2], psz[2], perr[2];
  Pinned hsz;   // 2 x kPipeMaxChunk u32 sizes
  Pinned herr;  // 2 error words
  uint32_t* sizes(uint32_t slot) const { return static_cast<uint32_t*>(hsz.h) + slot * kPipeMaxChunk; }
  unsigned long long* err(uint32_t slot) const { return static_cast<unsigned long long*>(herr.h) + slot; }
};

// (Members are destroyed in reverse order: everything after `stream` goes
// before it.)
struct myyuv_hip_ctx {
  int device = 0;
  Stream stream;
  // One context's scratch buffers (coef, slots, sizes, scan status words ...)
  // serve one call at a time: every entry point records `done` on its stream
  // and a call on another stream first waits for it (StreamOrder), so calls
  // on different streams through one context run in call order.
  Event done;
  hipStream_t last_stream = nullptr;
  DevBuf frame, coef, sizes, loff, tiles, payload, err, psize, desc, work, qtd;
  DevBuf stage, oslots, tinfo, srcoff;  // K2 -> K4 (codec_common.hpp)
  DevBuf bmp;   // staged BMP pixels (host-buffer BMP -> IYUV and back)
  DevBuf dframes;  // a chunk's decoded IYUV frames between the decoder and K8 (decompress_to_bmp_frames)
  DevBuf rmask; // per block: bit c = coefficient row c nonzero (K1 -> overflow passes, K5 -> K6)
  DevBuf binfo; // per block: K1 -> K2's classification (binfo_word, codec_common.hpp)
  DevBuf zq;    // 256 zero bytes: K6's source for rows the mask says are zero
  DevBuf sink;  // K1/K6 stores of lanes past a plane's end (128 x 16 B, never read)
  // K1 -> k_fdct_fix: the unproven units' lists and counts (fix_count /
  // fix_list, codec_common.hpp; fix_par alternates from launch to launch)
  DevBuf fix;
  uint32_t fix_par = 0;
  // K1, K6, k_coef_compare workgroups resident on the device
  uint32_t xf_resident[3] = {kXfWaves / 4, kXfWaves / 4, kXfWaves / 4};
  uint32_t fix_resident = kXfWaves / 4;                      // k_fdct_fix workgroups resident
  // k_fdct_fix's grid at qualities up to fix_qmax (MYYUV_FIX_GRID; 0, the
  // default: the resident count, as above fix_qmax).  A small fixed grid
  // measured no faster (profiles/r4h_fix_ab.txt), and busy content at low q
  // can list far more units than the bench frame's 0.07 %.
  uint32_t fix_grid = 0;
  uint32_t fix_qmax = 75;  // (MYYUV_FIX_QMAX)
  uint32_t launch_blocks = kMaxLaunchBlocks;  // blocks per launch (MYYUV_LAUNCH_BLOCKS: a test of the batch split)
  // encoder: K1 -> K2 through HBM (split), or the fused single-pass kernel
  // k_encode_tile (MYYUV_ENCODER=fused|split)
  bool fused = false;
  // decoder: fused (default), or K5 -> K6 through HBM (MYYUV_DECODER=split).
  // The fused decoder is k_decode_span (a wave per kDecSpan-block span) for
  // launches of at least dec_span_min 64-block groups (MYYUV_DEC_SPAN_MIN) and
  // k_decode_idct (a wave per group) below: a small launch has too few spans
  // to fill the chip.  MYYUV_DECODER=span / group: always the one / the other.
  bool fused_dec = true;
  uint32_t dec_span_min = kDecSpanMinDefault;
  // chained scan (k_chain.hpp): per-tile status words tagged with the launch
  // epoch, counted here
  DevBuf status;
  uint32_t epoch = 0;
  // quantisation tables of the last quality triple (host copy; qtd on the
  // device, rewritten in stream order when the triple changes)
  QTables qt;
  hipStream_t qt_stream = nullptr;
  uint8_t q_cached[3] = {0, 0, 0};
  bool q_valid = false;
  // the requantiser's two tables (RequantTables), cached the same way by the
  // (source, destination) quality triples; its own buffer, so qt / qtd and
  // their cache are untouched by a requantise call.  rqsrc: the host-buffer
  // call's staged source stream (`payload` takes its result)
  DevBuf rqt, rqsrc;
  RequantTables rq;
  hipStream_t rq_stream = nullptr;
  uint8_t rq_cached[6] = {0, 0, 0, 0, 0, 0};
  bool rq_valid = false;
  // the transform's use of the same tables: qs held as the transposed block
  // reads it (coef_xform.h xf_source_table) when rq_swap, which is part of the
  // cache key; rq_eq: bit p set when plane p's two tables, so held, are equal.
  // xfgen: the transform's scratch coefficient image for decode_general's
  // blocks (source block order; grown by that path alone)
  bool rq_swap = false;
  uint32_t rq_eq = 0;
  DevBuf xfgen;
  // the downscaler's tables (DownscaleTables: the source Q values and the
  // destination's QTables), cached by the (source, destination) quality
  // triples in a buffer of their own, as the requantiser's: qt / qtd and rq /
  // rqt and their caches are untouched by a downscale call
  DevBuf dst;
  DownscaleTables ds;
  hipStream_t ds_stream = nullptr;
  uint8_t ds_cached[6] = {0, 0, 0, 0, 0, 0};
  bool ds_valid = false;
  // crop and join: the output blocks' size bytes in destination order, and the
  // destination scan's group offsets and tile prefixes (the source scan's are
  // loff / tiles; the status words serve both scans, one after the other)
  DevBuf gsz, gloff, gtiles;
  // compare: the waves' totals (16 B per 64-block group) between the compare
  // kernels and k_metric_reduce; for the host-buffer calls the plane records,
  // the per-block map and the staged test frame (the reference frame is
  // staged in `frame`)
  DevBuf mpart, mrec, mmap, mtest;
  // probe: per frame the 12 stream-head bytes and the payload size the tile
  // scan writes, then an error word of its own (the scan reports a head-only
  // capacity as an overflow; nobody reads it); the host-buffer calls' records
  DevBuf pbsz, prec;
  // export to JPEG: per 64-block group the interval's size (the sizing
  // launch) and its file offset (k_jpeg_place); the host-buffer calls' file
  DevBuf jsz, joff, jout;
  // import from JPEG: the file (or the host-decoded coefficient image), the
  // segment table, the six decode tables and the call's rescale tables
  DevBuf jin, jseg, jtab, jrq;
  // profiling: the kernels' start/stop events until drain_profile reads
  // them; they are used again from launch to launch
  struct Stamp {
    int kid;
    Event start, stop;
  };
  uint32_t prof = 0;  // bit k: stamp kernel id k
  uint32_t skip = 0;  // diagnostic: bit k: do not launch kernel id k (myyuv_debug_skip_kernels)
  double ms[MYYUV_K_CEIL] = {};
  int64_t launches[MYYUV_K_CEIL] = {};
  std::vector<Stamp> pending;
  std::vector<Event> free_events;
  // set once every piece of it exists (pipe_init)
  std::unique_ptr<HostPipe> pipe;
  std::mutex mu;
  // Waits for everything the context queued (under a DeviceGuard of its device).
  ~myyuv_hip_ctx();
};

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// Orders a call on stream `s` after the context's previous call (see
// myyuv_hip_ctx::done); the record at scope exit publishes this call's work.
struct StreamOrder {
  myyuv_hip_ctx* c;
  hipStream_t s;
  StreamOrder(myyuv_hip_ctx* ctx, hipStream_t st) : c(ctx), s(st) {
    if (c->last_stream && c->last_stream != s) (void)hipStreamWaitEvent(s, c->done, 0);
  }
  ~StreamOrder() {
    if (hipEventRecord(c->done, s) == hipSuccess) c->last_stream = s;
  }
};

// An entry point's prologue: the context's lock, its device, the call's
// stream (NULL: the context's own) and its place in the call order.
struct Entry {
  std::lock_guard<std::mutex> lock;
  DeviceGuard dev;
  hipStream_t s;
  StreamOrder order;
  explicit Entry(myyuv_hip_ctx* c, void* stream = nullptr)
      : lock(c->mu), dev(c->device), s(stream ? static_cast<hipStream_t>(stream) : c->stream.h), order(c, s) {}
};

inline uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

inline Event take_event(myyuv_hip_ctx* c) {
  Event e;
  if (!c->free_events.empty()) {
    e = std::move(c->free_events.back());
    c->free_events.pop_back();
  } else {
    (void)hipEventCreate(&e.h);
  }
  return e;
}

// Launches kernel `k` on `s`.  When profiling, the start/stop events are the
// ones hipExtLaunchKernel stamps from the kernel's own dispatch packet: the
// kernel's execution time (what rocprofv3's kernel trace reports), without
// the few microseconds of queue latency a hipEventRecord bracket adds.
template <class... KArgs, class... Args>
int launch(myyuv_hip_ctx* c, int kid, void (*k)(KArgs...), dim3 grid, dim3 block, hipStream_t s,
           Args... args) {
  if ((c->skip >> kid) & 1u) return 0;
  Event a, b;
  const bool stamp = (c->prof >> kid) & 1u;
  if (stamp) {
    a = take_event(c);
    b = take_event(c);
  }
  hipExtLaunchKernelGGL(k, grid, block, 0, s, a.h, b.h, 0, static_cast<KArgs>(args)...);
  if (hipPeekAtLastError() != hipSuccess) {
    (void)hipGetLastError();
    return MYYUV_E_HIP;
  }
  if (stamp) c->pending.push_back({kid, std::move(a), std::move(b)});
  return 0;
}

// myyuv_hip.cpp
void drain_profile(myyuv_hip_ctx* c);
void finish_qtables(QTables& t, int planes);
// One plane of nblocks blocks, one block wide (the block-level known-answer
// entry points' geometry; planes 1 and 2 empty).
FrameGeom block_geom(uint32_t nblocks);
int reserve(myyuv_hip_ctx* c, const FrameGeom& G);
int launch_fdct(myyuv_hip_ctx* c, const FrameGeom& G, const uint8_t* in, const QTables* qt, uint32_t* k2ctl,
                hipStream_t s);
int launch_huff_encode(myyuv_hip_ctx* c, const FrameGeom& G, hipStream_t s);

#pragma GCC visibility pop

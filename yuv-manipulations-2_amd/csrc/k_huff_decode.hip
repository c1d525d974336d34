// k_huff_decode.hip — K5: per-block chunk parse + canonical Huffman decode on
// gfx950 (Huffman::fromDump, unpack11bit, decodeSymbol, decodeFromTreeData;
// myyuv_DCT/Huffman.cpp:243-277, :54-69, :106-154).
//
// One workgroup = one wave = up to 64 consecutive blocks of ONE plane, so the
// wave's chunks are one contiguous byte range of the plane's content[]; it is
// staged into LDS with 16-B loads issued together (the LDS image keeps the
// stream's 16-B grid; several rounds when it exceeds the 6 KiB stage), then
// each lane decodes its own block:
//   1. header: u16 nbits, u8 table_bytes;
//   2. table: one pass over the groups ((L-1)<<5 | (n-1)) + n x 11-bit values,
//      recording per length the code count and the bit address of its group.
//      No symbol table is unpacked: a decoded code's value is read in place
//      (11 bits at group_bit + 11 * rank), so the wave needs no LDS beyond
//      the stage;
//   3. symbols: the reference decodes bit-serially (puff style): at length L,
//      code = first L bits, match if code < first + count[L].  Here the next 8
//      bits are peeked from a 64-bit register window (refilled from LDS every
//      7 symbols, at most 56 bits apart) and:
//        * "regular" tables (every length in one group, first + count[L] <=
//          2^L: every table the reference writes) — the match conditions are
//          w8 < lim[L] with left-justified limits lim[L] = (first + count) <<
//          (8 - L), non-decreasing in L, so the matched length is 1 + #{L :
//          w8 >= lim[L]}: eight 16-bit compares in four SWAR subtractions;
//        * any other table (malformed or hand-made streams) — the bit-serial
//          conditions evaluated for L = 1..8 as the reference does (uint8
//          arithmetic of `first` kept), the value found by walking the groups
//          of that length in stream order (std::map<len, vector> append
//          semantics of tree_data).
//      Both give the reference's "bad code" / "unknown symbol" outcomes on
//      the same bit budget checks.
//   The symbol loop is unrolled over the 64 scan positions, so each decoded
//   value lands in a statically indexed register of the block's NATURAL-order
//   words (the de-zig-zag of Huffman.cpp:148-153 is free) and the block is
//   written as 8 quads of the codec_common.hpp layout that K6 reads.
#include "codec_common.hpp"
#include "coef_xform.h"
#include "downscale.h"
#include "huff_common.hpp"
#include "idct_scaled.h"
#include "jpeg_export.h"
#include "k1_store.hpp"
#include "k_metric.hpp"
#include "k_stream.hpp"
#include "requant.h"
#include "xform_common.hpp"

namespace myyuv_gpu {

namespace {

// 5 KiB stage: 80 B of chunk per block on average (a 4K frame at q=50 uses
// ~12 B); a wave whose chunks do not fit is staged in several rounds.
constexpr uint32_t kStageQuads = 320;
// One zero quad after the stage (zeroed at kernel start, never staged into):
// the symbol loop reads a lane's value from it when the lane takes none, so
// the value needs no select.
constexpr uint32_t kZeroBit = kStageQuads * 128u;
// after the zero quad: the table parse's per-lane value positions, 8 u32 per
// lane, length-major (decode_regular reads one per symbol, conflict-free:
// an LDS read instead of a select between 64-bit register pairs, a 64-bit
// shift and an add)
constexpr uint32_t kGposQuads = 8 * 64 * 4 / 16;

#ifndef MYYUV_K5_GROUP
#define MYYUV_K5_GROUP 2  // positions per "any lane left" test (1 / 2 / 4 / 8: 132.4 / 128.2 / 129.0 / 135.1 us per launch, tools/runs/r3n.sh)
#endif
// The symbol loop's arithmetic in full-rate forms (1; 0: as the compiler
// picks them): the value's stage bit by a 24-bit multiply-add (the code has
// at most 8 bits; written as a 32-bit product the compiler emits the 64-bit
// v_mad_u64_u32), and the message's bit count as a register of its own
// (left packed with the table size, every comparison with it is an SDWA
// form)
#ifndef MYYUV_K5_FORMS
#define MYYUV_K5_FORMS 1
#endif
#ifndef MYYUV_K5S_WAVES
#define MYYUV_K5S_WAVES 5  // the split decoder's K5
#endif
#ifndef MYYUV_K5_WAVES
#define MYYUV_K5_WAVES 5
#endif



// (c_zz, the zig-zag order as compile-time constants: huff_common.hpp's)
__constant__ uint8_t c_zz_dev[64] = MYYUV_ZIGZAG;

__device__ __forceinline__ void record_error(unsigned long long* err, uint64_t key, int code) {
  atomicMin(err, (unsigned long long)((key << 8) | (uint64_t)code));
}


// Inclusive sum over the wave's 64 lanes by DPP (rows of 16 by row_shr 1, 2,
// 4, 8, then row_bcast 15 / 31 across rows; lanes whose source is out of
// range add the old value 0).  Every lane must be active: under a partial
// EXEC, inactive lanes pass nothing on (the DPP rule).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);  // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);  // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);  // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);  // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);  // row_bcast:15
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return x;
}

__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t s) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31));
}

// One lane's chunk in the LDS stage (b0: its first byte).  Bits are in the
// stream's order: bit k of the chunk is bit k & 7 of byte k >> 3.
struct LdsChunk {
  const uint32_t* st;
  uint32_t b0;
  __device__ __forceinline__ uint32_t byte(uint32_t i) const {
    return reinterpret_cast<const uint8_t*>(st)[b0 + i];
  }
  __device__ __forceinline__ uint32_t bits32(uint32_t bit) const {
    const uint32_t P = 8 * b0 + bit, w = P >> 5;
    return funnel(st[w + 1], st[w], P);
  }
};

struct Table {
  uint32_t nbits = 0;   // symbol bits
  uint32_t sbit = 0;    // chunk bit of the first symbol bit
  uint32_t tb = 0;      // table bytes
  uint64_t cnt = 0;     // code count of length L in byte L-1
  uint32_t lim[4] = {0, 0, 0, 0};   // 16-bit fields: left-justified limit, lengths 2k+1, 2k+2
  bool regular = true;
};

// Header + table (Huffman::fromDump, Huffman.cpp:243-277).  Returns 0 or the
// MYYUV_E_* code (12: bad chunk).
template <class Chunk>
__device__ __forceinline__ int parse_table(const Chunk& c, uint32_t s, Table& T, uint32_t* gcol) {
  // (no early returns: a bad header only sets `bad`, and the walk and the
  // per-length pass run on whatever was read (inside the stage); each return
  // path would otherwise re-initialise the outputs at its branch level)
  // the chunk's first 20 bytes in registers, loaded together: the group walk
  // below is a chain of dependent byte reads, from registers for every table
  // that ends within them (at most 8 symbols always do), from LDS for the
  // rest in a second walk; both walks branch-free (a dynamic byte index as a
  // select chain compiled to nested EXEC branches, ~90 instructions a group)
  // (five named values, not an array: selects between an array's elements
  // are turned into a dynamically indexed scratch array)
  const uint32_t h0 = c.bits32(0), h1 = c.bits32(32), h2 = c.bits32(64), h3 = c.bits32(96), h4 = c.bits32(128);
  const uint32_t nbits = h0 & 0xFFFFu;
  const uint32_t tb = (h0 >> 16) & 0xFFu;
  const bool bad_hdr = s < 3 || nbits > 512 || 3 + tb + (nbits + 7) / 8 > s;
  auto reg_byte = [=](uint32_t i) -> uint32_t {  // i < 20
    const uint32_t k = i >> 2;
    const uint32_t w01 = (k & 1u) ? h1 : h0;
    const uint32_t w23 = (k & 1u) ? h3 : h2;
    const uint32_t w = k >= 4u ? h4 : ((k & 2u) ? w23 : w01);
    return (w >> (8u * (i & 3u))) & 0xFFu;
  };
  uint64_t cnt = 0, glo = 0, ghi = 0;
  uint32_t seen = 0, i = 3;
  bool regular = true, bad = bad_hdr;
  auto group = [&](uint32_t info) {  // the group whose info byte is at i
    const uint32_t L = (info >> 5) + 1, n = (info & 31) + 1;
    const uint32_t nbytes = (n * 11 + 7) / 8;
    bad = bad || i + 1 + nbytes > 3 + tb;
    cnt += (uint64_t)n << (8 * (L - 1));
    regular = regular && !(seen & (1u << L));
    seen |= 1u << L;
    const uint64_t gb = (uint64_t)(8 * (i + 1)) << (16 * ((L - 1) & 3));
    glo |= L <= 4 ? gb : 0ull;
    ghi |= L <= 4 ? 0ull : gb;
    i += 1 + nbytes;
  };
  if (3 + tb <= 20) {
    while (i - 3 < tb && !bad) group(reg_byte(i));
  } else {
    while (i - 3 < tb && !bad) group(c.byte(i));
  }
  // at most 64 entries per code length (include/myyuv_hip.h, "Table limits";
  // the total is limited by tb alone: 255 table bytes hold fewer than 186
  // entries, so no byte of cnt carries into the next).  One test of the eight
  // counts after the walk: a byte above 64 has bit 7 set once 63 is added.
  bad = bad || ((cnt + 0x3F3F3F3F3F3F3F3Full) & 0x8080808080808080ull) != 0;
  uint32_t F = 0;
#pragma unroll
  for (int L = 0; L < 8; L++) {  // length L + 1
    const uint32_t cL = (uint32_t)(cnt >> (8 * L)) & 0xFF;
    if (F + cL > (2u << L)) regular = false;
    const uint32_t lim = ((F + cL) << (7 - L)) & 0xFFFF;
    const uint32_t gb = (uint32_t)((L < 4 ? glo : ghi) >> (16 * (L & 3))) & 0xFFFF;
    T.lim[L >> 1] |= lim << (16 * (L & 1));
    gcol[64 * L] = 8 * c.b0 + gb - 11 * F;  // (mod 2^32: the first value's stage bit is 8 b0 + gb)
    F = (F + cL) << 1;
  }
  uint32_t nb = nbits;
#if MYYUV_K5_FORMS
  asm volatile("" : "+v"(nb));  // (materialised: no WORD_0 selects on h0 in the symbol loop)
#endif
  T.nbits = nb;
  T.sbit = 8 * (3 + tb);
  T.tb = tb;
  T.cnt = cnt;
  T.regular = regular;
  return bad ? 12 : 0;
}

// Symbols of REGULAR tables (Huffman.cpp:106-154) into nw (natural-order
// int16 pairs, zeroed by the caller).  Returns true for an `act` lane whose
// message fails (no code matches, or a code runs past nbits): the caller
// re-decodes that block with decode_general, which gives the reference's
// exact outcome (10 bad code / 11 unknown symbol) — regular tables decode
// identically on both paths, so only the error code is taken from it.
//
// Fully unrolled over the 64 scan positions (each value lands in a statically
// indexed register), with a uniform "any lane left" exit before every
// position; the body is straight-line (state updates by select: divergent
// branches make the compiler shuffle the whole nw[] array at every join).
// A lane's state after it stops (bp, window) is dead, so it advances
// unconditionally; only the value store is predicated.  The 64-bit window is
// rebuilt every 7 positions (at most 56 bits consumed) from three stage
// words.  Per position: the length by SWAR compares, the value's 11 bits read
// in place from the table (group bit + 11 * rank), one predicated OR.
// (Prefetching the stage words a few positions ahead, or deferring each value
// read by one position, measured no faster on MI355X, and with the loads
// three positions ahead the decoded values came out wrong nondeterministically
// in long straight-line groups: both are deliberately not done.)
// (ZeroBit: the stage bit of the wave's zero quad; the span decoder's stage
// is shorter)
template <uint32_t ZeroBit = kZeroBit>
__device__ __forceinline__ bool decode_regular(const LdsChunk& c, const Table& T, const uint32_t* gcol, bool act,
                                               uint32_t (&nw)[32]) {
  bool bad = false;
  uint32_t bp = 0;
  uint64_t rwin = 0;  // MSB-first window: the next symbol's first bit at bit 63
  act = act && T.nbits > 0;
  const uint32_t P0 = 8 * c.b0 + T.sbit;  // stage bit of the first symbol bit
#pragma unroll
  for (int j0 = 0; j0 < 64; j0 += MYYUV_K5_GROUP) {
    if (__ballot(act) == 0) continue;
#pragma unroll
  for (int j = j0; j < j0 + MYYUV_K5_GROUP; j++) {
    if (j % 7 == 0) {
      const uint32_t P = act ? P0 + bp : P0, w = P >> 5;
      const uint32_t q0 = c.st[w], q1 = c.st[w + 1], q2 = c.st[w + 2];
      rwin = ((uint64_t)__brev(funnel(q1, q0, P)) << 32) | __brev(funnel(q2, q1, P));
    }
    const uint32_t w8 = (uint32_t)(rwin >> 56);  // next 8 bits, MSB-first
    // matched length - 1 = #{L : w8 >= lim[L]} (eight 16-bit fields)
    const uint32_t W = w8 * 0x10001u | 0x80008000u;
    const uint32_t n = __popc((W - T.lim[0]) & 0x80008000u) + __popc((W - T.lim[1]) & 0x80008000u) +
                       __popc((W - T.lim[2]) & 0x80008000u) + __popc((W - T.lim[3]) & 0x80008000u);
    const uint32_t bpn = bp + n + 1;
    const bool ok = n < 8 && bpn <= T.nbits;
    bad = bad || (act && !ok);
    const bool take = act && ok;
    // the value: the code's n + 1 bits times 11 plus length n + 1's entry of
    // the lane's column of the LDS table, the stage bit of its length's first
    // value less 11 times its first code (n = 8, no match: not taken)
    const uint32_t G = gcol[64 * (n & 7u)];
#if MYYUV_K5_FORMS
    uint32_t vbit;  // (code < 2^8: v_mad_u32_u24; the compiler turns a 32-bit product + G into v_mad_u64_u32)
    asm("v_mad_u32_u24 %0, %1, 11, %2" : "=v"(vbit) : "v"((uint32_t)(rwin >> 32) >> ((31u - n) & 31u)), "v"(G));
#else
    const uint32_t vbit = ((uint32_t)(rwin >> 32) >> ((31u - n) & 31u)) * 11u + G;
#endif
    const uint32_t P = take ? vbit : ZeroBit, w = P >> 5;  // (stage bits; ZeroBit: the zero quad)
    const uint32_t raw = funnel(c.st[w + 1], c.st[w], P);
    const uint32_t v = (uint32_t)(((int32_t)(raw << 21)) >> 21);
    const int z = c_zz[j];
    if (z & 1) nw[z >> 1] |= v << 16;
    else nw[z >> 1] |= v & 0xFFFFu;
    rwin <<= (n + 1) & 63;
    bp = bpn;
    act = take && bpn < T.nbits;
  }
  }
  return bad;
}

// Symbols of any table, bit-serial conditions as the reference evaluates them
// (uint8 arithmetic of `first` kept), values found by walking the groups of
// the matched length in stream order; every coefficient is handed to put(z, v)
// (int16 v at natural index z), zeros after the last symbol: decode_general
// stores them straight into the quad layout (slot `g`), the region decoder
// into LDS.  Only lanes whose table is not regular (malformed or hand-made
// streams) come here, after the wave's regular lanes, with the unrolled state
// dead.
template <class Put>
__device__ __forceinline__ int decode_general_to(const LdsChunk c, const Table T, Put put) {
  int code = 0;
  uint32_t bp = 0, j = 0;
  while (bp < T.nbits && j < 64) {
    const uint32_t P = T.sbit + bp;
    const uint32_t x = c.byte(P >> 3) | (c.byte((P >> 3) + 1) << 8);
    const uint32_t w8 = __brev((x >> (P & 7)) & 0xFF) >> 24;  // next 8 bits, MSB-first
    uint32_t first = 0, mL = 0, r = 0;
    bool neg = false;
#pragma unroll
    for (uint32_t L = 1; L <= 8; L++) {
      const uint32_t cL = (uint32_t)(T.cnt >> (8 * (L - 1))) & 0xFF;
      const uint32_t cd = w8 >> (8 - L);
      if (mL == 0 && cd < cL + first) {
        mL = L;
        neg = cd < first;
        r = cd - first;
      }
      first = ((first + cL) << 1) & 0xFF;
    }
    if (mL == 0) {
      code = (bp + 8 > T.nbits) ? 10 : 11;
      break;
    }
    if (bp + mL > T.nbits || neg) {
      code = 10;
      break;
    }
    uint32_t i = 3, vbit = 0;
    while (i - 3 < T.tb) {
      const uint32_t info = c.byte(i);
      const uint32_t n = (info & 31) + 1;
      if ((info >> 5) + 1 == mL) {
        if (r < n) {
          vbit = 8 * (i + 1) + 11 * r;
          break;
        }
        r -= n;
      }
      i += 1 + (n * 11 + 7) / 8;
    }
    const uint32_t z = c_zz_dev[j];
    put(z, (uint16_t)(((int32_t)(c.bits32(vbit) << 21)) >> 21));
    bp += mL;
    j++;
  }
  for (; j < 64; j++) {
    const uint32_t z = c_zz_dev[j];
    put(z, (uint16_t)0);
  }
  return code;
}

__device__ __forceinline__ int decode_general(const LdsChunk c, const Table T, uint4* coef,
                                           uint32_t g) {
  uint16_t* out = reinterpret_cast<uint16_t*>(coef);
  return decode_general_to(c, T, [=](uint32_t z, uint16_t v) { out[coef_quad(g, z >> 3) * 8 + (z & 7)] = v; });
}

}  // namespace

#ifdef MYYUV_STAMPS
// diagnostic build only (-DMYYUV_STAMPS): the fused decoder's wave cycles
// per phase, per wave (plain stores at the wave's end; contended atomics
// would distort the timing): g_dec_wstamps[wave][8] = [0] setup (sizes,
// scan, offsets), [1] staging, [2] table parse, [3] symbol loop, [5] the DC
// blocks and the transform, [6] rounds, [7] = 1 for a wave that ran
// (myyuv_debug_dec_stamps, tools/dec_phase.py)
__device__ uint32_t g_dec_wstamps[65536 * 8];
struct DStamps {
  unsigned long long prev;
  uint32_t acc[8];
};
#define DSTAMP(k)                                                \
  do {                                                           \
    if (ds != nullptr) {                                         \
      __builtin_amdgcn_sched_barrier(0);                         \
      const unsigned long long _t = __builtin_amdgcn_s_memtime(); \
      __builtin_amdgcn_sched_barrier(0);                         \
      ds->acc[k] += (uint32_t)(_t - ds->prev);                   \
      ds->prev = _t;                                             \
    }                                                            \
  } while (0)
#else
struct DStamps {};
#define DSTAMP(k) \
  do {            \
  } while (0)
#endif

// K5's decode of one wave's 64-block group (blockIdx.x) of frame blockIdx.y:
// the natural-order words of each lane's block in nw (or, for a table that is
// not "regular", written to coef by decode_general: *direct).  Returns false
// when the frame's stream header is bad (nothing decoded).
struct DecodeGroup {
  uint32_t f, gbase, g0, g1, g;
  int p;
  bool live;
  bool good;  // live, and the lane's chunk decoded without an error
};
__device__ __forceinline__ bool decode_group(const uint8_t* __restrict__ in, const uint32_t* __restrict__ in_size,
                                             uint32_t cap, const StreamDesc* __restrict__ desc,
                                             const uint32_t* __restrict__ local_off,
                                             const uint32_t* __restrict__ tile_pre, const FrameGeom& G,
                                             uint32_t tiles_p0, uint32_t tiles_p1, uint4* __restrict__ coef,
                                             unsigned long long* __restrict__ err, uint4* stq, DecodeGroup& D,
                                             uint32_t (&nw)[32], bool& direct, DStamps* ds = nullptr) {
  // frame blockIdx.y of the batch: its stream slot, descriptor and scan;
  // coefficients at batch-global block gbase + g
  const uint32_t f = blockIdx.y;
  const uint32_t nblk = G.cum[3];
  const uint32_t gbase = f * nblk;
  const uint32_t ntiles = (nblk + kScanTile - 1) / kScanTile;
  in += (size_t)f * cap;
  desc += f;
  local_off += gbase;
  tile_pre += (size_t)f * (ntiles + 1);
  const int lane = threadIdx.x;
  // the lanes' per-length value positions (stage bit of the length's first
  // value - 11 * its first code; length-major: lane l's length L at
  // [64 L + l]), after the stage and its zero quad
  uint32_t* gcol = reinterpret_cast<uint32_t*>(stq + kStageQuads + 1) + lane;
  const uint32_t t = blockIdx.x;
  const int p = t >= tiles_p0 ? (t >= tiles_p0 + tiles_p1 ? 2 : 1) : 0;
  // the plane's fields by static index (a dynamic index into the kernel
  // argument G, or into the descriptor once loaded, is a scalar load: one
  // more dependent round trip)
  auto sel3 = [p](uint32_t a0, uint32_t a1, uint32_t a2) { return p == 0 ? a0 : (p == 1 ? a1 : a2); };
  const uint32_t cum_p = sel3(G.cum[0], G.cum[1], G.cum[2]), cum_p1 = sel3(G.cum[1], G.cum[2], G.cum[3]);
  const uint32_t tile_in_plane = t - sel3(0u, tiles_p0, tiles_p0 + tiles_p1);
  const uint32_t g0 = cum_p + tile_in_plane * kWave;
  const uint32_t g1 = min(g0 + kWave, cum_p1);
  const uint32_t g = g0 + lane;
  const bool live = g < g1;
  // every scalar of the setup in one round trip: the descriptor, the payload
  // size, the scan at the plane's start and the group's ends.  No branch on
  // `bad` in front of them (it would hold the rest back by a round trip): a
  // bad frame decodes nothing (no lane is ok) and returns false below.
  const StreamDesc dsc = *desc;
  const uint32_t isz = in_size[f];
  const uint32_t g1c = min(g1, nblk - 1);
  const uint32_t lo_p = local_off[cum_p], tp_p = tile_pre[cum_p / kScanTile];
  const uint32_t lo_0 = local_off[g0], tp_0 = tile_pre[g0 / kScanTile];
  const uint32_t lo_1 = local_off[g1c], tp_1 = tile_pre[g1c / kScanTile];
  const uint32_t stot = tile_pre[ntiles];  // rel(nblk) = the total
  __builtin_amdgcn_sched_barrier(0);  // (all issued before the first use waits)
  const uint32_t plane_pre = lo_p + tp_p, s0 = lo_0 + tp_0, s1 = lo_1 + tp_1;
  const bool bad = dsc.bad != 0;
  const uint32_t limit = bad ? 0u : min(isz, cap);
  // end of the wave's chunk range from the scan alone
  const uint32_t end_scan = g1 == nblk ? stot : s1;
  const uint32_t cpos = sel3(dsc.content_pos[0], dsc.content_pos[1], dsc.content_pos[2]);
  const uint32_t csize = sel3(dsc.content_size[0], dsc.content_size[1], dsc.content_size[2]);
  const uint32_t spos = sel3(dsc.sizes_pos[0], dsc.sizes_pos[1], dsc.sizes_pos[2]);
  const uint32_t E = cpos + min(end_scan - plane_pre, csize);
  // Round 1 stages from the group's first chunk (lane 0's: g0 < g1, so lane
  // 0 is live; when it is not ok, no lane is and no round runs).  Its
  // position needs no size byte, so its loads go out together with the size
  // bytes' (issued just before them: the VMEM counter drains in order, so
  // the size bytes' wait covers them either way) instead of after the size
  // scan: one dependent load round trip less before the table parse.
  const uint32_t pre0 = s0 - plane_pre;
  auto window = [&](uint32_t A, uint32_t& aw, uint32_t& wend, uint32_t& nq, uint32_t& nfull) {
    aw = A & ~15u;
    wend = aw + 16 * (kStageQuads - 1);
    nq = E > aw ? (min(E, wend) - aw + 15) >> 4 : 0u;
    nfull = limit >= aw ? min(nq, (limit - aw) >> 4) : 0u;  // quads below limit
  };
  // the first 256 quads straight into the stage (LDS-DMA: quad 64m + lane
  // from instruction m), all in flight together and holding no registers.
  // Unconditional, at clamped addresses: the quads they write at or past
  // nfull are rewritten by stage() up to nq, and past nq nothing reads the
  // stage
  auto load4 = [&](uint32_t aw, uint32_t nfull) {
#pragma unroll
    for (int m = 0; m < 4; m++) {
      const uint8_t* src = nfull > 0 ? in + aw + 16 * min(lane + 64u * m, nfull - 1) : in;
      __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)(stq + 64 * m),
                                       16, 0, 0);
    }
  };
  uint32_t aw, wend, nq, nfull;
  window(cpos + pre0, aw, wend, nq, nfull);
  load4(aw, nfull);
  __builtin_amdgcn_sched_barrier(0);  // (all four issued before the size bytes' load)
  const uint32_t gl = live ? g : g1 - 1;
  const uint32_t s = in[bad ? 0u : spos + (gl - cum_p)];
  // the chunk's offset: the group's (k_scan_chain keeps group starts only)
  // plus the wave's exclusive scan of the sizes
  // (by DPP, the whole wave active: six ds_bpermute round trips less)
  const uint32_t incl = wave_incl_scan(live ? s : 0u);
  const uint32_t rel = pre0 + incl - (live ? s : 0u);

  // plane-level check (DCT.cpp:21-33 reads past content_size otherwise):
  // the chunks must fit the declared content.
  bool ok = live && !bad;
  if (ok && rel + s > csize) {
    record_error(err, 2ull * ((uint64_t)G.fbase * nblk + gbase + cum_p), 9 /* MYYUV_E_PLANE_CONTENT */);
    ok = false;
  }

  int code = 0;
  direct = false;  // block written by decode_general

  // Rounds: stage the chunks of the first pending lane onwards (as many as
  // the stage holds, bytes at or past `limit` read as 0, one zero quad after),
  // decode the lanes whose chunks are inside.  Chunks are consecutive and at
  // most 255 B, so every round retires at least one lane; a 4K frame at q=50
  // needs one round per wave.
  uint64_t pending = __ballot(ok);
  DSTAMP(0);
  // the rest of one round's stage: the window past 256 quads, zeros at or
  // past `limit` and the slack quad
  auto stage = [&]() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // load4's LDS writes (before the zero quads)
    for (uint32_t k = lane + 256; k < nfull; k += 64)
      stq[k] = *reinterpret_cast<const uint4*>(in + aw + 16 * k);
    for (uint32_t k = nfull + lane; k <= nq; k += 64) {
      uint32_t v[4] = {0, 0, 0, 0};
      if (k < nq) {
#pragma unroll
        for (uint32_t b = 0; b < 16; b++) {
          const uint32_t a = aw + 16 * k + b;
          if (a < limit) v[b >> 2] |= (uint32_t)in[a] << (8 * (b & 3));
        }
      }
      stq[k] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
  };
  if (pending) stage();
  while (pending) {
#ifdef MYYUV_STAMPS
    if (ds != nullptr) ds->acc[6] += 1;
#endif
    DSTAMP(1);

    const bool mine = ((pending >> lane) & 1) && cpos + rel + s <= wend;
    const LdsChunk lc{reinterpret_cast<const uint32_t*>(stq), mine ? cpos + rel - aw : 0u};
    Table T;
    // (every lane parses, the others as a bad header of size 0 at the stage's
    // start: no branch level around the parse, whose outputs the compiler
    // would re-initialise on the skipped path)
    const int pcode = parse_table(lc, mine ? s : 0u, T, gcol);
    const bool go = mine && pcode == 0;
    int dcode = 0;
    DSTAMP(2);
    const bool failed = decode_regular(lc, T, gcol, go && T.regular, nw);
    // tables the reference never writes, and failed messages (for the
    // reference's exact error code): the bit-serial path
    if (go && (!T.regular || failed)) {
      direct = true;
      dcode = decode_general(lc, T, coef, gbase + g);
    }
    if (mine) code = go ? dcode : pcode;
    pending &= ~__ballot(mine);
    DSTAMP(3);
    if (pending) {  // the next round, from the lowest pending lane's chunk
      __syncthreads();  // it overwrites the stage
      const int lo = __ffsll((long long)pending) - 1;
      window(cpos + __shfl(rel, lo, 64), aw, wend, nq, nfull);
      load4(aw, nfull);
      stage();
    }
  }
  // every LDS-DMA load has landed before the stage is reused or the wave
  // ends, whether or not a round ran (no lane ok: round 1's loads were still
  // issued)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (ok && code) record_error(err, 2ull * ((uint64_t)G.fbase * nblk + gbase + g) + 1, code);
  D.f = f;
  D.gbase = gbase;
  D.g0 = g0;
  D.g1 = g1;
  D.g = g;
  D.p = p;
  D.live = live;
  D.good = ok && code == 0;
  return !bad;
}

__global__ __launch_bounds__(64, MYYUV_K5S_WAVES) void k_huff_decode(const uint8_t* __restrict__ in,
                                                   const uint32_t* __restrict__ in_size,
                                                   uint32_t cap,
                                                   const StreamDesc* __restrict__ desc,
                                                   const uint32_t* __restrict__ local_off,
                                                   const uint32_t* __restrict__ tile_pre,
                                                   FrameGeom G, uint32_t tiles_p0,
                                                   uint32_t tiles_p1,
                                                   uint4* __restrict__ coef,
                                                   uint8_t* __restrict__ rmask,
                                                   unsigned long long* __restrict__ err) {
  __shared__ uint4 stq[kStageQuads + 1 + kGposQuads];
  if (threadIdx.x == 0) stq[kStageQuads] = make_uint4(0u, 0u, 0u, 0u);  // (ordered by decode_group's barrier)
  DecodeGroup D;
  uint32_t nw[32];
#pragma unroll
  for (int w = 0; w < 32; w++) nw[w] = 0;
  bool direct;
  if (!decode_group(in, in_size, cap, desc, local_off, tile_pre, G, tiles_p0, tiles_p1, coef, err, stq, D, nw,
                    direct))
    return;  // the frame's stream header is bad (k_scan_chain recorded it)
  const uint32_t gbase = D.gbase, g = D.g;
  const bool live = D.live;
  // ---- natural-order words to the quad layout (1 KiB contiguous per store)
  // Only the nonzero rows are stored; bit c of the block's row mask says
  // whether row c holds a nonzero coefficient, and K6 reads just those.
  // decode_general wrote all 64 coefficients itself: mask 0xFF.
  if (live) {
    uint32_t m = 0xFFu;
    if (!direct) {
      m = 0;
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const bool nz = (nw[4 * c] | nw[4 * c + 1] | nw[4 * c + 2] | nw[4 * c + 3]) != 0u;
        m |= nz ? 1u << c : 0u;
        if (nz) coef[coef_quad(gbase + g, c)] = make_uint4(nw[4 * c], nw[4 * c + 1], nw[4 * c + 2], nw[4 * c + 3]);
      }
    }
    rmask[gbase + g] = (uint8_t)m;
  }
}

// The pixel of a block whose only nonzero coefficient may be the DC, four
// times in a word (k_decode_idct's comment on such blocks derives it): with
// Z[0][0] = z, R = fl(fl(c * z) * c) for all 64 pixels, c the one value of the
// literal basis' row 0 — the full transform's two roundings, then its clamp
// and rounding to a pixel.  q0 = Q[0][0] of the plane.
__device__ __forceinline__ uint32_t dc_block_pixels(int16_t dc, float q0) {
  constexpr float c0 = xf::c_dct[0];
  static_assert(xf::c_dct[0] == xf::c_dct[1] && xf::c_dct[0] == xf::c_dct[7], "row 0 of the basis is one value");
  const float z = (float)dc * q0;   // dequantise (DCT.cpp:331)
  const float u = 0.0f + c0 * z;    // stage 1: the k = 0 term
  float S = 0.0f + u * c0;          // stage 2: the k = 0 term
  S = __builtin_amdgcn_fmed3f(S, -128.0f, 127.0f);  // (as idct_rows, DCT.cpp:358-362)
  uint32_t px = xf::bits(S + xf::kMagicPx);
  if (__builtin_amdgcn_fractf(S) == 0.5f)
    px = (uint32_t)((int)__builtin_truncf(S + __builtin_copysignf(xf::kHalfDown, S)) + 128);
  return (px & 0xFFu) * 0x01010101u;
}

// Fused decoder (K5 + K6; MYYUV_DECODER=fused): the wave decodes its 64-block
// group as K5 does, then runs K6's transform on it in 8-block units straight
// from its registers: the unit's 8 decoding lanes write their blocks' int16
// images into the wave's transpose tile (laid over the chunk stage, dead by
// then), and the wave's lanes take (block, row) roles (idct_row8,
// xform_common.hpp).  The coefficients never reach HBM.
__global__ __launch_bounds__(64, MYYUV_K5_WAVES) void k_decode_idct(const uint8_t* __restrict__ in,
                                                   const uint32_t* __restrict__ in_size,
                                                   uint32_t cap,
                                                   const StreamDesc* __restrict__ desc,
                                                   const uint32_t* __restrict__ local_off,
                                                   const uint32_t* __restrict__ tile_pre,
                                                   FrameGeom G, uint32_t tiles_p0,
                                                   uint32_t tiles_p1, const QTables* __restrict__ qt,
                                                   uint4* __restrict__ coef,
                                                   uint8_t* __restrict__ frame,
                                                   unsigned long long* __restrict__ err) {
  static_assert(sizeof(uint4) * kStageQuads >= sizeof(float) * xf::kXfTile16, "the tile over the stage");
  __shared__ uint4 stq[kStageQuads + 1 + kGposQuads];
  __shared__ float sq[64];
  __shared__ uint16_t s_blk[64];
  const uint32_t lane = threadIdx.x;
  if (lane == 0) stq[kStageQuads] = make_uint4(0u, 0u, 0u, 0u);  // (ordered by decode_group's barrier)
  {
    // the plane's Q table by LDS-DMA (no register, no wait here; landed by
    // decode_group's final vmcnt wait, before idct_rows)
    const uint32_t t = blockIdx.x;
    const int p = t >= tiles_p0 ? (t >= tiles_p0 + tiles_p1 ? 2 : 1) : 0;
    __builtin_amdgcn_global_load_lds((const void*)&qt->q[p][lane], (__attribute__((address_space(3))) void*)sq, 4,
                                     0, 0);
  }
#ifdef MYYUV_STAMPS
  DStamps dst;
  DStamps* ds = &dst;
  dst.prev = __builtin_amdgcn_s_memtime();
#pragma unroll
  for (int k = 0; k < 8; k++) dst.acc[k] = k == 7 ? 1u : 0u;
#else
  DStamps* ds = nullptr;
#endif
  DecodeGroup D;
  uint32_t nw[32];
#pragma unroll
  for (int w = 0; w < 32; w++) nw[w] = 0;
  bool direct;
  if (!decode_group(in, in_size, cap, desc, local_off, tile_pre, G, tiles_p0, tiles_p1, coef, err, stq, D, nw,
                    direct, ds))
    return;  // the frame's stream header is bad (k_scan_chain recorded it)
  DSTAMP(4);
  if (D.live && direct) {  // decode_general wrote the block to coef (a table the reference never writes)
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const uint4 v = coef[coef_quad(D.gbase + D.g, c)];
      nw[4 * c] = v.x;
      nw[4 * c + 1] = v.y;
      nw[4 * c + 2] = v.z;
      nw[4 * c + 3] = v.w;
    }
  }
  // ---- K6 on the group.  Blocks whose only nonzero coefficient is the DC
  // (53 % of the bench frame's blocks) decode to one constant pixel value:
  // with Z[0][0] = z the only nonzero coefficient, stage 1 leaves U[i][0] =
  // fl(D[0][i] * z), stage 2 R[i][v] = fl(U[i][0] * D[0][v]) (the other
  // products are +-0 and every sum starts at +0), and row 0 of the literal
  // basis is one value c, so R = fl(fl(c * z) * c) for all 64 pixels — the
  // same two roundings as the full transform, which the lane evaluates for its
  // own block and stores as 8 rows.  The other blocks are compacted into
  // 8-block units for the transform (up to eight; their rows are written
  // wherever the blocks lie).
  const int p = D.p;
  xf::Unit U;
  U.p = p;
  U.cum = G.cum[p];
  U.nb = G.cum[p + 1] - G.cum[p];
  U.poff = p == 0 ? G.poff[0] : (p == 1 ? G.poff[1] : G.poff[2]);
  U.pw = p == 0 ? G.pw[0] : (p == 1 ? G.pw[1] : G.pw[2]);
  U.bw = p == 0 ? G.bw[0] : (p == 1 ? G.bw[1] : G.bw[2]);
  U.bmag = p == 0 ? G.bmag[0] : (p == 1 ? G.bmag[1] : G.bmag[2]);
  U.local0 = 0;
  uint8_t* fr = frame + (size_t)D.f * G.fbytes;
  uint32_t acc = nw[0] & 0xFFFF0000u;
#pragma unroll
  for (int w = 1; w < 32; w++) acc |= nw[w];
  const bool isdc = D.live && acc == 0u;
  if (isdc) {
    const uint32_t v4 = dc_block_pixels((int16_t)nw[0], sq[0]);
    const uint2 row = make_uint2(v4, v4);
#pragma unroll
    for (uint32_t r = 0; r < 8; r++) {
      const uint32_t off = xf::block_row_offset(U, D.g - U.cum, r);
      *reinterpret_cast<uint2*>(fr + off) = row;
    }
  }
  // (compacted in block order: ordering the units by sparsity kind — row 0
  // only, column 0 only, the rest — measured no faster, profiles/r3zl_*)
  const uint64_t rest = __ballot(D.live && !isdc);
  const uint32_t nrest = (uint32_t)__popcll(rest);
  const uint32_t rrank = __builtin_amdgcn_mbcnt_hi((uint32_t)(rest >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rest, 0u));
  if (D.live && !isdc) s_blk[rrank] = (uint16_t)lane;  // compacted position -> the block's lane in the group
  float* tile = reinterpret_cast<float*>(stq);
  // 16-block units while more than 8 blocks are left (lane (b, q): rows 2q,
  // 2q+1 of block b, idct_rows), the last 1-8 blocks as one 8-block unit
  // (lane (b, r): row r, idct_row8, half the products per step).  Slots past
  // the last block are zero, so they do not keep steps alive; slot `lane` is
  // zeroed by lane `lane` whether or not that lane also writes a compacted
  // block: the two slots differ (rrank < nrest <= base + lane).
#pragma unroll 1
  for (uint32_t base = 0; base < nrest;) {
    const bool wide = nrest - base > 8u;
    const uint32_t span = wide ? 16u : 8u, stride = wide ? (uint32_t)xf::kTile : (uint32_t)xf::kTile8;
    const uint32_t s = rrank - base;
    if (D.live && !isdc && rrank >= base && s < span) {
      uint4* img = reinterpret_cast<uint4*>(tile + s * stride + (wide ? xf::img_word(s) : 0u));
#pragma unroll
      for (int c = 0; c < 8; c++) img[c] = make_uint4(nw[4 * c], nw[4 * c + 1], nw[4 * c + 2], nw[4 * c + 3]);
    }
    if (lane < span && base + lane >= nrest) {
      uint4* img = reinterpret_cast<uint4*>(tile + lane * stride + (wide ? xf::img_word(lane) : 0u));
#pragma unroll
      for (int c = 0; c < 8; c++) img[c] = make_uint4(0u, 0u, 0u, 0u);
    }
    xf::wave_sync();
    if (wide) {
      const uint32_t q = lane & 3u, b = lane >> 2;
      uint2 w0, w1;
      xf::idct_rows(tile + b * xf::kTile, q, b, sq, w0, w1);
      if (base + b < nrest) {
        const uint32_t gl = D.g0 + s_blk[base + b];  // the block of compacted position base + b
        const uint32_t off = xf::block_row_offset(U, gl - U.cum, 2u * q);
        *reinterpret_cast<uint2*>(fr + off) = w0;
        *reinterpret_cast<uint2*>(fr + off + U.pw) = w1;
      }
    } else {
      const uint32_t r = lane & 7u, b = lane >> 3;
      float qc[8];  // the lane's column of the plane's Q table, Q[k][r]
#pragma unroll
      for (int k = 0; k < 8; k++) qc[k] = sq[8 * k + r];
      const uint2 w = xf::idct_row8(tile + b * xf::kTile8, r, qc);
      if (base + b < nrest) {
        const uint32_t gl = D.g0 + s_blk[base + b];
        *reinterpret_cast<uint2*>(fr + xf::block_row_offset(U, gl - U.cum, r)) = w;
      }
    }
    xf::wave_sync();  // the next unit rewrites the tile
    base += span;
  }
  DSTAMP(5);
#ifdef MYYUV_STAMPS
  const uint32_t wid = blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
  for (int k = 0; k < 8; k++)
    if (lane == (uint32_t)k && wid < 65536) g_dec_wstamps[wid * 8 + k] = dst.acc[k];
#endif
}

// ---- span decoder -----------------------------------------------------------
//
// k_decode_span: the fused decoder with a wave owning a SPAN of kDecSpan
// consecutive blocks of one plane (2, 4 or 8 of k_decode_idct's groups; grid
// (spans of the three planes, frames); a plane's last span and its last
// group are partial).  53 % of the bench frame's blocks are one-symbol blocks
// whose 7-byte chunk is a closed form of the DC's low 11 bits
// (single_chunk_words, codec_common.hpp), and in k_decode_idct they occupy
// lanes of the table parse and the symbol loop like any other.  Here:
//   span phase: lane l takes block 64 j + l of every group j; the size bytes
//     of all groups are loaded together and scanned per group (the chunk's
//     offset: the group's start from k_scan_chain plus the scan), then the
//     first 7 bytes of every 7-byte chunk, and the blocks whose chunk IS the
//     closed form (single_chunk_key) are finished at once: dc_block_pixels and
//     the 8 row stores.  Every other live block whose chunk lies inside the
//     plane's content is a "real" block: ballots and ranks compact them, in
//     block order, into a list in LDS (index in the span, offset from the
//     span's first chunk, size);
//   passes: ceil(real / 64), none for a span of closed forms.  Lane l takes
//     list entry 64 p + l; the pass stages the bytes from its first entry's
//     chunk to its last entry's end (consecutive passes: consecutive,
//     disjoint ranges; the closed-form chunks lying between are staged along)
//     in k_decode_idct's rounds, parses, decodes and transforms as it does,
//     the blocks' places taken from the list.
// The stage is the 16-block transform tile's 4,608 B (a round still holds 17
// longest chunks); with the list the wave's LDS stays at 8 KiB, 5 waves per
// SIMD.  Error keys, codes and their order are k_decode_idct's (atomicMin:
// the order of passes does not matter).
constexpr uint32_t kSpanStageQuads = 288;
constexpr uint32_t kSpanZeroBit = kSpanStageQuads * 128u;
constexpr uint32_t kSpanGroups = kDecSpan / kWave;
static_assert(sizeof(uint4) * kSpanStageQuads >= sizeof(float) * xf::kXfTile16, "the tile over the stage");
static_assert(16 * (kSpanStageQuads - 1) >= 15 + 255, "a round holds its first chunk wherever it starts in its quad");
// A list entry.  The offset from the span's first chunk is at most
// (kDecSpan - 1) * 255: 16 bits up to 256 blocks.
#if MYYUV_DEC_SPAN <= 256
typedef uint32_t SpanEnt;
__device__ __forceinline__ SpanEnt span_ent(uint32_t idx, uint32_t off, uint32_t s) {
  return (off & 0xFFFFu) | (s << 16) | (idx << 24);
}
__device__ __forceinline__ uint32_t ent_off(SpanEnt e) { return e & 0xFFFFu; }
__device__ __forceinline__ uint32_t ent_size(SpanEnt e) { return (e >> 16) & 0xFFu; }
__device__ __forceinline__ uint32_t ent_idx(SpanEnt e) { return e >> 24; }
#else
typedef uint2 SpanEnt;
__device__ __forceinline__ SpanEnt span_ent(uint32_t idx, uint32_t off, uint32_t s) {
  return make_uint2(off, s | (idx << 8));
}
__device__ __forceinline__ uint32_t ent_off(SpanEnt e) { return e.x; }
__device__ __forceinline__ uint32_t ent_size(SpanEnt e) { return e.y & 0xFFu; }
__device__ __forceinline__ uint32_t ent_idx(SpanEnt e) { return e.y >> 8; }
#endif

__global__ __launch_bounds__(64, MYYUV_K5_WAVES) void k_decode_span(const uint8_t* __restrict__ in,
                                                   const uint32_t* __restrict__ in_size,
                                                   uint32_t cap,
                                                   const StreamDesc* __restrict__ desc,
                                                   const uint32_t* __restrict__ local_off,
                                                   const uint32_t* __restrict__ tile_pre,
                                                   FrameGeom G, uint32_t spans_p0,
                                                   uint32_t spans_p1, const QTables* __restrict__ qt,
                                                   uint4* __restrict__ coef,
                                                   uint8_t* __restrict__ frame,
                                                   unsigned long long* __restrict__ err) {
  __shared__ uint4 stq[kSpanStageQuads + 1 + kGposQuads];
  __shared__ float sq[64];
  __shared__ uint16_t s_blk[64];
  __shared__ SpanEnt s_ent[kDecSpan];
  const uint32_t lane = threadIdx.x;
  // (the zero quad lies past the tile and the Q table is its own array: no
  // pass overwrites either)
  if (lane == 0) stq[kSpanStageQuads] = make_uint4(0u, 0u, 0u, 0u);  // (ordered by stage()'s barrier)
  const uint32_t t = blockIdx.x;
  const int p = t >= spans_p0 ? (t >= spans_p0 + spans_p1 ? 2 : 1) : 0;
  // the plane's Q table by LDS-DMA (landed by the span phase's vmcnt wait)
  __builtin_amdgcn_global_load_lds((const void*)&qt->q[p][lane], (__attribute__((address_space(3))) void*)sq, 4, 0,
                                   0);
  const uint32_t f = blockIdx.y;
  const uint32_t nblk = G.cum[3];
  const uint32_t gbase = f * nblk;
  const uint32_t ntiles = (nblk + kScanTile - 1) / kScanTile;
  in += (size_t)f * cap;
  desc += f;
  local_off += gbase;
  tile_pre += (size_t)f * (ntiles + 1);
  auto sel3 = [p](uint32_t a0, uint32_t a1, uint32_t a2) { return p == 0 ? a0 : (p == 1 ? a1 : a2); };
  const uint32_t cum_p = sel3(G.cum[0], G.cum[1], G.cum[2]), cum_p1 = sel3(G.cum[1], G.cum[2], G.cum[3]);
  const uint32_t span_in_plane = t - sel3(0u, spans_p0, spans_p0 + spans_p1);
  const uint32_t b0 = cum_p + span_in_plane * kDecSpan;  // the span's blocks: [b0, b1) of the frame
  const uint32_t b1 = min(b0 + kDecSpan, cum_p1);
  // every scalar of the setup in one round trip: the descriptor, the payload
  // size, the scan at the plane's start, at the span's group starts (a group
  // past the span's end: the span's own start, unused) and at its end
  const StreamDesc dsc = *desc;
  const uint32_t isz = in_size[f];
  const uint32_t b1c = min(b1, nblk - 1);
  const uint32_t lo_p = local_off[cum_p], tp_p = tile_pre[cum_p / kScanTile];
  uint32_t lo_j[kSpanGroups], tp_j[kSpanGroups];
#pragma unroll
  for (uint32_t j = 0; j < kSpanGroups; j++) {
    const uint32_t gs = b0 + kWave * j < b1 ? b0 + kWave * j : b0;
    lo_j[j] = local_off[gs];
    tp_j[j] = tile_pre[gs / kScanTile];
  }
  const uint32_t lo_1 = local_off[b1c], tp_1 = tile_pre[b1c / kScanTile];
  const uint32_t stot = tile_pre[ntiles];  // rel(nblk) = the total
  __builtin_amdgcn_sched_barrier(0);  // (all issued before the first use waits)
  if (dsc.bad != 0) {  // the frame's stream header is bad (k_scan_chain recorded it): nothing is decoded
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the Q table's LDS-DMA load)
    return;
  }
  const uint32_t plane_pre = lo_p + tp_p;
  const uint32_t limit = min(isz, cap);
  const uint32_t end_scan = b1 == nblk ? stot : lo_1 + tp_1;
  const uint32_t cpos = sel3(dsc.content_pos[0], dsc.content_pos[1], dsc.content_pos[2]);
  const uint32_t csize = sel3(dsc.content_size[0], dsc.content_size[1], dsc.content_size[2]);
  const uint32_t spos = sel3(dsc.sizes_pos[0], dsc.sizes_pos[1], dsc.sizes_pos[2]);
  // the span's chunks end here (inside the declared content)
  const uint32_t E_span = cpos + min(end_scan - plane_pre, csize);
  const uint32_t pre0 = lo_j[0] + tp_j[0] - plane_pre;  // the span's first chunk in the plane's content

  xf::Unit U;
  U.p = p;
  U.cum = cum_p;
  U.nb = cum_p1 - cum_p;
  U.poff = sel3(G.poff[0], G.poff[1], G.poff[2]);
  U.pw = sel3(G.pw[0], G.pw[1], G.pw[2]);
  U.bw = sel3(G.bw[0], G.bw[1], G.bw[2]);
  U.bmag = p == 0 ? G.bmag[0] : (p == 1 ? G.bmag[1] : G.bmag[2]);
  U.local0 = 0;
  uint8_t* fr = frame + (size_t)f * G.fbytes;

  // ---- span phase: sizes, offsets, the closed forms, the real list
  uint32_t sz[kSpanGroups], rel[kSpanGroups];
  bool ok[kSpanGroups];
#pragma unroll
  for (uint32_t j = 0; j < kSpanGroups; j++) {  // (all size bytes' loads together)
    const uint32_t g = b0 + kWave * j + lane;
    sz[j] = in[spos + ((g < b1 ? g : b1 - 1) - cum_p)];
  }
  bool over = false;
#pragma unroll
  for (uint32_t j = 0; j < kSpanGroups; j++) {
    const bool live = b0 + kWave * j + lane < b1;
    const uint32_t s = live ? sz[j] : 0u;
    // (by DPP, the whole wave active: uniform control flow up to here)
    rel[j] = lo_j[j] + tp_j[j] - plane_pre + wave_incl_scan(s) - s;
    // plane-level check (DCT.cpp:21-33 reads past content_size otherwise):
    // the chunks must fit the declared content
    ok[j] = live && rel[j] + s <= csize;
    over = over || (live && !ok[j]);
  }
  if (over) record_error(err, 2ull * ((uint64_t)G.fbase * nblk + gbase + cum_p), 9 /* MYYUV_E_PLANE_CONTENT */);
  // the 7-byte chunks' bytes 0..3 and 3..6, all loads together (the other
  // lanes read the slot's first bytes: no branch around the loads)
  uint32_t hw[kSpanGroups], tw[kSpanGroups];
  bool cand[kSpanGroups];
#pragma unroll
  for (uint32_t j = 0; j < kSpanGroups; j++) {
    cand[j] = ok[j] && sz[j] == kSingleChunk && cpos + rel[j] + kSingleChunk <= limit;
    const uint8_t* a = in + (cand[j] ? cpos + rel[j] : 0u);
    __builtin_memcpy(&hw[j], a, 4);
    __builtin_memcpy(&tw[j], a + 3, 4);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (and the Q table)
  const float q0 = sq[0];
  uint32_t nreal = 0;
#pragma unroll
  for (uint32_t j = 0; j < kSpanGroups; j++) {
    uint32_t key;
    const bool single = single_chunk_key(hw[j], tw[j], key) && cand[j];
    if (single) {
      const uint32_t v4 = dc_block_pixels((int16_t)(((int32_t)(key << 21)) >> 21), q0);
      const uint2 row = make_uint2(v4, v4);
      const uint32_t local = b0 + kWave * j + lane - cum_p;
#pragma unroll
      for (uint32_t r = 0; r < 8; r++) *reinterpret_cast<uint2*>(fr + xf::block_row_offset(U, local, r)) = row;
    }
    const bool real = ok[j] && !single;
    const uint64_t m = __ballot(real);
    const uint32_t rank =
        nreal + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (real) s_ent[rank] = span_ent(kWave * j + lane, rel[j] - pre0, sz[j]);
    nreal += (uint32_t)__popcll(m);
  }
  xf::wave_sync();  // the list

  // ---- passes over the real list
  float* tile = reinterpret_cast<float*>(stq);
  const uint32_t npass = (nreal + kWave - 1) / kWave;
#pragma unroll 1
  for (uint32_t pass = 0; pass < npass; pass++) {
    // (the lane index made anew per pass, by mbcnt of an opaque mask with
    // every lane active: neither it nor what derives from it, the tile and
    // table addresses, is held in registers across the symbol loop)
    uint32_t ones = ~0u;
    asm volatile("" : "+s"(ones));
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(ones, __builtin_amdgcn_mbcnt_lo(ones, 0u));
    uint32_t* gcol = reinterpret_cast<uint32_t*>(stq + kSpanStageQuads + 1) + lane;
    const uint32_t e0 = kWave * pass, nhere = min(nreal - e0, (uint32_t)kWave);
    const bool have = lane < nhere;
    const SpanEnt ent = s_ent[e0 + (have ? lane : nhere - 1u)];
    const uint32_t s = have ? ent_size(ent) : 0u;
    const uint32_t prel = pre0 + ent_off(ent);  // the chunk in the plane's content
    const uint32_t g = b0 + ent_idx(ent);        // the block in the frame
    // the pass's bytes: from its first entry's chunk to its last entry's end
    // (lanes past the last entry hold a copy of it)
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)prel);
    const uint32_t E = min(E_span, cpos + (uint32_t)__builtin_amdgcn_readlane((int)(prel + ent_size(ent)), 63));
    auto window = [&](uint32_t A, uint32_t& aw, uint32_t& wend, uint32_t& nq, uint32_t& nfull) {
      aw = A & ~15u;
      wend = aw + 16 * (kSpanStageQuads - 1);
      nq = E > aw ? (min(E, wend) - aw + 15) >> 4 : 0u;
      nfull = limit >= aw ? min(nq, (limit - aw) >> 4) : 0u;  // quads below limit
    };
    auto load4 = [&](uint32_t aw, uint32_t nfull) {  // (as decode_group's: every address below `limit`)
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const uint32_t o = nfull > 0 ? aw + 16 * min(lane + 64u * m, nfull - 1) : 0u;
        __builtin_amdgcn_global_load_lds((const void*)(in + o),
                                         (__attribute__((address_space(3))) void*)(stq + 64 * m), 16, 0, 0);
      }
    };
    uint32_t aw, wend, nq, nfull;
    window(cpos + first, aw, wend, nq, nfull);
    __syncthreads();  // the last pass's tile is read
    load4(aw, nfull);
    auto stage = [&]() {  // (decode_group's)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // load4's LDS writes (before the zero quads)
      for (uint32_t k = lane + 256; k < nfull; k += 64)
        stq[k] = *reinterpret_cast<const uint4*>(in + aw + 16 * k);
      for (uint32_t k = nfull + lane; k <= nq; k += 64) {
        uint32_t v[4] = {0, 0, 0, 0};
        if (k < nq) {
#pragma unroll
          for (uint32_t b = 0; b < 16; b++) {
            const uint32_t a = aw + 16 * k + b;
            if (a < limit) v[b >> 2] |= (uint32_t)in[a] << (8 * (b & 3));
          }
        }
        stq[k] = make_uint4(v[0], v[1], v[2], v[3]);
      }
      __syncthreads();
    };
    uint32_t nw[32];
#pragma unroll
    for (int w = 0; w < 32; w++) nw[w] = 0;
    int code = 0;
    bool direct = false;  // block written by decode_general
    uint64_t pending = __ballot(have);
    stage();
    while (pending) {  // rounds, as decode_group's: every round retires at least the lowest pending lane
      const bool mine = ((pending >> lane) & 1) && cpos + prel + s <= wend;
      const LdsChunk lc{reinterpret_cast<const uint32_t*>(stq), mine ? cpos + prel - aw : 0u};
      Table T;
      const int pcode = parse_table(lc, mine ? s : 0u, T, gcol);
      const bool go = mine && pcode == 0;
      int dcode = 0;
      const bool failed = decode_regular<kSpanZeroBit>(lc, T, gcol, go && T.regular, nw);
      if (go && (!T.regular || failed)) {
        direct = true;
        dcode = decode_general(lc, T, coef, gbase + g);
      }
      if (mine) code = go ? dcode : pcode;
      pending &= ~__ballot(mine);
      if (pending) {  // the next round, from the lowest pending lane's chunk
        __syncthreads();  // it overwrites the stage
        const int lo = __ffsll((long long)pending) - 1;
        window(cpos + (uint32_t)__builtin_amdgcn_readlane((int)prel, lo), aw, wend, nq, nfull);
        load4(aw, nfull);
        stage();
      }
    }
    if (have && code) record_error(err, 2ull * ((uint64_t)G.fbase * nblk + gbase + g) + 1, code);
    if (have && direct) {  // decode_general wrote the block to coef (a table the reference never writes)
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const uint4 v = coef[coef_quad(gbase + g, c)];
        nw[4 * c] = v.x;
        nw[4 * c + 1] = v.y;
        nw[4 * c + 2] = v.z;
        nw[4 * c + 3] = v.w;
      }
    }
    // ---- K6 on the pass, as k_decode_idct's on its group
    uint32_t acc = nw[0] & 0xFFFF0000u;
#pragma unroll
    for (int w = 1; w < 32; w++) acc |= nw[w];
    const bool isdc = have && acc == 0u;
    if (isdc) {
      const uint32_t v4 = dc_block_pixels((int16_t)nw[0], sq[0]);
      const uint2 row = make_uint2(v4, v4);
#pragma unroll
      for (uint32_t r = 0; r < 8; r++) *reinterpret_cast<uint2*>(fr + xf::block_row_offset(U, g - cum_p, r)) = row;
    }
    const uint64_t rest = __ballot(have && !isdc);
    const uint32_t nrest = (uint32_t)__popcll(rest);
    const uint32_t rrank =
        __builtin_amdgcn_mbcnt_hi((uint32_t)(rest >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rest, 0u));
    if (have && !isdc) s_blk[rrank] = (uint16_t)ent_idx(ent);  // compacted position -> the block in the span
#pragma unroll 1
    for (uint32_t base = 0; base < nrest;) {
      const bool wide = nrest - base > 8u;
      const uint32_t span = wide ? 16u : 8u, stride = wide ? (uint32_t)xf::kTile : (uint32_t)xf::kTile8;
      const uint32_t sl = rrank - base;
      if (have && !isdc && rrank >= base && sl < span) {
        uint4* img = reinterpret_cast<uint4*>(tile + sl * stride + (wide ? xf::img_word(sl) : 0u));
#pragma unroll
        for (int c = 0; c < 8; c++) img[c] = make_uint4(nw[4 * c], nw[4 * c + 1], nw[4 * c + 2], nw[4 * c + 3]);
      }
      if (lane < span && base + lane >= nrest) {
        uint4* img = reinterpret_cast<uint4*>(tile + lane * stride + (wide ? xf::img_word(lane) : 0u));
#pragma unroll
        for (int c = 0; c < 8; c++) img[c] = make_uint4(0u, 0u, 0u, 0u);
      }
      xf::wave_sync();
      if (wide) {
        const uint32_t q = lane & 3u, b = lane >> 2;
        uint2 w0, w1;
        xf::idct_rows(tile + b * xf::kTile, q, b, sq, w0, w1);
        if (base + b < nrest) {
          const uint32_t off = xf::block_row_offset(U, b0 - cum_p + s_blk[base + b], 2u * q);
          *reinterpret_cast<uint2*>(fr + off) = w0;
          *reinterpret_cast<uint2*>(fr + off + U.pw) = w1;
        }
      } else {
        const uint32_t r = lane & 7u, b = lane >> 3;
        float qc[8];  // the lane's column of the plane's Q table, Q[k][r]
#pragma unroll
        for (int k = 0; k < 8; k++) qc[k] = sq[8 * k + r];
        const uint2 w = xf::idct_row8(tile + b * xf::kTile8, r, qc);
        if (base + b < nrest)
          *reinterpret_cast<uint2*>(fr + xf::block_row_offset(U, b0 - cum_p + s_blk[base + b], r)) = w;
      }
      xf::wave_sync();  // the next unit rewrites the tile
      base += span;
    }
  }
}

// ---- region decode --------------------------------------------------------
//
// k_decode_region: the fused decoder for a rectangle of whole blocks of the
// frame (RegionSegs, codec_common.hpp).  One wave per segment (blockIdx.x) of
// frame blockIdx.y: a run of up to 64 consecutive blocks of one block row, so
// its chunks are one contiguous byte range of the plane's content, as a
// group's are.  The run starts anywhere in its 64-block group and may cross
// into the next one; k_scan_chain keeps offsets at group starts only, so with
// j the run's first block inside the plane its first chunk is at
//   scanned(cum_p + (j & ~63)) - scanned(cum_p) + sum of the sizes of [j & ~63, j)
// (the sum: one masked load of up to 63 size bytes and a wave scan), and lane
// l's chunk follows by the exclusive scan of the run's own sizes.  Only the
// size bytes and the run's chunks are read: a malformed chunk outside the
// rectangle is never seen.  The rows go into a frame of the rectangle's own
// geometry (R); error keys name the SOURCE frame's blocks.
//
// decode_run is decode_group's sibling (a copy of its rounds with the setup
// above in front: the two existing decoders compile to what they did).  It
// differs in three places: the size bytes are needed for the first chunk's
// position, so round 1's loads go out after them; the end of the run's
// bytes comes from the wave's own scan; and blocks with a table that is not
// "regular" are decoded (decode_general_to) into the value-position table's
// 2 KiB of LDS, dead by then, 16 lanes at a time, and read back into nw: the
// region path has no coefficient buffer in HBM.  The rounds themselves are
// decode_run_at, which takes the run as (plane, first block, length);
// decode_run picks the region segment's run and names its output blocks.
struct DecodeRun {
  uint32_t f;
  int p;
  uint32_t jo0, n;  // the run's first block in the OUTPUT plane, its length
  bool live;
};
// decode_run's rounds for the run of n <= 64 blocks that starts at block j of
// plane p of the source frame (wave-uniform), whoever chose it: the region
// path's segments (decode_run below) and the downscaler's runs (k_downscale).
// good: the lane is live and its block decoded without an error.
__device__ __forceinline__ bool decode_run_at(const uint8_t* __restrict__ in, const uint32_t* __restrict__ in_size,
                                              uint32_t cap, const StreamDesc* __restrict__ desc,
                                              const uint32_t* __restrict__ local_off,
                                              const uint32_t* __restrict__ tile_pre, const FrameGeom& G,
                                              unsigned long long* __restrict__ err, uint4* stq, const int p,
                                              const uint32_t j, const uint32_t n, uint32_t (&nw)[32], bool& live_out,
                                              bool& good) {
  const uint32_t f = blockIdx.y;
  const uint32_t nblk = G.cum[3];
  const uint32_t gbase = f * nblk;
  const uint32_t ntiles = (nblk + kScanTile - 1) / kScanTile;
  in += (size_t)f * cap;
  desc += f;
  local_off += gbase;
  tile_pre += (size_t)f * (ntiles + 1);
  const uint32_t lane = threadIdx.x;
  uint32_t* gtab = reinterpret_cast<uint32_t*>(stq + kStageQuads + 1);
  uint32_t* gcol = gtab + lane;
  auto sel3 = [p](uint32_t a0, uint32_t a1, uint32_t a2) { return p == 0 ? a0 : (p == 1 ? a1 : a2); };
  const uint32_t cum_p = sel3(G.cum[0], G.cum[1], G.cum[2]);
  // the run's group's first block, and the group's blocks in front of the run
  const uint32_t jg = j & ~(uint32_t)(kWave - 1), npre = j - jg;
  const bool live = lane < n;
  const uint32_t g = cum_p + j + lane;  // the lane's block in the source frame
  const StreamDesc dsc = *desc;
  const uint32_t isz = in_size[f];
  const uint32_t lo_p = local_off[cum_p], tp_p = tile_pre[cum_p / kScanTile];
  const uint32_t lo_g = local_off[cum_p + jg], tp_g = tile_pre[(cum_p + jg) / kScanTile];
  __builtin_amdgcn_sched_barrier(0);  // (all issued before the first use waits)
  const bool bad = dsc.bad != 0;
  const uint32_t limit = bad ? 0u : min(isz, cap);
  const uint32_t cpos = sel3(dsc.content_pos[0], dsc.content_pos[1], dsc.content_pos[2]);
  const uint32_t csize = sel3(dsc.content_size[0], dsc.content_size[1], dsc.content_size[2]);
  const uint32_t spos = sel3(dsc.sizes_pos[0], dsc.sizes_pos[1], dsc.sizes_pos[2]);
  // the lane's own size byte and the size byte of block jg + lane in front of
  // the run, loaded together (both inside the plane's size table: the header
  // checks passed, or `bad` and byte 0)
  const uint32_t s = in[bad ? 0u : spos + j + (live ? lane : n - 1u)];
  const uint32_t sp = in[bad ? 0u : spos + jg + (lane < npre ? lane : 0u)];
  const uint32_t incl = wave_incl_scan(live ? s : 0u);
  const uint32_t pincl = wave_incl_scan(lane < npre ? sp : 0u);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  const uint32_t pre0 = (lo_g + tp_g) - (lo_p + tp_p) + (uint32_t)__builtin_amdgcn_readlane((int)pincl, 63);
  const uint32_t rel = pre0 + incl - (live ? s : 0u);
  // end of the run's chunk range, inside the declared content
  const uint32_t E = cpos + min(pre0 + total, csize);
  auto window = [&](uint32_t A, uint32_t& aw, uint32_t& wend, uint32_t& nq, uint32_t& nfull) {
    aw = A & ~15u;
    wend = aw + 16 * (kStageQuads - 1);
    nq = E > aw ? (min(E, wend) - aw + 15) >> 4 : 0u;
    nfull = limit >= aw ? min(nq, (limit - aw) >> 4) : 0u;  // quads below limit
  };
  auto load4 = [&](uint32_t aw, uint32_t nfull) {  // (as decode_group's: every address below `limit`)
#pragma unroll
    for (int m = 0; m < 4; m++) {
      const uint8_t* src = nfull > 0 ? in + aw + 16 * min(lane + 64u * m, nfull - 1) : in;
      __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)(stq + 64 * m),
                                       16, 0, 0);
    }
  };
  uint32_t aw, wend, nq, nfull;
  window(cpos + pre0, aw, wend, nq, nfull);
  load4(aw, nfull);

  // plane-level check, for the rectangle's blocks
  bool ok = live && !bad;
  if (ok && rel + s > csize) {
    record_error(err, 2ull * ((uint64_t)G.fbase * nblk + gbase + cum_p), 9 /* MYYUV_E_PLANE_CONTENT */);
    ok = false;
  }

  int code = 0;
  uint64_t pending = __ballot(ok);
  auto stage = [&]() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // load4's LDS writes (before the zero quads)
    for (uint32_t q = lane + 256; q < nfull; q += 64)
      stq[q] = *reinterpret_cast<const uint4*>(in + aw + 16 * q);
    for (uint32_t q = nfull + lane; q <= nq; q += 64) {
      uint32_t v[4] = {0, 0, 0, 0};
      if (q < nq) {
#pragma unroll
        for (uint32_t b = 0; b < 16; b++) {
          const uint32_t a = aw + 16 * q + b;
          if (a < limit) v[b >> 2] |= (uint32_t)in[a] << (8 * (b & 3));
        }
      }
      stq[q] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
  };
  if (pending) stage();
  while (pending) {
    const bool mine = ((pending >> lane) & 1) && cpos + rel + s <= wend;
    const LdsChunk lc{reinterpret_cast<const uint32_t*>(stq), mine ? cpos + rel - aw : 0u};
    Table T;
    const int pcode = parse_table(lc, mine ? s : 0u, T, gcol);
    const bool go = mine && pcode == 0;
    int dcode = 0;
    const bool failed = decode_regular(lc, T, gcol, go && T.regular, nw);
    // the bit-serial path (tables the reference never writes, and failed
    // messages for the reference's exact code), 16 lanes at a time: lane of
    // rank r among them owns 128 B (64 int16, natural order) at 128 r of the
    // value-position table, which the next round's parse rewrites
    uint64_t dm = __ballot(go && (!T.regular || failed));
    while (dm) {
      const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(dm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)dm, 0u));
      const bool sel = ((dm >> lane) & 1) && rk < 16u;
      if (sel) {
        uint16_t* slot = reinterpret_cast<uint16_t*>(gtab) + 64u * rk;
        dcode = decode_general_to(lc, T, [=](uint32_t z, uint16_t v) { slot[z] = v; });
        const uint4* img = reinterpret_cast<const uint4*>(slot);
#pragma unroll
        for (int c = 0; c < 8; c++) {
          const uint4 v = img[c];
          nw[4 * c] = v.x;
          nw[4 * c + 1] = v.y;
          nw[4 * c + 2] = v.z;
          nw[4 * c + 3] = v.w;
        }
      }
      dm &= ~__ballot(sel);
    }
    if (mine) code = go ? dcode : pcode;
    pending &= ~__ballot(mine);
    if (pending) {  // the next round, from the lowest pending lane's chunk
      __syncthreads();  // it overwrites the stage
      const int lo = __ffsll((long long)pending) - 1;
      window(cpos + __shfl(rel, lo, 64), aw, wend, nq, nfull);
      load4(aw, nfull);
      stage();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every LDS-DMA load has landed (whether or not a round ran)
  if (ok && code) record_error(err, 2ull * ((uint64_t)G.fbase * nblk + gbase + g) + 1, code);
  live_out = live;
  good = ok && code == 0;
  return !bad;
}

__device__ __forceinline__ bool decode_run(const uint8_t* __restrict__ in, const uint32_t* __restrict__ in_size,
                                           uint32_t cap, const StreamDesc* __restrict__ desc,
                                           const uint32_t* __restrict__ local_off,
                                           const uint32_t* __restrict__ tile_pre, const FrameGeom& G,
                                           const FrameGeom& R, const RegionSegs& S,
                                           unsigned long long* __restrict__ err, uint4* stq, DecodeRun& D,
                                           uint32_t (&nw)[32]) {
  const uint32_t t = blockIdx.x;
  const int p = t >= S.scum[1] ? (t >= S.scum[2] ? 2 : 1) : 0;
  auto sel3 = [p](uint32_t a0, uint32_t a1, uint32_t a2) { return p == 0 ? a0 : (p == 1 ? a1 : a2); };
  const uint32_t spr = sel3(S.spr[0], S.spr[1], S.spr[2]);
  const uint32_t ts = t - sel3(0u, S.scum[1], S.scum[2]);
  const uint32_t row = ts / spr, k = ts - row * spr;
  const uint32_t rbw = sel3(R.bw[0], R.bw[1], R.bw[2]), sbw = sel3(G.bw[0], G.bw[1], G.bw[2]);
  const uint32_t n = min((uint32_t)kWave, rbw - kWave * k);
  // the run's first block inside the source plane
  const uint32_t j = (sel3(S.by[0], S.by[1], S.by[2]) + row) * sbw + sel3(S.bx[0], S.bx[1], S.bx[2]) + kWave * k;
  bool good;
  const bool frame_ok =
      decode_run_at(in, in_size, cap, desc, local_off, tile_pre, G, err, stq, p, j, n, nw, D.live, good);
  D.f = blockIdx.y;
  D.p = p;
  D.jo0 = row * rbw + kWave * k;
  D.n = n;
  return frame_ok;
}

__global__ __launch_bounds__(64, MYYUV_K5_WAVES) void k_decode_region(const uint8_t* __restrict__ in,
                                                     const uint32_t* __restrict__ in_size,
                                                     uint32_t cap,
                                                     const StreamDesc* __restrict__ desc,
                                                     const uint32_t* __restrict__ local_off,
                                                     const uint32_t* __restrict__ tile_pre,
                                                     FrameGeom G, FrameGeom R, RegionSegs S,
                                                     const QTables* __restrict__ qt,
                                                     uint8_t* __restrict__ frame,
                                                     unsigned long long* __restrict__ err) {
  static_assert(sizeof(uint4) * kStageQuads >= sizeof(float) * xf::kXfTile16, "the tile over the stage");
  static_assert(kGposQuads * 16 >= 16 * 128, "16 blocks of int16[64] in the value-position table");
  __shared__ uint4 stq[kStageQuads + 1 + kGposQuads];
  __shared__ float sq[64];
  __shared__ uint16_t s_blk[64];
  const uint32_t lane = threadIdx.x;
  if (lane == 0) stq[kStageQuads] = make_uint4(0u, 0u, 0u, 0u);  // (ordered by decode_run's barrier)
  {
    // the plane's Q table by LDS-DMA (landed by decode_run's final vmcnt wait)
    const uint32_t t = blockIdx.x;
    const int p = t >= S.scum[1] ? (t >= S.scum[2] ? 2 : 1) : 0;
    __builtin_amdgcn_global_load_lds((const void*)&qt->q[p][lane], (__attribute__((address_space(3))) void*)sq, 4,
                                     0, 0);
  }
  DecodeRun D;
  uint32_t nw[32];
#pragma unroll
  for (int w = 0; w < 32; w++) nw[w] = 0;
  if (!decode_run(in, in_size, cap, desc, local_off, tile_pre, G, R, S, err, stq, D, nw))
    return;  // the frame's stream header is bad (k_scan_chain recorded it)
  // ---- K6 on the run, as k_decode_idct's on its group, into the output
  // frame's geometry: lane l's block is block jo0 + l of plane p of R
  const int p = D.p;
  xf::Unit U;
  U.p = p;
  U.cum = R.cum[p];
  U.nb = R.cum[p + 1] - R.cum[p];
  U.poff = p == 0 ? R.poff[0] : (p == 1 ? R.poff[1] : R.poff[2]);
  U.pw = p == 0 ? R.pw[0] : (p == 1 ? R.pw[1] : R.pw[2]);
  U.bw = p == 0 ? R.bw[0] : (p == 1 ? R.bw[1] : R.bw[2]);
  U.bmag = p == 0 ? R.bmag[0] : (p == 1 ? R.bmag[1] : R.bmag[2]);
  U.local0 = 0;
  uint8_t* fr = frame + (size_t)D.f * R.fbytes;
  uint32_t acc = nw[0] & 0xFFFF0000u;
#pragma unroll
  for (int w = 1; w < 32; w++) acc |= nw[w];
  const bool isdc = D.live && acc == 0u;
  if (isdc) {  // the DC-only constant block (see k_decode_idct)
    constexpr float c0 = xf::c_dct[0];
    const float z = (float)(int16_t)nw[0] * sq[0];  // dequantise (DCT.cpp:331)
    const float u = 0.0f + c0 * z;                  // stage 1: the k = 0 term
    float Sv = 0.0f + u * c0;                       // stage 2: the k = 0 term
    Sv = __builtin_amdgcn_fmed3f(Sv, -128.0f, 127.0f);  // (as idct_rows, DCT.cpp:358-362)
    uint32_t px = xf::bits(Sv + xf::kMagicPx);
    if (__builtin_amdgcn_fractf(Sv) == 0.5f)
      px = (uint32_t)((int)__builtin_truncf(Sv + __builtin_copysignf(xf::kHalfDown, Sv)) + 128);
    const uint32_t v4 = (px & 0xFFu) * 0x01010101u;
    const uint2 rowv = make_uint2(v4, v4);
#pragma unroll
    for (uint32_t r = 0; r < 8; r++)
      *reinterpret_cast<uint2*>(fr + xf::block_row_offset(U, D.jo0 + lane, r)) = rowv;
  }
  const uint64_t rest = __ballot(D.live && !isdc);
  const uint32_t nrest = (uint32_t)__popcll(rest);
  const uint32_t rrank = __builtin_amdgcn_mbcnt_hi((uint32_t)(rest >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rest, 0u));
  if (D.live && !isdc) s_blk[rrank] = (uint16_t)lane;  // compacted position -> the block's lane in the run
  float* tile = reinterpret_cast<float*>(stq);
#pragma unroll 1
  for (uint32_t base = 0; base < nrest;) {
    const bool wide = nrest - base > 8u;
    const uint32_t span = wide ? 16u : 8u, stride = wide ? (uint32_t)xf::kTile : (uint32_t)xf::kTile8;
    const uint32_t s = rrank - base;
    if (D.live && !isdc && rrank >= base && s < span) {
      uint4* img = reinterpret_cast<uint4*>(tile + s * stride + (wide ? xf::img_word(s) : 0u));
#pragma unroll
      for (int c = 0; c < 8; c++) img[c] = make_uint4(nw[4 * c], nw[4 * c + 1], nw[4 * c + 2], nw[4 * c + 3]);
    }
    if (lane < span && base + lane >= nrest) {
      uint4* img = reinterpret_cast<uint4*>(tile + lane * stride + (wide ? xf::img_word(lane) : 0u));
#pragma unroll
      for (int c = 0; c < 8; c++) img[c] = make_uint4(0u, 0u, 0u, 0u);
    }
    xf::wave_sync();
    if (wide) {
      const uint32_t q = lane & 3u, b = lane >> 2;
      uint2 w0, w1;
      xf::idct_rows(tile + b * xf::kTile, q, b, sq, w0, w1);
      if (base + b < nrest) {
        const uint32_t off = xf::block_row_offset(U, D.jo0 + s_blk[base + b], 2u * q);
        *reinterpret_cast<uint2*>(fr + off) = w0;
        *reinterpret_cast<uint2*>(fr + off + U.pw) = w1;
      }
    } else {
      const uint32_t r = lane & 7u, b = lane >> 3;
      float qc[8];  // the lane's column of the plane's Q table, Q[k][r]
#pragma unroll
      for (int kk = 0; kk < 8; kk++) qc[kk] = sq[8 * kk + r];
      const uint2 w = xf::idct_row8(tile + b * xf::kTile8, r, qc);
      if (base + b < nrest)
        *reinterpret_cast<uint2*>(fr + xf::block_row_offset(U, D.jo0 + s_blk[base + b], r)) = w;
    }
    xf::wave_sync();  // the next unit rewrites the tile
    base += span;
  }
}

// ---- scaled decode --------------------------------------------------------
//
// k_decode_scaled<N>: the fused decoder at 1/denom size, N = 8 / denom in
// {4, 2, 1} (include/myyuv_hip.h, "Scaled decode").  Grid and decode are
// k_decode_idct's: one wave per 64-block group (blockIdx.x) of frame
// blockIdx.y, decode_group unchanged, so the whole chunk is decoded and a
// malformed one gives the full decode's code and block; a block with a table
// that is not "regular" goes through the coefficient buffer as there.  Then
// each lane transforms the N x N low-frequency corner of its own block from
// its nw[] registers (idct_scaled.h: at most 16 coefficients, 128 products;
// no transpose tile) and stores N rows of N bytes at block (by, bx) of the
// plane's (bw N) x (bh N) image: a group's blocks are consecutive in a block
// row, so consecutive lanes write adjacent bytes.  Every offset of a row is a
// multiple of N bytes (plane offsets and widths are), so a row is one store of
// N bytes.
template <int N>
__global__ __launch_bounds__(64, MYYUV_K5_WAVES) void k_decode_scaled(const uint8_t* __restrict__ in,
                                                     const uint32_t* __restrict__ in_size,
                                                     uint32_t cap,
                                                     const StreamDesc* __restrict__ desc,
                                                     const uint32_t* __restrict__ local_off,
                                                     const uint32_t* __restrict__ tile_pre,
                                                     FrameGeom G, uint32_t tiles_p0,
                                                     uint32_t tiles_p1, const QTables* __restrict__ qt,
                                                     uint4* __restrict__ coef,
                                                     uint8_t* __restrict__ frame,
                                                     unsigned long long* __restrict__ err) {
  static_assert(N == 1 || N == 2 || N == 4, "1/8, 1/4 or 1/2");
  __shared__ uint4 stq[kStageQuads + 1 + kGposQuads];
  __shared__ float sq[64];
  const uint32_t lane = threadIdx.x;
  if (lane == 0) stq[kStageQuads] = make_uint4(0u, 0u, 0u, 0u);  // (ordered by decode_group's barrier)
  {
    // the plane's Q table by LDS-DMA (landed by decode_group's final vmcnt wait)
    const uint32_t t = blockIdx.x;
    const int p = t >= tiles_p0 ? (t >= tiles_p0 + tiles_p1 ? 2 : 1) : 0;
    __builtin_amdgcn_global_load_lds((const void*)&qt->q[p][lane], (__attribute__((address_space(3))) void*)sq, 4,
                                     0, 0);
  }
  DecodeGroup D;
  uint32_t nw[32];
#pragma unroll
  for (int w = 0; w < 32; w++) nw[w] = 0;
  bool direct;
  if (!decode_group(in, in_size, cap, desc, local_off, tile_pre, G, tiles_p0, tiles_p1, coef, err, stq, D, nw,
                    direct))
    return;  // the frame's stream header is bad (k_scan_chain recorded it)
  if (!D.live) return;
  // the corner's coefficients, natural order: coefficient 8 u + v is half
  // v & 1 of word 4 u + (v >> 1).  decode_general wrote a `direct` block to
  // coef: the corner's rows (quad u = row u) are read back.
  int16_t z[N * N];
  float q[N * N];
#pragma unroll
  for (int u = 0; u < N; u++) {
    uint32_t w0 = nw[4 * u], w1 = nw[4 * u + 1];
    if (direct) {
      const uint4 v = coef[coef_quad(D.gbase + D.g, u)];
      w0 = v.x;
      w1 = v.y;
    }
#pragma unroll
    for (int v = 0; v < N; v++) {
      const uint32_t w = v < 2 ? w0 : w1;
      z[u * N + v] = (int16_t)((v & 1) ? w >> 16 : w & 0xFFFFu);
      q[u * N + v] = sq[8 * u + v];
    }
  }
  uint8_t px[N * N];
  myyuv_scaled::idct_scaled_block<N>(z, q, px);
  // plane p of the scaled frame: offsets and sizes are the full frame's
  // divided by denom^2 = 64 / N^2 (whole: W and H are multiples of 16)
  const int p = D.p;
  const uint32_t cum = p == 0 ? G.cum[0] : (p == 1 ? G.cum[1] : G.cum[2]);
  const uint32_t poff = p == 0 ? G.poff[0] : (p == 1 ? G.poff[1] : G.poff[2]);
  const uint32_t bw = p == 0 ? G.bw[0] : (p == 1 ? G.bw[1] : G.bw[2]);
  const uint64_t bmag = p == 0 ? G.bmag[0] : (p == 1 ? G.bmag[1] : G.bmag[2]);
  const uint32_t local = D.g - cum;
  const uint32_t by = div_magic(local, bmag), bx = local - by * bw;
  const uint32_t pwn = bw * N;
  uint8_t* o = frame + (size_t)D.f * ((G.fbytes >> 6) * (N * N)) + (poff >> 6) * (N * N) + by * N * pwn + bx * N;
#pragma unroll
  for (int i = 0; i < N; i++) {
    if constexpr (N == 1) {
      o[0] = px[0];
    } else if constexpr (N == 2) {
      *reinterpret_cast<uint16_t*>(o + i * pwn) = (uint16_t)(px[2 * i] | (px[2 * i + 1] << 8));
    } else {
      *reinterpret_cast<uint32_t*>(o + i * pwn) =
          (uint32_t)px[4 * i] | ((uint32_t)px[4 * i + 1] << 8) | ((uint32_t)px[4 * i + 2] << 16) |
          ((uint32_t)px[4 * i + 3] << 24);
    }
  }
}
template __global__ void k_decode_scaled<1>(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*,
                                            const uint32_t*, const uint32_t*, FrameGeom, uint32_t, uint32_t,
                                            const QTables*, uint4*, uint8_t*, unsigned long long*);
template __global__ void k_decode_scaled<2>(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*,
                                            const uint32_t*, const uint32_t*, FrameGeom, uint32_t, uint32_t,
                                            const QTables*, uint4*, uint8_t*, unsigned long long*);
template __global__ void k_decode_scaled<4>(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*,
                                            const uint32_t*, const uint32_t*, FrameGeom, uint32_t, uint32_t,
                                            const QTables*, uint4*, uint8_t*, unsigned long long*);

// ---- downscale ------------------------------------------------------------
//
// k_downscale<N>: a DCT stream at 1/denom size from a DCT stream, N = 8 / denom
// in {4, 2, 1} (include/myyuv_hip.h, "Downscale"): the scaled decode, K1 and
// its exact path in one launch, the scaled frame never in HBM.  The work map is
// downscale.h's: wave blockIdx.x of frame blockIdx.y owns a segment of a band
// (up to 64 source block columns of the denom source block rows under one
// output block row).
//  - Decode: the band as denom runs, one after the other (decode_run_at: each
//    run one contiguous byte range, one chunk per lane, the whole chunk decoded;
//    tables that are not "regular" in the value-position table, as the region
//    path).  After a run every lane transforms its block's N x N corner
//    (idct_scaled_block<N>, the scaled decode's arithmetic and clamp) and
//    writes its N rows of N bytes into the wave's pixel image: the wave's
//    output blocks as 8 x 8-byte block images (lane_pixel).  The image is an
//    LDS array of its own: the stage is live again in the next run.
//  - Forward transform: the wave's n / denom output blocks in units of 16, four
//    lanes per block (fdct_core: K1's fast path, and on a failed proof the
//    exact path in the same wave, so there is no fix list).  The transpose tile
//    lies over the stage, which is dead after the last run.  Each unit's quads,
//    row masks and info words go out as K1's do (store_block_rows_buf) at the
//    DESTINATION block index; block slots past the wave's output are dropped
//    by the descriptors' range.
// The zero-block rule of k_requant holds at the destination: every output
// block belongs to exactly one wave, and the wave writes its mask and info word
// whatever the stream holds.  A lane whose chunk failed, and every lane of a
// frame whose header k_scan_chain rejected, contributes zero coefficients,
// that is pixel 128; the error is in the shared error word, keyed by the
// SOURCE block (record_error's minimum: decompress's first bad block in any
// wave order).
// (4 waves per SIMD: the wave's LDS, 10-11 KiB with the image and K1's tables,
// admits 16 workgroups per CU)
template <int N>
__global__ __launch_bounds__(64, 4) void k_downscale(const uint8_t* __restrict__ in,
                                                 const uint32_t* __restrict__ in_size,
                                                 uint32_t cap,
                                                 const StreamDesc* __restrict__ desc,
                                                 const uint32_t* __restrict__ local_off,
                                                 const uint32_t* __restrict__ tile_pre,
                                                 FrameGeom G, FrameGeom Gd, myyuv_downscale::Map M,
                                                 const DownscaleTables* __restrict__ dt,
                                                 uint4* __restrict__ coef,
                                                 uint8_t* __restrict__ rmask,
                                                 uint32_t* __restrict__ binfo,
                                                 unsigned long long* __restrict__ err) {
  static_assert(N == 1 || N == 2 || N == 4, "1/8, 1/4 or 1/2");
  constexpr uint32_t kDen = 8 / N;
  // the wave's output blocks (64 / denom), and at least one 16-block unit
  constexpr uint32_t kImgBlocks = kWave / kDen > kXfUnit ? kWave / kDen : kXfUnit;
  static_assert(sizeof(uint4) * kStageQuads >= sizeof(float) * xf::kXfTile16,
                "the transpose tile over the stage (dead after the last run)");
  static_assert(kGposQuads * 16 >= 16 * 128, "16 blocks of int16[64] in the value-position table");
  static_assert(myyuv_downscale::kSeg == kWave, "a lane per source block column");
  static_assert(offsetof(QTables, r) == sizeof(float) * xf::kSqR && offsetof(QTables, kb) == sizeof(float) * xf::kSqKb,
                "layout");
  __shared__ uint4 stq[kStageQuads + 1 + kGposQuads];
  __shared__ uint4 simg[kImgBlocks * 4];  // the pixel image: NOT over the stage, which the next run refills
  __shared__ float sqs[64];               // the source plane's Q table
  __shared__ float sqr[xf::kSqWords];     // the destination's QTables (the wave's plane filled in)
  __shared__ uint4 szz[8];
  const uint32_t lane = threadIdx.x;
  const myyuv_downscale::Wave W = myyuv_downscale::wave_of(M, blockIdx.x);
  const int p = W.p;
  if (lane == 0) stq[kStageQuads] = make_uint4(0u, 0u, 0u, 0u);  // (ordered by decode_run_at's barrier)
  // the plane's tables by LDS-DMA (landed by decode_run_at's final vmcnt wait)
  __builtin_amdgcn_global_load_lds((const void*)&dt->qs[p][lane], (__attribute__((address_space(3))) void*)sqs, 4, 0,
                                   0);
  __builtin_amdgcn_global_load_lds((const void*)&dt->d.q[p][lane],
                                   (__attribute__((address_space(3))) void*)(sqr + p * 64), 4, 0, 0);
  __builtin_amdgcn_global_load_lds((const void*)&dt->d.r[p][lane],
                                   (__attribute__((address_space(3))) void*)(sqr + xf::kSqR + p * 64), 4, 0, 0);
  if (lane < 8) sqr[xf::kSqKb + p * 8 + lane] = dt->d.kb[p][lane];
  xf::stage_zz(szz);
  // pixel 128 everywhere: block slots past the wave's output are transformed
  // with the rest of their unit
  for (uint32_t i = lane; i < kImgBlocks * 4; i += kWave)
    simg[i] = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
  uint8_t* img = reinterpret_cast<uint8_t*>(simg);

#pragma unroll 1
  for (uint32_t r = 0; r < kDen; r++) {
    if (r != 0) __syncthreads();  // the run's loads overwrite the stage
    uint32_t nw[32];
#pragma unroll
    for (int w = 0; w < 32; w++) nw[w] = 0;
    bool live, good;
    (void)decode_run_at(in, in_size, cap, desc, local_off, tile_pre, G, err, stq, p,
                        myyuv_downscale::run_first(M, W, r), W.n, nw, live, good);
    // the corner's coefficients, natural order (see k_decode_scaled); a lane
    // that is not `good` (a failed chunk: partial symbols; a rejected frame; a
    // lane past the run) takes zeros
    int16_t z[N * N];
    float q[N * N];
#pragma unroll
    for (int u = 0; u < N; u++) {
      const uint32_t w0 = good ? nw[4 * u] : 0u, w1 = good ? nw[4 * u + 1] : 0u;
#pragma unroll
      for (int v = 0; v < N; v++) {
        const uint32_t w = v < 2 ? w0 : w1;
        z[u * N + v] = (int16_t)((v & 1) ? w >> 16 : w & 0xFFFFu);
        q[u * N + v] = sqs[8 * u + v];
      }
    }
    uint8_t px[N * N];
    myyuv_scaled::idct_scaled_block<N>(z, q, px);
    if (live) {
#pragma unroll
      for (int i = 0; i < N; i++) {
        uint8_t* o = img + myyuv_downscale::lane_pixel(kDen, r, lane, (uint32_t)i);
        if constexpr (N == 1) {
          o[0] = px[0];
        } else if constexpr (N == 2) {
          *reinterpret_cast<uint16_t*>(o) = (uint16_t)(px[2 * i] | (px[2 * i + 1] << 8));
        } else {
          *reinterpret_cast<uint32_t*>(o) = (uint32_t)px[4 * i] | ((uint32_t)px[4 * i + 1] << 8) |
                                            ((uint32_t)px[4 * i + 2] << 16) | ((uint32_t)px[4 * i + 3] << 24);
        }
      }
    }
  }
  xf::wave_sync();  // the image is complete; the stage is dead

  // ---- K1's per-unit body on the wave's output blocks, lane (b, q)
  const uint32_t q = lane & 3u, b = lane >> 2;
  float* tb = reinterpret_cast<float*>(stq) + b * xf::kTile;
  const xf::K1Rsrc rs = xf::k1_rsrc(coef, rmask, binfo, Gd);
  const uint32_t g0 = blockIdx.y * Gd.cum[3] + (p == 0 ? Gd.cum[0] : (p == 1 ? Gd.cum[1] : Gd.cum[2]));
#pragma unroll 1
  for (uint32_t u0 = 0; u0 < W.nout; u0 += kXfUnit) {
    const uint32_t slot = u0 + b;  // (< kImgBlocks: nout <= 64 / denom)
    const bool lv = slot < W.nout;
    const uint32_t g = g0 + myyuv_downscale::out_block(W, slot);
    xf::fdct_core(img + 64u * slot, tb, q, lv, sqr, p, [&](const uint32_t (&c)[16], bool keep, auto hz) {
      xf::store_block_rows_buf<decltype(hz)::value>(c, q, lv && keep, g, rs, szz);
    });
    xf::wave_sync();  // the next unit rewrites the tile
  }
}
#define MYYUV_DOWNSCALE_INST(N)                                                                                   \
  template __global__ void k_downscale<N>(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*,           \
                                          const uint32_t*, const uint32_t*, FrameGeom, FrameGeom,                 \
                                          myyuv_downscale::Map, const DownscaleTables*, uint4*, uint8_t*,         \
                                          uint32_t*, unsigned long long*);
MYYUV_DOWNSCALE_INST(1)
MYYUV_DOWNSCALE_INST(2)
MYYUV_DOWNSCALE_INST(4)
#undef MYYUV_DOWNSCALE_INST

// ---- requantise -----------------------------------------------------------
//
// k_requant: the decoder half of the requantiser (include/myyuv_hip.h,
// "Requantise").  Grid and decode are k_decode_idct's: one wave per 64-block
// group (blockIdx.x) of frame blockIdx.y, decode_group unchanged; a block with
// a table that is not "regular" goes through the coefficient buffer as there
// and is read back.  Then each lane rescales its block's 64 coefficients from
// the source plane's table to the destination's in its nw[] registers
// (requant.h; an all-zero row stays zero and is skipped) and writes K1's
// hand-off for K2: the nonzero rows as natural-order quads, the row mask and
// the block's info word, with msz and the class of the REQUANTISED block.
//
// Every live lane writes a mask and an info word, whatever the stream holds:
// a lane whose chunk failed (D.good false: the partial symbols decode_regular
// left in nw are dropped), and every lane of a frame whose header
// k_scan_chain rejected, hands over an all-zero block (mask 0, msz 0, the
// single class).  K2 indexes by these words, so it never sees what the
// workspace held before; the error itself is in the shared error word.
__global__ __launch_bounds__(64, MYYUV_K5_WAVES) void k_requant(const uint8_t* __restrict__ in,
                                               const uint32_t* __restrict__ in_size,
                                               uint32_t cap,
                                               const StreamDesc* __restrict__ desc,
                                               const uint32_t* __restrict__ local_off,
                                               const uint32_t* __restrict__ tile_pre,
                                               FrameGeom G, uint32_t tiles_p0,
                                               uint32_t tiles_p1, const RequantTables* __restrict__ rt,
                                               uint4* __restrict__ coef,
                                               uint8_t* __restrict__ rmask,
                                               uint32_t* __restrict__ binfo,
                                               unsigned long long* __restrict__ err) {
  __shared__ uint4 stq[kStageQuads + 1 + kGposQuads];
  __shared__ float sqs[64], sqd[64];
  const uint32_t lane = threadIdx.x;
  if (lane == 0) stq[kStageQuads] = make_uint4(0u, 0u, 0u, 0u);  // (ordered by decode_group's barrier)
  {
    // the plane's two Q tables by LDS-DMA (landed by decode_group's final vmcnt wait)
    const uint32_t t = blockIdx.x;
    const int p = t >= tiles_p0 ? (t >= tiles_p0 + tiles_p1 ? 2 : 1) : 0;
    __builtin_amdgcn_global_load_lds((const void*)&rt->qs[p][lane], (__attribute__((address_space(3))) void*)sqs, 4,
                                     0, 0);
    __builtin_amdgcn_global_load_lds((const void*)&rt->qd[p][lane], (__attribute__((address_space(3))) void*)sqd, 4,
                                     0, 0);
  }
  DecodeGroup D;
  CoefRegs R;
  uint32_t(&nw)[32] = R.w;
#pragma unroll
  for (int w = 0; w < 32; w++) nw[w] = 0;
  bool direct;
  const bool frame_ok = decode_group(in, in_size, cap, desc, local_off, tile_pre, G, tiles_p0, tiles_p1, coef, err,
                                     stq, D, nw, direct);
  if (!D.live) return;
  const uint32_t g = D.gbase + D.g;
  const bool keep = frame_ok && D.good;
  if (keep && direct) {  // decode_general wrote the block to coef (a table the reference never writes)
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const uint4 v = coef[coef_quad(g, c)];
      nw[4 * c] = v.x;
      nw[4 * c + 1] = v.y;
      nw[4 * c + 2] = v.z;
      nw[4 * c + 3] = v.w;
    }
  }
#pragma unroll
  for (int w = 0; w < 32; w++) nw[w] = keep ? nw[w] : 0u;
  requant_handoff(R, g, true, sqs, sqd, coef, rmask, binfo);
}

// ---- transform ------------------------------------------------------------
//
// k_coef_xform: the decoder half of the coefficient-domain transform
// (include/myyuv_hip.h, "Transform": flip, rotate, transpose).  Grid, decode
// and hand-off are k_requant's, with two differences.
//  - decode_general writes an irregular-table block at the SOURCE index of the
//    buffer it is given, and that slot of the hand-off image is some other
//    wave's destination: the decode gets a scratch image of its own (`gen`),
//    and the block is read back from there.
//  - Each lane moves its block inside its registers (coef_xform.h: the
//    transpose with static register indices, the rescale where the plane's two
//    tables differ, the mirrors' signs) and writes quads, mask and info word
//    at the block's DESTINATION index, xf_dest_block of its position in the
//    plane.  `rt->qs` is the source table as the transposed block reads it
//    (xf_source_table, by the host); bit p of `eq`: plane p's two tables are
//    equal, the rescale is the identity and is skipped.
// The zero-block rule of k_requant holds at the destination: the map is a
// bijection of the plane's blocks and every live lane writes, whatever the
// stream holds, so every destination block has exactly one writer.
// For a mirror the wave's 64 quads of a row land reversed inside one or two
// 1 KiB runs of the image; for a swap every lane's quad lands in a run of its
// own ("Transform", has the measurement).
__global__ __launch_bounds__(64, MYYUV_K5_WAVES) void k_coef_xform(const uint8_t* __restrict__ in,
                                                  const uint32_t* __restrict__ in_size,
                                                  uint32_t cap,
                                                  const StreamDesc* __restrict__ desc,
                                                  const uint32_t* __restrict__ local_off,
                                                  const uint32_t* __restrict__ tile_pre,
                                                  FrameGeom G, uint32_t tiles_p0,
                                                  uint32_t tiles_p1, const RequantTables* __restrict__ rt,
                                                  uint32_t op, uint32_t eq,
                                                  uint4* __restrict__ gen,
                                                  uint4* __restrict__ coef,
                                                  uint8_t* __restrict__ rmask,
                                                  uint32_t* __restrict__ binfo,
                                                  unsigned long long* __restrict__ err) {
  __shared__ uint4 stq[kStageQuads + 1 + kGposQuads];
  __shared__ float sqs[64], sqd[64];
  const uint32_t lane = threadIdx.x;
  if (lane == 0) stq[kStageQuads] = make_uint4(0u, 0u, 0u, 0u);  // (ordered by decode_group's barrier)
  {
    // the plane's two Q tables by LDS-DMA (landed by decode_group's final vmcnt wait)
    const uint32_t t = blockIdx.x;
    const int p = t >= tiles_p0 ? (t >= tiles_p0 + tiles_p1 ? 2 : 1) : 0;
    __builtin_amdgcn_global_load_lds((const void*)&rt->qs[p][lane], (__attribute__((address_space(3))) void*)sqs, 4,
                                     0, 0);
    __builtin_amdgcn_global_load_lds((const void*)&rt->qd[p][lane], (__attribute__((address_space(3))) void*)sqd, 4,
                                     0, 0);
  }
  DecodeGroup D;
  CoefRegs R;
  uint32_t(&nw)[32] = R.w;
#pragma unroll
  for (int w = 0; w < 32; w++) nw[w] = 0;
  bool direct;
  const bool frame_ok = decode_group(in, in_size, cap, desc, local_off, tile_pre, G, tiles_p0, tiles_p1, gen, err,
                                     stq, D, nw, direct);
  if (!D.live) return;
  const bool keep = frame_ok && D.good;
  if (keep && direct) {  // decode_general wrote the block to the scratch image, at the source index
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const uint4 v = gen[coef_quad(D.gbase + D.g, c)];
      nw[4 * c] = v.x;
      nw[4 * c + 1] = v.y;
      nw[4 * c + 2] = v.z;
      nw[4 * c + 3] = v.w;
    }
  }
#pragma unroll
  for (int w = 0; w < 32; w++) nw[w] = keep ? nw[w] : 0u;
  // the destination block (plane fields by static index, as decode_group)
  const int p = D.p;
  const uint32_t cum_p = p == 0 ? G.cum[0] : (p == 1 ? G.cum[1] : G.cum[2]);
  const uint32_t bw = p == 0 ? G.bw[0] : G.bw[1];                // (planes 1 and 2 have one shape)
  const uint32_t bh = (p == 0 ? G.ph[0] : G.ph[1]) >> 3;
  const uint32_t local = D.g - cum_p;
  const uint32_t by = div_magic(local, p == 0 ? G.bmag[0] : G.bmag[1]);
  const uint32_t g = D.gbase + cum_p + myyuv_xform::xf_dest_block(op, bw, bh, local - by * bw, by);
  if (op & myyuv_xform::kSwap) {  // (wave-uniform)
    uint32_t t[32];
    myyuv_xform::xf_transpose(nw, t);
#pragma unroll
    for (int w = 0; w < 32; w++) nw[w] = t[w];
  }
  const bool mx = (op & myyuv_xform::kMirrorX) != 0, my = (op & myyuv_xform::kMirrorY) != 0;
  const bool same = (eq >> p) & 1u;
  uint32_t m = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    if ((nw[4 * c] | nw[4 * c + 1] | nw[4 * c + 2] | nw[4 * c + 3]) != 0u) {
      if (!same) myyuv_xform::xf_rescale_row(nw, c, sqs + 8 * c, sqd + 8 * c);
      myyuv_xform::xf_sign_row(nw, c, mx, my);
    }
    const bool nz = (nw[4 * c] | nw[4 * c + 1] | nw[4 * c + 2] | nw[4 * c + 3]) != 0u;
    m |= nz ? 1u << c : 0u;
    if (nz) coef[coef_quad(g, c)] = make_uint4(nw[4 * c], nw[4 * c + 1], nw[4 * c + 2], nw[4 * c + 3]);
  }
  int msz;
  uint32_t cls;
  block_class_msz(R, msz, cls);
  rmask[g] = (uint8_t)m;
  binfo[g] = binfo_word(m, (uint32_t)msz, cls, nw[0] & 0xFFFFu);
}

// ---- compare --------------------------------------------------------------
//
// k_decode_compare: the fused decoder with a reference frame where
// k_decode_idct has its output (include/myyuv_hip.h, "Compare").  Grid, decode,
// DC-only shortcut and transform units are k_decode_idct's, decode_group
// unchanged, so a malformed stream gives the full decode's code and block.
// Where k_decode_idct stores a pixel row at block_row_offset(...), this kernel
// has loaded the reference frame's row from the same offset (issued before the
// unit's transform, which hides the latency) and adds the row's part of the
// block's sums (metric.h).  A block's rows sit in 4 lanes of a 16-block unit,
// in 8 lanes of an 8-block unit (mt::fold_lanes) and in one lane for a
// DC-only block; one of them leaves the block's six sums in LDS at the block's
// lane of the group (component-major, at the end of the value-position table,
// dead after decode_group).  After the last unit lane l takes block l's sums and
// the wave finishes as k_frame_compare does (mt::finish): the 24-step quotient
// runs once per group, every lane busy, and the group's totals go to its slot
// of `part` for k_metric_reduce (k_color.hip).  The decoded frame never exists
// in HBM.  ref_fbytes: G.fbytes, or 0 when every frame is compared with one
// reference frame.
__global__ __launch_bounds__(64, MYYUV_K5_WAVES) void k_decode_compare(const uint8_t* __restrict__ in,
                                                      const uint32_t* __restrict__ in_size,
                                                      uint32_t cap,
                                                      const StreamDesc* __restrict__ desc,
                                                      const uint32_t* __restrict__ local_off,
                                                      const uint32_t* __restrict__ tile_pre,
                                                      FrameGeom G, uint32_t tiles_p0,
                                                      uint32_t tiles_p1, const QTables* __restrict__ qt,
                                                      uint4* __restrict__ coef,
                                                      const uint8_t* __restrict__ ref, uint32_t ref_fbytes,
                                                      uint4* __restrict__ part,
                                                      myyuv_block_metric* __restrict__ map,
                                                      unsigned long long* __restrict__ err) {
  static_assert(sizeof(uint4) * kStageQuads >= sizeof(float) * xf::kXfTile16, "the tile over the stage");
  __shared__ uint4 stq[kStageQuads + 1 + kGposQuads];
  __shared__ float sq[64];
  __shared__ uint16_t s_blk[64];
  const uint32_t lane = threadIdx.x;
  if (lane == 0) stq[kStageQuads] = make_uint4(0u, 0u, 0u, 0u);  // (ordered by decode_group's barrier)
  {
    // the plane's Q table by LDS-DMA (landed by decode_group's final vmcnt wait)
    const uint32_t t = blockIdx.x;
    const int p = t >= tiles_p0 ? (t >= tiles_p0 + tiles_p1 ? 2 : 1) : 0;
    __builtin_amdgcn_global_load_lds((const void*)&qt->q[p][lane], (__attribute__((address_space(3))) void*)sq, 4,
                                     0, 0);
  }
  DecodeGroup D;
  uint32_t nw[32];
#pragma unroll
  for (int w = 0; w < 32; w++) nw[w] = 0;
  bool direct;
  if (!decode_group(in, in_size, cap, desc, local_off, tile_pre, G, tiles_p0, tiles_p1, coef, err, stq, D, nw,
                    direct)) {
    // the frame's stream header is bad (k_scan_chain recorded it): the wave adds nothing
    if (lane == 0) *mt::wave_slot(part) = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  if (D.live && direct) {  // decode_general wrote the block to coef (a table the reference never writes)
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const uint4 v = coef[coef_quad(D.gbase + D.g, c)];
      nw[4 * c] = v.x;
      nw[4 * c + 1] = v.y;
      nw[4 * c + 2] = v.z;
      nw[4 * c + 3] = v.w;
    }
  }
  const int p = D.p;
  xf::Unit U;
  U.p = p;
  U.cum = G.cum[p];
  U.nb = G.cum[p + 1] - G.cum[p];
  U.poff = p == 0 ? G.poff[0] : (p == 1 ? G.poff[1] : G.poff[2]);
  U.pw = p == 0 ? G.pw[0] : (p == 1 ? G.pw[1] : G.pw[2]);
  U.bw = p == 0 ? G.bw[0] : (p == 1 ? G.bw[1] : G.bw[2]);
  U.bmag = p == 0 ? G.bmag[0] : (p == 1 ? G.bmag[1] : G.bmag[2]);
  U.local0 = 0;
  const uint8_t* fr = ref + (size_t)D.f * ref_fbytes;
  // LDS after the decode: the transpose tile over the stage (4608 B), then the
  // unit's reference rows (xl: 4 words per lane, word m of lane l at
  // xl[64 m + l], 1 KiB over the stage's end, the zero quad and the start of
  // the value-position table), then the blocks' sums at the table's end
  // (block l's component c at gs[64 c + l])
  constexpr uint32_t kSumWords = 6 * 64, kRefWords = 4 * 64;
  constexpr uint32_t kLdsWords = (kStageQuads + 1 + kGposQuads) * 4;
  static_assert(xf::kXfTile16 + kRefWords + kSumWords <= kLdsWords, "tile, reference rows and sums");
  uint32_t* xl = reinterpret_cast<uint32_t*>(stq) + xf::kXfTile16;
  uint32_t* gs = reinterpret_cast<uint32_t*>(stq) + (kLdsWords - kSumWords);
  auto put_sums = [gs](uint32_t l, const mt::Sums& s) {
    gs[l] = s.sx;
    gs[64 + l] = s.sy;
    gs[128 + l] = s.sxx;
    gs[192 + l] = s.syy;
    gs[256 + l] = s.sxy;
    gs[320 + l] = s.mx;
  };
  uint32_t acc = nw[0] & 0xFFFF0000u;
#pragma unroll
  for (int w = 1; w < 32; w++) acc |= nw[w];
  const bool isdc = D.live && acc == 0u;
  if (isdc) {  // the DC-only constant block (see k_decode_idct), against the block's 8 reference rows
    uint2 rr[8];
#pragma unroll
    for (uint32_t r = 0; r < 8; r++)
      rr[r] = *reinterpret_cast<const uint2*>(fr + xf::block_row_offset(U, D.g - U.cum, r));
    constexpr float c0 = xf::c_dct[0];
    const float z = (float)(int16_t)nw[0] * sq[0];  // dequantise (DCT.cpp:331)
    const float u = 0.0f + c0 * z;                  // stage 1: the k = 0 term
    float S = 0.0f + u * c0;                        // stage 2: the k = 0 term
    S = __builtin_amdgcn_fmed3f(S, -128.0f, 127.0f);  // (as idct_rows, DCT.cpp:358-362)
    uint32_t px = xf::bits(S + xf::kMagicPx);
    if (__builtin_amdgcn_fractf(S) == 0.5f)
      px = (uint32_t)((int)__builtin_truncf(S + __builtin_copysignf(xf::kHalfDown, S)) + 128);
    const uint32_t v4 = (px & 0xFFu) * 0x01010101u;
    mt::Sums s;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      myyuv_metric::add_word(s, rr[r].x, v4);
      myyuv_metric::add_word(s, rr[r].y, v4);
    }
    put_sums(lane, s);
  }
  const uint64_t rest = __ballot(D.live && !isdc);
  const uint32_t nrest = (uint32_t)__popcll(rest);
  const uint32_t rrank = __builtin_amdgcn_mbcnt_hi((uint32_t)(rest >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rest, 0u));
  if (D.live && !isdc) s_blk[rrank] = (uint16_t)lane;  // compacted position -> the block's lane in the group
  xf::wave_sync();  // (s_blk is read at the top of the first unit)
  float* tile = reinterpret_cast<float*>(stq);
#pragma unroll 1
  for (uint32_t base = 0; base < nrest;) {
    const bool wide = nrest - base > 8u;
    const uint32_t span = wide ? 16u : 8u, stride = wide ? (uint32_t)xf::kTile : (uint32_t)xf::kTile8;
    // the unit's reference rows, issued before its transform by LDS-DMA (they
    // hold no register while it runs; the kernel sits at the register budget
    // of its five waves per SIMD): lane (b, q) rows 2q, 2q + 1 of block b, or
    // lane (b, r) row r.  Slots past the last block read the last block's.
    const uint32_t ub = wide ? lane >> 2 : lane >> 3;
    const uint32_t ur = wide ? 2u * (lane & 3u) : lane & 7u;
    {
      const uint32_t ul = s_blk[min(base + ub, nrest - 1u)];  // the block's lane in the group
      const uint8_t* src = fr + xf::block_row_offset(U, D.g0 + ul - U.cum, ur);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the last unit's reads of xl)
      __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)xl, 4, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(src + 4), (__attribute__((address_space(3))) void*)(xl + 64), 4,
                                       0, 0);
      if (wide) {
        __builtin_amdgcn_global_load_lds((const void*)(src + U.pw),
                                         (__attribute__((address_space(3))) void*)(xl + 128), 4, 0, 0);
        __builtin_amdgcn_global_load_lds((const void*)(src + U.pw + 4),
                                         (__attribute__((address_space(3))) void*)(xl + 192), 4, 0, 0);
      }
    }
    const uint32_t s = rrank - base;
    if (D.live && !isdc && rrank >= base && s < span) {
      uint4* img = reinterpret_cast<uint4*>(tile + s * stride + (wide ? xf::img_word(s) : 0u));
#pragma unroll
      for (int c = 0; c < 8; c++) img[c] = make_uint4(nw[4 * c], nw[4 * c + 1], nw[4 * c + 2], nw[4 * c + 3]);
    }
    if (lane < span && base + lane >= nrest) {
      uint4* img = reinterpret_cast<uint4*>(tile + lane * stride + (wide ? xf::img_word(lane) : 0u));
#pragma unroll
      for (int c = 0; c < 8; c++) img[c] = make_uint4(0u, 0u, 0u, 0u);
    }
    xf::wave_sync();
    mt::Sums ps;
    if (wide) {
      const uint32_t q = lane & 3u, b = lane >> 2;
      uint2 w0, w1;
      xf::idct_rows(tile + b * xf::kTile, q, b, sq, w0, w1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the reference rows are in xl
      myyuv_metric::add_word(ps, xl[lane], w0.x);
      myyuv_metric::add_word(ps, xl[64 + lane], w0.y);
      myyuv_metric::add_word(ps, xl[128 + lane], w1.x);
      myyuv_metric::add_word(ps, xl[192 + lane], w1.y);
      mt::fold_lanes<4>(ps);
      if (q == 0u && base + b < nrest) put_sums(s_blk[base + b], ps);
    } else {
      const uint32_t r = lane & 7u, b = lane >> 3;
      float qc[8];  // the lane's column of the plane's Q table, Q[k][r]
#pragma unroll
      for (int k = 0; k < 8; k++) qc[k] = sq[8 * k + r];
      const uint2 w = xf::idct_row8(tile + b * xf::kTile8, r, qc);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the reference rows are in xl
      myyuv_metric::add_word(ps, xl[lane], w.x);
      myyuv_metric::add_word(ps, xl[64 + lane], w.y);
      mt::fold_lanes<8>(ps);
      if (r == 0u && base + b < nrest) put_sums(s_blk[base + b], ps);
    }
    xf::wave_sync();  // the next unit rewrites the tile
    base += span;
  }
  xf::wave_sync();  // the blocks' sums, from the lanes that left them to the blocks' own lanes
  mt::Sums bs;
  bs.sx = gs[lane];
  bs.sy = gs[64 + lane];
  bs.sxx = gs[128 + lane];
  bs.syy = gs[192 + lane];
  bs.sxy = gs[256 + lane];
  bs.mx = gs[320 + lane];
  // (the block's index built again from the lane: the 64-bit index of the
  // coefficient buffer would otherwise stay live, one register pair too many,
  // from the decode to here)
  uint32_t gl = lane;
  asm volatile("" : "+v"(gl));
  mt::finish(bs, D.live, mt::wave_slot(part), map != nullptr ? map + (D.gbase + D.g0 + gl) : nullptr);
}

// ---- export to JPEG -------------------------------------------------------
//
// k_jpeg_export: a stream's blocks written as the restart intervals of a
// baseline JPEG (include/myyuv_hip.h, "Export to JPEG"; the code of a block is
// jpeg_export.h's).  Grid and decode are k_requant's: one wave per 64-block
// group (blockIdx.x) of frame blockIdx.y, decode_group unchanged, a block with
// a table that is not "regular" read back from the coefficient buffer.  A
// group is one plane's consecutive blocks, which is one restart interval of
// that plane's non-interleaved scan, so the wave owns the interval:
//   1. lane l's DC prediction is lane l - 1's DC (0 for lane 0);
//   2. every lane counts its block's bits (jp::BitCount), the wave scans them,
//      and the last live lane adds the 1-bits that fill the last byte;
//   3. the lanes write their blocks' bits at their offsets into an LDS bit
//      image laid over the chunk stage and the value-position table, both dead
//      after the decode: a 64-bit accumulator per lane, flushed word by word
//      with ds_or (a word is shared by neighbouring blocks).  Words hold the
//      stream's bytes most significant first;
//   4. the wave reads the image 256 bytes at a time, counts each lane's 0xFF
//      bytes, scans the counts and (Write) stores the bytes with a 0x00 after
//      every 0xFF at the interval's place in the file.
// The image holds kJpegImgWords words (7,168 B, about 112 B per block; a
// natural picture needs 1-2 KB per group).  A longer interval (up to 13,280 B
// when every coefficient is +-1023) takes several rounds of steps 3 and 4 over
// consecutive windows of the interval's bits: a lane encodes its block again
// in every round whose window its bits touch, and the sink drops the words
// outside the window.
//
// Every live lane contributes a block, whatever the stream holds: a lane whose
// chunk failed, and every lane of a frame whose header k_scan_chain rejected,
// contributes the all-zero block (k_requant's rule); the error itself is in
// the shared error word.
//
// Write = false: the sizing launch; gbuf[group] = the interval's stuffed bytes.
// k_jpeg_place then turns the sizes into file offsets (the scan headers, the
// RST markers and EOI fall between the intervals).  Write = true: the same
// work again, the bytes stored at out + f * cap_out + goff[group], at most
// gbuf[group] of them, and nothing for a frame whose file exceeds cap_out.
// No buffer scales with the worst case: the scratch is two words per group.
namespace jp = myyuv_jpeg;

__device__ const jp::CodeTables d_jpeg_tab[2] = {jp::kLumTables, jp::kChrTables};

constexpr uint32_t kJpegImgWords = ((kStageQuads + 1 + kGposQuads) * 4) & ~63u;
constexpr uint32_t kJpegImgBits = kJpegImgWords * 32;
static_assert(kJpegImgWords * 4 <= sizeof(uint4) * (kStageQuads + 1 + kGposQuads), "the image over the stage");
static_assert(kJpegImgBits >= 2 * jp::kMaxBlockBits, "a block touches at most two windows");

struct JpegLdsTab {
  const uint32_t* t;
  __device__ __forceinline__ uint32_t dc(uint32_t cat) const { return t[256 + cat]; }
  __device__ __forceinline__ uint32_t ac(uint32_t sym) const { return t[sym]; }
};

// Bits into the LDS image from bit `pos` of the interval on; w0: the window's
// first word.  The first word starts with pos & 31 zero bits (a neighbour's).
struct JpegLdsSink {
  uint32_t* img;
  uint32_t w0;
  uint64_t acc;
  uint32_t n, wi;
  __device__ __forceinline__ JpegLdsSink(uint32_t* image, uint32_t first_word, uint32_t pos)
      : img(image), w0(first_word), acc(0), n(pos & 31u), wi(pos >> 5) {}
  __device__ __forceinline__ void flush(uint32_t word) {
    const uint32_t k = wi - w0;  // (below the window: wraps past it)
    if (k < kJpegImgWords) atomicOr(&img[k], word);
    wi++;
  }
  __device__ __forceinline__ void put(uint32_t bits, uint32_t count) {
    acc = (acc << count) | bits;
    n += count;
    if (n >= 32) {
      n -= 32;
      flush((uint32_t)(acc >> n));
      acc &= (1ull << n) - 1ull;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n) flush((uint32_t)acc << (32 - n));
  }
};

#ifndef MYYUV_JPEG_WAVES
// waves per SIMD of the register budget (the LDS allows 4.75): the 8192x8192 q50 export took 470 / 389 / 426 /
// 558 us at 2 / 3 / 4 / 5 (184 VGPRs and no spill at 2; 16 / 69 / 121 spilled registers at 3 / 4 / 5)
#define MYYUV_JPEG_WAVES 3
#endif
template <bool Write>
__global__ __launch_bounds__(64, MYYUV_JPEG_WAVES) void k_jpeg_export(const uint8_t* __restrict__ in,
                                                   const uint32_t* __restrict__ in_size,
                                                   uint32_t cap,
                                                   const StreamDesc* __restrict__ desc,
                                                   const uint32_t* __restrict__ local_off,
                                                   const uint32_t* __restrict__ tile_pre,
                                                   FrameGeom G, uint32_t tiles_p0,
                                                   uint32_t tiles_p1, uint4* __restrict__ coef,
                                                   uint32_t* __restrict__ gbuf,
                                                   const uint32_t* __restrict__ goff,
                                                   const uint32_t* __restrict__ out_sizes,
                                                   uint8_t* __restrict__ out, uint32_t cap_out,
                                                   unsigned long long* __restrict__ err) {
  __shared__ uint4 stq[kStageQuads + 1 + kGposQuads];
  __shared__ uint32_t stab[jp::kTabWords];
  const uint32_t lane = threadIdx.x;
  if (lane == 0) stq[kStageQuads] = make_uint4(0u, 0u, 0u, 0u);  // (ordered by decode_group's barrier)
  {
    // the plane's code tables (visible after the barrier that follows the decode)
    const uint32_t t = blockIdx.x;
    const uint32_t* src = d_jpeg_tab[t >= tiles_p0 ? 1 : 0].e;
    for (uint32_t k = lane; k < jp::kTabWords; k += kWave) stab[k] = src[k];
  }
  DecodeGroup D;
  uint32_t nw[32];
#pragma unroll
  for (int w = 0; w < 32; w++) nw[w] = 0;
  bool direct;
  const bool frame_ok = decode_group(in, in_size, cap, desc, local_off, tile_pre, G, tiles_p0, tiles_p1, coef, err,
                                     stq, D, nw, direct);
  const bool keep = frame_ok && D.live && D.good;
  if (keep && direct) {  // decode_general wrote the block to coef (a table the reference never writes)
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const uint4 v = coef[coef_quad(D.gbase + D.g, c)];
      nw[4 * c] = v.x;
      nw[4 * c + 1] = v.y;
      nw[4 * c + 2] = v.z;
      nw[4 * c + 3] = v.w;
    }
  }
#pragma unroll
  for (int w = 0; w < 32; w++) nw[w] = keep ? nw[w] : 0u;
  __syncthreads();  // the decode's LDS reads are done, the tables are in place

  const uint32_t nlive = D.g1 - D.g0;
  const bool last = lane + 1 == nlive;
  const int dc = (int)(int16_t)(nw[0] & 0xFFFFu);
  const int up = __shfl_up(dc, 1, kWave);
  const int pred = lane == 0 ? 0 : up;
  auto cf = [&nw](int k) {
    const int n = jp::kZigzag[k];
    const uint32_t w = nw[n >> 1];
    return (int)(int16_t)((n & 1) ? (w >> 16) : (w & 0xFFFFu));
  };
  const JpegLdsTab tab{stab};
  jp::BitCount cnt;
  jp::encode_block(cf, pred, tab, cnt);
  const uint32_t nbits = D.live ? cnt.n : 0u;
  const uint32_t incl = wave_incl_scan(nbits);
  const uint32_t pos = incl - nbits;
  const uint32_t tbits = (uint32_t)__shfl((int)incl, kWave - 1, kWave);
  const uint32_t pad = (0u - tbits) & 7u;
  const uint32_t T = tbits + pad;  // a multiple of 8, at least 8

  const uint32_t ntg = gridDim.x;
  const uint32_t gi = D.f * ntg + blockIdx.x;
  uint32_t* img = reinterpret_cast<uint32_t*>(stq);
  uint8_t* q = nullptr;
  const uint8_t* qend = nullptr;
  if (Write) {
    const uint32_t total = out_sizes[D.f];
    if (total <= cap_out) {
      const uint32_t o = goff[gi];
      const uint32_t sz = min(gbuf[gi], total - min(o, total));
      q = out + (size_t)D.f * cap_out + o;
      qend = q + sz;
      // what stands in front of the interval (k_jpeg_place left room for it,
      // after the file header: o >= kHeaderBytes + kSosBytes): the plane's
      // scan header, or RSTm with m counted within the plane
      const uint32_t t = blockIdx.x;
      const uint32_t tp = t - (D.p == 0 ? 0u : (D.p == 1 ? tiles_p0 : tiles_p0 + tiles_p1));
      if (lane == 0 && o >= jp::kHeaderBytes + jp::kSosBytes && o <= total) {
        if (tp == 0) {
          jp::write_sos(q - jp::kSosBytes, (uint32_t)D.p);
        } else {
          q[-2] = 0xFF;
          q[-1] = (uint8_t)(0xD0u + ((tp - 1u) & 7u));
        }
      }
    }
  }
  uint32_t nff = 0;  // the 0xFF bytes of the windows so far
  for (uint32_t b0 = 0; b0 < T; b0 += kJpegImgBits) {
    const uint32_t wbits = min(T - b0, kJpegImgBits);
    for (uint32_t k = lane; k < (wbits + 31) >> 5; k += kWave) img[k] = 0u;
    __syncthreads();
    const uint32_t end = pos + nbits + (last ? pad : 0u);
    if (D.live && end > b0 && pos < b0 + wbits) {
      JpegLdsSink sink(img, b0 >> 5, pos);
      jp::encode_block(cf, pred, tab, sink);
      if (last && pad) sink.put((1u << pad) - 1u, pad);
      sink.finish();
    }
    __syncthreads();
    const uint32_t wbytes = wbits >> 3;
    for (uint32_t j0 = 0; j0 < wbytes; j0 += 4 * kWave) {
      const uint32_t j = j0 + 4 * lane;
      const uint32_t nb = j < wbytes ? min(4u, wbytes - j) : 0u;
      const uint32_t word = nb ? img[j >> 2] : 0u;
      uint32_t ff = 0;
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) ff += (k < nb && ((word >> (24 - 8 * k)) & 0xFFu) == 0xFFu) ? 1u : 0u;
      const uint32_t fincl = wave_incl_scan(ff);
      if (Write && q != nullptr) {
        uint8_t* o = q + ((b0 >> 3) + j + nff + fincl - ff);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
          const uint32_t b = (word >> (24 - 8 * k)) & 0xFFu;
          if (k < nb) {
            if (o < qend) *o = (uint8_t)b;
            o++;
            if (b == 0xFFu) {
              if (o < qend) *o = 0;
              o++;
            }
          }
        }
      }
      nff += (uint32_t)__shfl((int)fincl, kWave - 1, kWave);
    }
    __syncthreads();  // the image is zeroed again
  }
  if (!Write && lane == 0) gbuf[gi] = (T >> 3) + nff;
}
template __global__ void k_jpeg_export<false>(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*,
                                              const uint32_t*, const uint32_t*, FrameGeom, uint32_t, uint32_t, uint4*,
                                              uint32_t*, const uint32_t*, const uint32_t*, uint8_t*, uint32_t,
                                              unsigned long long*);
template __global__ void k_jpeg_export<true>(const uint8_t*, const uint32_t*, uint32_t, const StreamDesc*,
                                             const uint32_t*, const uint32_t*, FrameGeom, uint32_t, uint32_t, uint4*,
                                             uint32_t*, const uint32_t*, const uint32_t*, uint8_t*, uint32_t,
                                             unsigned long long*);

// k_jpeg_place: one workgroup per frame turns the groups' interval sizes into
// file offsets and writes the file header and EOI.  In front of group t's
// interval stands its plane's scan header (the plane's first group) or the
// marker RSTm, m = (t - 1) mod 8 counted within the plane: the placement
// leaves room for them, the writing launch's waves write them with their
// intervals.  goff[t]: the file offset of the interval's first
// byte; out_sizes[f]: the file's size (0xFFFFFFFF when it does not fit 32
// bits).  A file beyond cap_out is MYYUV_E_CAPACITY (no block) and nothing of
// it is written; out == nullptr: sizes and offsets only.
__global__ __launch_bounds__(256) void k_jpeg_place(const uint32_t* __restrict__ gsize, uint32_t* __restrict__ goff,
                                                    uint32_t t0, uint32_t t1, uint32_t t2, jp::Head H,
                                                    uint8_t* __restrict__ out, uint32_t cap_out,
                                                    uint32_t* __restrict__ out_sizes,
                                                    unsigned long long* __restrict__ err) {
  // kPer consecutive groups per thread and round: a thread's own sum (below
  // 2^32: at most 16 x 26.6 KB), the wave's scan by DPP, the four waves'
  // totals through LDS; the running offset in 64 bits
  constexpr uint32_t kPer = 16;
  __shared__ uint32_t wsum[4];
  const uint32_t f = blockIdx.x, tid = threadIdx.x, ntg = t0 + t1 + t2;
  gsize += (size_t)f * ntg;
  goff += (size_t)f * ntg;
  unsigned long long run = jp::kHeaderBytes;
  for (uint32_t base = 0; base < ntg; base += 256 * kPer) {
    const uint32_t tb = base + tid * kPer;
    uint32_t v[kPer], own = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPer; i++) {
      const uint32_t t = tb + i;
      const bool first = t == 0 || t == t0 || t == t0 + t1;
      v[i] = t < ntg ? gsize[t] : 0u;
      own += t < ntg ? v[i] + (first ? jp::kSosBytes : 2u) : 0u;
    }
    const uint32_t incl = wave_incl_scan(own);
    if ((tid & 63u) == 63u) wsum[tid >> 6] = incl;
    __syncthreads();
    unsigned long long at = run + (incl - own);  // the end of the interval before this thread's first
    unsigned long long all = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      at += k < (tid >> 6) ? wsum[k] : 0u;
      all += wsum[k];
    }
#pragma unroll
    for (uint32_t i = 0; i < kPer; i++) {
      const uint32_t t = tb + i;
      const bool first = t == 0 || t == t0 || t == t0 + t1;
      at += first ? jp::kSosBytes : 2u;  // the scan header or the marker in front of the interval
      if (t < ntg) goff[t] = (uint32_t)min(at, 0xFFFFFFFFull);
      at += v[i];
    }
    run += all;
    __syncthreads();  // (wsum is written again)
  }
  const unsigned long long total = run + 2;
  if (tid == 0) {
    out_sizes[f] = (uint32_t)min(total, 0xFFFFFFFFull);
    if (total > cap_out) record_error(err, 0, 5 /* MYYUV_E_CAPACITY, any frame */);
  }
  if (out == nullptr || total > cap_out) return;
  out += (size_t)f * cap_out;
  for (uint32_t k = tid; k < jp::kHeaderBytes; k += 256) out[k] = H.b[k];
  if (tid == 0) {
    out[total - 2] = 0xFF;
    out[total - 1] = 0xD9;
  }
}

}  // namespace myyuv_gpu

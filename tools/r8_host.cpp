// Host harness (test infrastructure): runs K2's register-resident encoders
// (huff_common.hpp, compiled for the host) on blocks read from stdin and
// writes the chunks to stdout, for tests/test_r8_host.py to compare with the
// oracle.  argv[1]: "4" / "8" = build_r<CAP> + emit_chunk on every block;
// "auto" = the kernel's class dispatch (block_class); "dense" = "auto" packed
// the way k_huff_encode packs a tile (DenseWriter); "16" = build_r16 +
// emit_chunk16 (the CAP-16 overflow tier, huff_r16.hpp); "single" = the
// single-class marker's closed form against build_single_dc + emit_chunk
// (check_single: no input).
//   in: u32 n, then n x 64 int16 coefficients in natural order
//   out: per block u8 ok, u8 size, then `size` chunk bytes (ok = 1);
//        "dense": u32 run bytes, then the run
#include <cstdio>
#include <cstring>
#include <vector>

#include "huff_common.hpp"
#include "huff_r16.hpp"

using namespace myyuv_gpu;

// Host writer with the put / align_byte interface emit_chunk expects.
struct HostWriter {
  uint8_t* out;
  uint64_t acc = 0;
  int nacc = 0;
  int pos = 0;
  void put(uint32_t v, int n) {
    acc |= (uint64_t)v << nacc;
    nacc += n;
    while (nacc >= 8) {
      out[pos++] = (uint8_t)acc;
      acc >>= 8;
      nacc -= 8;
    }
  }
  void align_byte() {
    if (nacc > 0) put(0, 8 - nacc);
  }
};

static bool build(const CoefRegs& R, const char* mode, EncState& S) {
  const int msz = R.msz();
  if (mode[0] == '4') return build_r<4>(R, msz, 64, S);
  if (mode[0] == '8') return build_r<8>(R, msz, 64, S);
  const uint32_t cls = block_class(R, msz);
  if (cls == kClassOvf) return false;  // straight to the overflow worklist
  if (cls == kClassSingle) {
    build_single(R, S);
    return true;
  }
  return cls == kClassR4 ? build_r<4>(R, msz, 64, S) : build_r<8>(R, msz, 64, S);
}

// "single": the K2 -> K4 marker of a single-class block (codec_common.hpp
// single_chunk_words) against the encoder it stands for: for every 11-bit
// key as a sign-extended DC coefficient, and for the all-zero block, the two
// source words must be the 7 bytes emit_chunk(build_single_dc) writes, zeros
// after.  Reads nothing; prints the number of cases checked.
static int check_single() {
  uint32_t checked = 0;
  for (int c = -1; c < 2048; c++) {  // (-1: the all-zero block through build_single)
    const int dc = c < 0 ? 0 : (c >= 1024 ? c - 2048 : c);
    EncState S;
    if (c < 0) {
      CoefRegs R;
      for (int w = 0; w < 32; w++) R.w[w] = 0u;
      if (R.msz() != 0 || block_class(R, 0) != kClassSingle) return 4;
      build_single(R, S);
    } else {
      build_single_dc(dc, S);
    }
    uint8_t want[8] = {0};
    HostWriter hw{want};
    emit_chunk(S, 1, hw);
    hw.align_byte();
    if (hw.pos != (int)kSingleChunk || S.size != kSingleChunk) return 3;
    const uint32_t so = kSrcSingle | ((uint32_t)dc & 0x7FFu);
    if (!src_is_single(so) || so == kSrcOverflow) return 5;
    uint32_t w[2];
    single_chunk_words(so, w[0], w[1]);
    if (std::memcmp(w, want, 8) != 0) {
      fprintf(stderr, "single: key %d: words %08x %08x\n", c, w[0], w[1]);
      return 1;
    }
    checked++;
  }
  // a stage offset and the overflow mark are no markers
  if (src_is_single(0u) || src_is_single(kWinTilesBig * kTileCap - 1u) || src_is_single(kSrcOverflow)) return 5;
  printf("%u\n", checked);
  return 0;
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "auto";
  if (mode[0] == 's') return check_single();
  uint32_t n = 0;
  if (fread(&n, 4, 1, stdin) != 1) return 2;
  std::vector<int16_t> c((size_t)n * 64);
  if (fread(c.data(), 2, c.size(), stdin) != c.size()) return 2;
  std::vector<EncState> st(n);
  std::vector<uint8_t> ok(n);
  for (uint32_t b = 0; b < n; b++) {
    CoefRegs R;
    for (int w = 0; w < 32; w++)
      R.w[w] = (uint16_t)c[b * 64 + 2 * w] | ((uint32_t)(uint16_t)c[b * 64 + 2 * w + 1] << 16);
    ok[b] = build(R, mode[0] == 'd' ? "auto" : mode, st[b]);
  }
  if (mode[0] == '1') {  // "16": the CAP-16 tier
    for (uint32_t b = 0; b < n; b++) {
      CoefRegs R;
      for (int w = 0; w < 32; w++)
        R.w[w] = (uint16_t)c[b * 64 + 2 * w] | ((uint32_t)(uint16_t)c[b * 64 + 2 * w + 1] << 16);
      EncState16 S16;
      uint32_t col[16] = {0};  // "16l": the kernel's LDS-column heap over a local column
      const bool ok16 = mode[2] == 'l' ? build_r16(R, R.msz(), 64, S16, r16::LdsHeap16<1>{col})
                                       : build_r16(R, R.msz(), 64, S16);
      const uint8_t hdr[2] = {(uint8_t)ok16, ok16 ? (uint8_t)S16.size : (uint8_t)0};
      fwrite(hdr, 1, 2, stdout);
      if (ok16) {
        uint8_t bytes[kMaxChunk] = {0};
        HostWriter hw{bytes};
        emit_chunk16(S16, 64, hw);
        hw.align_byte();
        if (hw.pos != (int)S16.size) return 3;
        fwrite(bytes, 1, S16.size, stdout);
      }
    }
    return 0;
  }
  if (mode[0] == 'd') {
    // "dense": K2's tile run — the accepted blocks' chunks back to back in
    // block order, each written by DenseWriter at its offset with the next
    // accepted chunk's header; out: u32 run bytes, the run
    std::vector<uint32_t> off(n + 1, 0);
    for (uint32_t b = 0; b < n; b++) off[b + 1] = off[b] + (ok[b] ? st[b].size : 0);
    std::vector<uint32_t> run(off[n] / 4 + 2, 0xA5A5A5A5u);  // canary: every dword must be stored
    for (uint32_t b = 0; b < n; b++) {
      if (!ok[b]) continue;
      uint32_t next = 0;
      for (uint32_t k = b + 1; k < n; k++)
        if (ok[k]) {
          next = st[k].hdr | 0x80000000u;
          break;
        }
      DenseWriter dw;
      dw.init(run.data(), off[b]);
      emit_chunk(st[b], 64, dw);
      dw.finish(next);
    }
    const uint32_t total = off[n];
    fwrite(&total, 4, 1, stdout);
    fwrite(run.data(), 1, total, stdout);
    return 0;
  }
  for (uint32_t b = 0; b < n; b++) {
    const uint8_t hdr[2] = {ok[b], ok[b] ? (uint8_t)st[b].size : (uint8_t)0};
    fwrite(hdr, 1, 2, stdout);
    if (ok[b]) {
      uint8_t bytes[kMaxChunk] = {0};
      HostWriter hw{bytes};
      emit_chunk(st[b], 64, hw);
      hw.align_byte();
      if (hw.pos != (int)st[b].size) return 3;
      fwrite(bytes, 1, st[b].size, stdout);
    }
  }
  return 0;
}

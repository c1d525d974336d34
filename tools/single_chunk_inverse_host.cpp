// single_chunk_inverse_host.cpp — host check of codec_common.hpp's
// single_chunk_key, the span decoder's closed-form test, against
// single_chunk_words, the encoder side's closed form:
//   * for every 11-bit key, the 7 bytes of single_chunk_words are recognised
//     and give the key back;
//   * every 7-byte string one bit, or one byte (all 255 other values), away
//     from such a chunk is recognised exactly when it is itself the closed
//     form of some key (a change inside the key's 11 bits), decided here by
//     comparing with all 2,048 closed forms;
//   * the chunks a span decoder must not take for it: messages of 2..8
//     positions, an empty table, a longer table.
// Prints the number of strings checked; exit status 0 when all agree.
// Stand-alone (its own main), built plainly and with ASan + UBSan by
// tests/test_single_chunk_inverse_host.py.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "codec_common.hpp"

using namespace myyuv_gpu;

static void closed_form(uint32_t key, uint8_t out[7]) {
  uint32_t w[2];
  single_chunk_words(kSrcSingle | key, w[0], w[1]);
  uint8_t b[8];
  std::memcpy(b, w, 8);
  std::memcpy(out, b, 7);
}

// the predicate as the kernel applies it: bytes 0..3 and bytes 3..6
static bool recognised(const uint8_t c[7], uint32_t& key) {
  uint32_t h, t;
  std::memcpy(&h, c, 4);
  std::memcpy(&t, c + 3, 4);
  return single_chunk_key(h, t, key);
}

static uint8_t g_all[2048][7];

// The key whose closed form c is, or -1.  Bytes 4 and 5 of key k's closed
// form hold k (main checks it for every key), so only the entry of c's own
// bytes 4 and 5 can be equal to c.
static int by_search(const uint8_t c[7]) {
  const int k = (c[4] | (c[5] << 8)) & 0x7FF;
  return std::memcmp(g_all[k], c, 7) == 0 ? k : -1;
}

static long g_checked = 0;

static bool agree(const uint8_t c[7]) {
  uint32_t key = 0;
  const bool got = recognised(c, key);
  const int want = by_search(c);
  g_checked++;
  if (got != (want >= 0) || (got && (int)key != want)) {
    std::fprintf(stderr, "%02x %02x %02x %02x %02x %02x %02x: predicate %d key %u, search %d\n", c[0], c[1], c[2],
                 c[3], c[4], c[5], c[6], (int)got, key, want);
    return false;
  }
  return true;
}

int main() {
  for (uint32_t k = 0; k < 2048; k++) {
    closed_form(k, g_all[k]);
    // the word w1 beyond the 7 bytes is zero too (K4 copies whole words)
    uint32_t w0, w1;
    single_chunk_words(k, w0, w1);
    if (w1 >> 24) return 2;
    if ((uint32_t)(g_all[k][4] | (g_all[k][5] << 8)) != k) return 2;
  }
  for (uint32_t k = 0; k < 2048; k++) {
    uint32_t key = ~0u;
    if (!recognised(g_all[k], key) || key != k) return 3;
    if (!agree(g_all[k])) return 4;
    for (int bit = 0; bit < 56; bit++) {
      uint8_t c[7];
      std::memcpy(c, g_all[k], 7);
      c[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
      if (!agree(c)) return 5;
    }
    for (int byte = 0; byte < 7; byte++)
      for (int v = 0; v < 256; v++) {
        if (v == g_all[k][byte]) continue;
        uint8_t c[7];
        std::memcpy(c, g_all[k], 7);
        c[byte] = (uint8_t)v;
        if (!agree(c)) return 6;
      }
  }
  // 7-byte chunks that are no closed form: nbits 0 / 2..9, table bytes 0 / 4
  for (uint32_t k = 0; k < 2048; k += 37) {
    for (int nbits = 0; nbits <= 9; nbits++) {
      if (nbits == 1) continue;
      uint8_t c[7];
      std::memcpy(c, g_all[k], 7);
      c[0] = (uint8_t)nbits;
      uint32_t key;
      if (recognised(c, key) || !agree(c)) return 7;
    }
    for (int tb = 0; tb <= 4; tb += 4) {
      uint8_t c[7];
      std::memcpy(c, g_all[k], 7);
      c[2] = (uint8_t)tb;
      uint32_t key;
      if (recognised(c, key) || !agree(c)) return 8;
    }
  }
  std::printf("%ld\n", g_checked);
  return 0;
}

// rate_search_host.cpp — the search of "Encode to a target" (csrc/rate_search.h,
// the code the library's compress_to_* entry points run) driven from tables on
// the host, for tests/test_rate_search_host.py.  Plain C++; no HIP, no library.
//
// stdin (text):
//   size                 then 100 payload sizes (q = 1 .. 100)
//   sse                  then 300 squared errors (q = 1 .. 100, planes Y U V each)
//   psnr                 (no table)
//   N                    then N targets: a budget | three ceilings | dB nsamples
// stdout, one line per target:
//   size, sse:  <ok> <q0> <q1> <q2> <failed_planes> <probes> : <q q q> ; <q q q> ; ...
//   psnr:       <sse>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rate_search.h"

// myyuv_metric_psnr (myyuv_hip.cpp)
static double psnr(uint64_t sse, uint64_t nsamples) {
  if (sse == 0) return HUGE_VAL;
  return 10.0 * std::log10(65025.0 * (double)nsamples / (double)sse);
}

int main() {
  char mode[16] = {};
  if (std::scanf("%15s", mode) != 1) return 2;
  const bool is_size = !std::strcmp(mode, "size"), is_sse = !std::strcmp(mode, "sse");
  if (!is_size && !is_sse && std::strcmp(mode, "psnr")) return 2;
  std::vector<uint64_t> table(is_size ? 100 : (is_sse ? 300 : 0));
  for (auto& v : table)
    if (std::scanf("%" SCNu64, &v) != 1) return 2;
  unsigned n = 0;
  if (std::scanf("%u", &n) != 1) return 2;
  for (unsigned i = 0; i < n; i++) {
    if (!is_size && !is_sse) {
      char text[64];
      uint64_t ns;
      if (std::scanf("%63s %" SCNu64, text, &ns) != 2) return 2;
      std::printf("%" PRIu64 "\n", myyuv_rate::sse_for_psnr(std::strtod(text, nullptr), ns, psnr));
      continue;
    }
    uint64_t t[3] = {0, 0, 0};
    for (int p = 0; p < (is_size ? 1 : 3); p++)
      if (std::scanf("%" SCNu64, &t[p]) != 1) return 2;
    myyuv_rate::Search s = is_size ? myyuv_rate::Search::size(t[0]) : myyuv_rate::Search::sse(t);
    std::vector<uint8_t> asked;
    uint8_t q[3];
    while (s.next(q)) {
      asked.insert(asked.end(), q, q + 3);
      uint64_t sse[3] = {0, 0, 0};
      uint64_t bytes = 0;
      if (is_size)
        bytes = table[q[0] - 1];
      else
        for (int p = 0; p < 3; p++) sse[p] = table[(q[p] - 1) * 3 + p];
      s.answer(bytes, sse);
      if (asked.size() > 3 * 64) return 3;  // (a search that does not end)
    }
    std::printf("%d %u %u %u %u %u :", s.failed ? 0 : 1, s.quality[0], s.quality[1], s.quality[2], s.failed_planes,
                s.probes);
    for (size_t k = 0; k < asked.size(); k += 3)
      std::printf(" %u %u %u %s", asked[k], asked[k + 1], asked[k + 2], k + 3 < asked.size() ? ";" : "");
    std::printf("\n");
  }
  return 0;
}

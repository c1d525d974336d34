// rate_search.h — the search of "Encode to a target" (include/myyuv_hip.h): a
// state machine that, given the answers so far, names the next quality triple
// to probe or the result.  Plain C++, no HIP.  Included by the library
// (myyuv_hip.cpp, the compress_to_* entry points) and by the host program
// tools/rate_search_host.cpp (tests/test_rate_search_host.py), so the search
// under test is the library's own.
//
//   Search s = Search::size(budget)  or  Search::sse(max_sse);
//   uint8_t q[3];
//   while (s.next(q)) s.answer(<payload bytes at q>, <the three planes' sse at q>);
//   s.failed ? (s.failed_planes, s.quality = the failing probe) : s.quality
//
// Size mode reads only the size of an answer, distortion mode only the sse.
#pragma once
#include <stdint.h>

namespace myyuv_rate {

struct Search {
  bool size_mode = true;
  uint64_t budget = 0;             // size mode: payload bytes
  uint64_t max_sse[3] = {0, 0, 0}; // distortion mode
  // per plane (size mode: plane 0 stands for all three)
  uint8_t lo[3] = {1, 1, 1}, hi[3] = {100, 100, 100};
  bool fixed[3] = {false, false, false};  // the plane's result is known
  uint8_t quality[3] = {0, 0, 0};         // the result (or the failing probe)
  uint8_t asked[3] = {0, 0, 0};           // the probe next() named last
  uint32_t step = 0;                      // probes answered so far
  uint32_t probes = 0;                    // probes named so far
  bool done = false, failed = false;
  uint8_t failed_planes = 0;

  static Search size(uint64_t max_payload_bytes) {
    Search s;
    s.size_mode = true;
    s.budget = max_payload_bytes;
    return s;
  }
  static Search sse(const uint64_t max[3]) {
    Search s;
    s.size_mode = false;
    for (int p = 0; p < 3; p++) s.max_sse[p] = max[p];
    return s;
  }

  // The next probe into q; false when the search is over.
  bool next(uint8_t q[3]) {
    if (done) return false;
    for (int p = 0; p < 3; p++) {
      const int k = size_mode ? 0 : p;
      if (step == 0)
        asked[p] = 100;
      else if (step == 1)
        asked[p] = fixed[k] ? quality[k] : 1;
      else
        asked[p] = fixed[k] ? quality[k] : (uint8_t)((lo[k] + hi[k]) / 2);
      q[p] = asked[p];
    }
    probes++;
    return true;
  }

  // The answer to the probe next() named: the payload's bytes and the planes' sse.
  void answer(uint64_t payload_bytes, const uint64_t sse[3]) {
    const int planes = size_mode ? 1 : 3;
    if (step == 0) {
      if (size_mode) {
        if (payload_bytes <= budget) finish_plane(0, 100);
      } else {
        for (int p = 0; p < 3; p++)
          if (sse[p] > max_sse[p]) failed_planes |= (uint8_t)(1u << p);
        if (failed_planes) fail();
      }
    } else if (step == 1) {
      if (size_mode) {
        if (!fixed[0] && payload_bytes > budget) fail();
      } else {
        for (int p = 0; p < 3; p++)
          if (!fixed[p] && sse[p] <= max_sse[p]) finish_plane(p, 1);
      }
    } else {
      for (int k = 0; k < planes; k++) {
        if (fixed[k]) continue;
        const uint8_t mid = asked[k];
        // size: lo fits, hi does not; distortion: lo fails, hi meets
        if (size_mode ? payload_bytes <= budget : !(sse[k] <= max_sse[k]))
          lo[k] = mid;
        else
          hi[k] = mid;
      }
    }
    step++;
    if (failed) return;
    if (step >= 2) {
      for (int k = 0; k < planes; k++)
        if (!fixed[k] && hi[k] - lo[k] <= 1) finish_plane(k, size_mode ? lo[k] : hi[k]);
    }
    bool all = true;
    for (int k = 0; k < planes; k++) all = all && fixed[k];
    if (all) {
      if (size_mode) quality[1] = quality[2] = quality[0];
      done = true;
    }
  }

 private:
  void finish_plane(int k, uint8_t q) {
    fixed[k] = true;
    quality[k] = q;
  }
  void fail() {
    failed = done = true;
    for (int p = 0; p < 3; p++) quality[p] = asked[p];  // (size mode names no plane)
  }
};

// myyuv_metric_sse_for_psnr: the largest s with psnr(s, nsamples) >= db, by the
// formula s <= 65025 nsamples / 10^(db / 10) and then stepped against `psnr`
// itself (the caller's myyuv_metric_psnr), so the two cannot disagree.
// db <= 0: 65025 nsamples; +inf: 0 (psnr(0) is +inf).  NaN: 0.
template <class Psnr>
inline uint64_t sse_for_psnr(double db, uint64_t nsamples, Psnr psnr) {
  const uint64_t top = 65025ull * nsamples;
  if (db != db) return 0;
  if (db <= 0.0) return top;
  const double lim = 65025.0 * (double)nsamples / __builtin_pow(10.0, db / 10.0);
  uint64_t s = lim >= (double)top ? top : (lim > 0.0 ? (uint64_t)lim : 0);
  while (s < top && psnr(s + 1, nsamples) >= db) s++;
  while (s > 0 && !(psnr(s, nsamples) >= db)) s--;
  return s;
}

}  // namespace myyuv_rate

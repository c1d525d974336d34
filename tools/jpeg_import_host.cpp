// jpeg_import_host.cpp — the JPEG import's marker parser and block decoder
// (csrc/jpeg_import.h: the code k_jpeg_import and the library's host decode
// run) as a stand-alone host program, for tests/test_jpeg_import_host.py.
//
//   jpeg_import_host < file.jpg > out
//
// out, little-endian: i32 code of inspect (0, 21 unsupported, 22 syntax); when
// 0: u32 W, H, Wp, Hp, scans, segments, Ri[3], interleaved; u8 qt[3][64]
// (natural order); the segment table, 5 x u32 per interval (offset, length,
// first MCU, MCU count, scan); i32 code of the decode (0 or 23), i64 the
// lowest failing block (-1: none); the coefficient image, int16 [blocks][64]
// in natural order and the stream's block order.  Exit status 0 whenever `out`
// was written.
#include <cstdio>
#include <memory>
#include <vector>

#include "jpeg_import.h"

namespace {

template <class T>
void put(std::vector<uint8_t>& o, T v) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
  o.insert(o.end(), p, p + sizeof(T));
}

}  // namespace

int main() {
  std::vector<uint8_t> file;
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), stdin)) > 0;) file.insert(file.end(), buf, buf + n);
  // (an exact-size heap copy: a read one byte past the file is a sanitizer finding)
  std::unique_ptr<uint8_t[]> exact(new uint8_t[file.size() ? file.size() : 1]);
  for (size_t i = 0; i < file.size(); i++) exact[i] = file[i];
  const uint8_t* f = exact.get();
  const uint32_t size = (uint32_t)file.size();
  using namespace myyuv_jpegin;
  auto I = std::make_unique<Info>();
  std::vector<uint8_t> out;
  int rc = inspect(f, size, *I, nullptr, 0);
  std::vector<Seg> segs(rc ? 0 : I->nseg);
  if (!rc) rc = inspect(f, size, *I, segs.data(), (uint32_t)segs.size());
  put<int32_t>(out, rc);
  if (!rc) {
    const Plan& P = I->plan;
    for (uint32_t v : {I->W, I->H, I->Wp, I->Hp, P.nscan, I->nseg, P.ri[0], P.ri[1], P.ri[2], (uint32_t)(P.ns[0] == 3)})
      put<uint32_t>(out, v);
    for (int p = 0; p < 3; p++) out.insert(out.end(), I->qt[p], I->qt[p] + 64);
    for (const Seg& s : segs)
      for (uint32_t v : {s.off, s.len, s.mcu0, s.nmcu, s.scan}) put<uint32_t>(out, v);
    std::vector<int16_t> img((size_t)P.cum[3] * 64, 0);
    int64_t bad = -1;
    const int drc = decode_scans(f, size, *I, segs.data(), (uint32_t)segs.size(), img.data(), &bad);
    put<int32_t>(out, drc);
    put<int64_t>(out, bad);
    const uint8_t* p = reinterpret_cast<const uint8_t*>(img.data());
    out.insert(out.end(), p, p + img.size() * 2);
  }
  return fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 1;
}

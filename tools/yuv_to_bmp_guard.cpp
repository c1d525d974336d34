// yuv_to_bmp_guard.cpp — myyuv::yuv_to_bmp must refuse a frame whose BMP pixel
// array does not fit BMP::imageSize()'s 32 bits (|w| * |h| * bit_count / 8)
// before it allocates or touches the GPU: such a BMP cannot be dumped, and a
// wrapped size would make the result buffer too small for what the device
// writes.  Host only (no GPU needed: the guard precedes the codec context);
// meant to be built with AddressSanitizer, linked against libmyyuv_amd.so.
// Prints "ok" when every oversized case throws "Invalid argument".
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "myyuv_yuv.hpp"

static bool refused(uint32_t w, uint32_t h, uint16_t bits) {
  myyuv::YUV y;
  y.header.fourcc_format = myyuv::YUV::FourccFormats::IYUV;
  y.header.width = w;
  y.header.height = h;
  y.header.data_size = 1;  // (never read: the guard comes first)
  y.header.data_pos = sizeof(myyuv::YUVHeader);
  y.data = new uint8_t[1]();
  try {
    myyuv::BMP b = myyuv::yuv_to_bmp(y, bits);
    std::printf("%ux%u %u bpp: accepted, imageSize %u\n", w, h, bits, b.imageSize());
  } catch (const std::runtime_error& e) {
    if (std::strcmp(e.what(), "Invalid argument") == 0) return true;
    std::printf("%ux%u %u bpp: %s\n", w, h, bits, e.what());
  }
  return false;
}

int main() {
  bool ok = true;
  ok &= refused(16384, 8192, 32);    // 2^27 pixels: imageSize() wraps to 0 at 32 bpp
  ok &= refused(32768, 16384, 24);   // 2^29 pixels: w * h * 24 wraps to 0 too
  ok &= refused(16384, 12288, 24);   // 201 M pixels: 24 bpp wraps, 32-bit BGRA bytes (805 MB) would not
  ok &= refused(16384, 8192 + 2, 32);
  ok &= refused(65536, 65536, 32);
  if (!ok) return 1;
  std::puts("ok");
  return 0;
}

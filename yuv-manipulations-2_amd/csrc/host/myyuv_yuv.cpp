// myyuv_yuv.cpp — the C++ host surface (myyuv::YUV + the DCT codec entry
// points) over the gfx950 C ABI.  Behaviour follows the reference
// (myyuv_lib/myyuv_yuv.cpp:130-536, myyuv_DCT/DCT.cpp:371-488): same header
// normalisation on load, same header rewrites on compress/decompress, same
// std::runtime_error messages.  The per-block work runs on the GPU; this file
// only validates, allocates (new[], as YUV's destructor expects) and copies.
#include "myyuv_yuv.hpp"

#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <vector>

#include <exception>
#include <thread>

#include "myyuv_hip.h"

namespace {

// One codec context per host thread (the C ABI contexts are not shared
// across threads); device from MYYUV_HIP_DEVICE, default 0.
struct ThreadCodec {
  myyuv_hip_handle h = nullptr;
  ~ThreadCodec() {
    if (h) myyuv_hip_destroy(h);
  }
  myyuv_hip_handle get() {
    if (!h) {
      const char* dev = std::getenv("MYYUV_HIP_DEVICE");
      const int rc = myyuv_hip_create(dev ? std::atoi(dev) : 0, &h);
      if (rc) throw std::runtime_error(myyuv_hip_strerror(rc));
    }
    return h;
  }
};
thread_local ThreadCodec t_codec;

[[noreturn]] void fail(int rc) { throw std::runtime_error(myyuv_hip_error_message(rc)); }

uint8_t* dup(const uint8_t* src, size_t n) {
  if (!src) return nullptr;
  uint8_t* p = new uint8_t[n];
  std::memcpy(p, src, n);
  return p;
}

}  // namespace

namespace myyuv {

std::unordered_map<YUV::FourccFormat, YUV::FormatGroup> YUV::yuv_format_group_map = {
    {FourccFormats::IYUV, FormatGroup::PLANAR},
};
std::unordered_map<YUV::FourccFormat, std::array<uint8_t, YUV::max_planes>> YUV::yuv_order_planes_map = {
    {FourccFormats::IYUV, {0, 1, 2, no_plane}},
};
std::unordered_map<YUV::FourccFormat, std::array<uint32_t, 2>> YUV::yuv_resolution_fraction_map = {
    {FourccFormats::IYUV, {2, 2}},
};

// BMP -> IYUV (myyuv_yuv.cpp:88-128): K7 on the GPU (myyuv_gpu_bmp_to_iyuv);
// the raw-image header as the reference's lambda sets it.
std::unordered_map<YUV::FourccFormat, std::function<YUV(const BMP&)>> YUV::bmp_to_yuv_map = {
    {FourccFormats::IYUV,
     [](const BMP& bmp) -> YUV {
       YUV res;
       const uint32_t w = bmp.trueWidth(), h = bmp.trueHeight();
       res.header.fourcc_format = FourccFormats::IYUV;
       res.header.width = w;
       res.header.height = h;
       res.header.data_size = w * h * 3 / 2;
       res.header.data_pos = sizeof(YUVHeader);
       res.data = new uint8_t[res.header.data_size];
       const int rc = myyuv_gpu_bmp_to_iyuv(t_codec.get(), bmp.data, bmp.header.width, bmp.header.height,
                                            bmp.header.bit_count, res.data);
       if (rc) fail(rc);
       return res;
     }},
};

// Registry: the [DCT][IYUV] entries are the drop-in (myyuv_yuv.cpp:130-160).
std::unordered_map<YUV::Compression,
                   std::unordered_map<YUV::FourccFormat, std::function<YUV(const YUV&, const void*, uint32_t)>>>
    YUV::compress_map = {
        {Compressions::DCT,
         {{FourccFormats::IYUV,
           [](const YUV& yuv, const void* params, uint32_t params_size) -> YUV {
             if (params_size != 3)
               throw std::runtime_error("Error compression: incorrect parameters count. 3 parameters required");
             const uint8_t* p = static_cast<const uint8_t*>(params);
             return myyuvDCT::compress_DCT_planar(yuv, {p[0], p[1], p[2]});
           }}}},
};
std::unordered_map<YUV::Compression, std::unordered_map<YUV::FourccFormat, std::function<YUV(const YUV&)>>>
    YUV::decompress_map = {
        {Compressions::DCT,
         {{FourccFormats::IYUV,
           [](const YUV& yuv) -> YUV {
             if (yuv.header.compression_params_size != 3)
               throw std::runtime_error(
                   "Error decompression: incorrect parameters count. 3 parameters required");
             const uint8_t* p = yuv.compression_params;
             return myyuvDCT::decompress_DCT_planar(yuv, {p[0], p[1], p[2]});
           }}}},
};

YUV::YUV(const std::string& path) { load(path); }

YUV::YUV(const BMP& bmp, FourccFormat format) { load(bmp, format); }

// myyuv_yuv.cpp:512-523
void YUV::load(const BMP& bmp, FourccFormat format) {
  if (!bmp.isValid()) throw std::runtime_error("BMP is invalid");
  auto it = bmp_to_yuv_map.find(format);
  if (it == bmp_to_yuv_map.end()) throw std::runtime_error("Incorrect format");
  YUV tmp = it->second(bmp);
  *this = std::move(tmp);
}

YUV::YUV(const YUV& yuv) { *this = yuv; }

YUV& YUV::operator=(const YUV& yuv) {
  if (this == &yuv) return *this;
  uint8_t* d = dup(yuv.data, yuv.header.data_size);
  uint8_t* p = nullptr;
  try {
    p = dup(yuv.compression_params, yuv.header.compression_params_size);
  } catch (...) {
    delete[] d;
    throw;
  }
  delete[] data;
  delete[] compression_params;
  data = d;
  compression_params = p;
  header = yuv.header;
  return *this;
}

YUV::YUV(YUV&& yuv) noexcept { *this = std::move(yuv); }

YUV& YUV::operator=(YUV&& yuv) noexcept {
  std::swap(header, yuv.header);
  std::swap(compression_params, yuv.compression_params);
  std::swap(data, yuv.data);
  return *this;
}

YUV::~YUV() {
  delete[] data;
  delete[] compression_params;
}

bool YUV::isValid() const noexcept {
  const bool params_ok = (header.compression_params_size > 0 && compression_params != nullptr) ||
                         (header.compression == Compressions::NONE && compression_params == nullptr) ||
                         (header.compression_params_size == 0 && compression_params == nullptr);
  return data != nullptr && params_ok && isValidHeader();
}

bool YUV::isValidHeader() const noexcept {
  return header.type[0] == 'Y' && header.type[1] == 'U' &&
         isImplementedFormat(getFourccFormat(), getCompression()) && header.width > 0 &&
         header.height > 0 && header.data_pos >= sizeof(YUVHeader) + header.compression_params_size &&
         header.data_size > 0;
}

bool YUV::isImplementedFormat(FourccFormat format, Compression compression) noexcept {
  if (!yuv_format_group_map.count(format) || !yuv_resolution_fraction_map.count(format)) return false;
  if (compression == Compressions::NONE) return true;
  const auto c = compress_map.find(compression);
  const auto d = decompress_map.find(compression);
  return c != compress_map.end() && d != decompress_map.end() && c->second.count(format) &&
         d->second.count(format);
}

std::array<uint32_t, 2> YUV::getResolutionFraction() const {
  if (!isImplementedFormat(getFourccFormat(), Compressions::NONE))
    throw std::runtime_error("Error. Unimplemented format.");
  return yuv_resolution_fraction_map.at(getFourccFormat());
}

std::array<uint8_t, YUV::max_planes> YUV::getYUVPlanesOrder() const {
  if (!isImplementedFormat(getFourccFormat(), Compressions::NONE))
    throw std::runtime_error("Error. Unimplemented format.");
  const auto it = yuv_order_planes_map.find(getFourccFormat());
  if (it == yuv_order_planes_map.end()) throw std::runtime_error("Error. Planar type unimplemented (?)");
  return it->second;
}

std::array<uint32_t, 2> YUV::getWidthHeightChannel(uint8_t channel) const {
  const auto order = getYUVPlanesOrder();
  if (channel >= max_planes || order[channel] == no_plane) return {0, 0};
  if (channel == 1 || channel == 2) {
    const auto f = getResolutionFraction();
    return {header.width / f[0], header.height / f[1]};
  }
  return {header.width, header.height};
}

std::array<uint32_t, YUV::max_planes> YUV::getFormatSizeBits() const {
  const auto f = getResolutionFraction();
  const auto order = getYUVPlanesOrder();
  const uint32_t frac = f[0] * f[1];
  std::array<uint32_t, max_planes> bits = {8, 8 / frac, 8 / frac, 8};
  for (uint32_t i = 0; i < max_planes; i++)
    if (order[i] == no_plane) bits[i] = 0;
  return bits;
}

uint32_t YUV::getImageSize() const {
  const auto bits = getFormatSizeBits();
  uint64_t total = 0;
  for (uint32_t b : bits) total += (uint64_t)header.width * header.height * b / 8;
  if (total > 0xFFFFFFFFull) throw std::runtime_error("Error. Image too large.");
  return (uint32_t)total;
}

std::array<const uint8_t*, YUV::max_planes> YUV::getYUVPlanes() const {
  const auto order = getYUVPlanesOrder();
  const auto bits = getFormatSizeBits();
  std::array<const uint8_t*, max_planes> res = {nullptr, nullptr, nullptr, nullptr};
  // planes are stored back to back in `order`
  const uint8_t* cur = data;
  for (uint32_t slot = 0; slot < max_planes; slot++) {
    for (uint32_t ch = 0; ch < max_planes; ch++) {
      if (order[ch] != slot) continue;
      if (bits[ch]) res[ch] = cur;
      cur += (size_t)header.width * header.height * bits[ch] / 8;
    }
  }
  return res;
}

std::array<uint8_t*, YUV::max_planes> YUV::getYUVPlanes() {
  const auto c = static_cast<const YUV*>(this)->getYUVPlanes();
  return {const_cast<uint8_t*>(c[0]), const_cast<uint8_t*>(c[1]), const_cast<uint8_t*>(c[2]),
          const_cast<uint8_t*>(c[3])};
}

YUV::FormatGroup YUV::getFormatGroup(FourccFormat format) noexcept {
  const auto it = yuv_format_group_map.find(format);
  return it == yuv_format_group_map.end() ? FormatGroup::UNKNOWN : it->second;
}

YUV YUV::compress(Compression compression, const void* params, uint32_t params_size) const {
  if (getCompression() != Compressions::NONE) throw std::runtime_error("Error already compressed");
  const auto c = compress_map.find(compression);
  if (c == compress_map.end()) throw std::runtime_error("Error this compression is unimplemented");
  const auto f = c->second.find(getFourccFormat());
  if (f == c->second.end()) throw std::runtime_error("Error compression for this format is unimplemented");
  return f->second(*this, params, params_size);
}

YUV YUV::decompress() const {
  if (getCompression() == Compressions::NONE) return *this;
  const auto c = decompress_map.find(getCompression());
  if (c == decompress_map.end()) throw std::runtime_error("Error this decompression is unimplemented");
  const auto f = c->second.find(getFourccFormat());
  if (f == c->second.end()) throw std::runtime_error("Error decompression for this format is unimplemented");
  return f->second(*this);
}

// YUV::load (myyuv_yuv.cpp:485-510): header, params at params_pos, data at
// data_pos; params_pos / data_pos normalised to 64 / 64 + params_size and a
// raw image's data_size recomputed from its geometry.
void YUV::load(const std::string& path) {
  YUV res;
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("Error opening file to read " + path);
  f.read(reinterpret_cast<char*>(&res.header), sizeof(res.header));
  if (!res.isValidHeader()) throw std::runtime_error("Error bad header " + path);
  if (res.header.compression_params_size > 0) {
    f.seekg(res.header.compression_params_pos, std::ios::beg);
    res.compression_params = new uint8_t[res.header.compression_params_size]();
    f.read(reinterpret_cast<char*>(res.compression_params), res.header.compression_params_size);
  }
  f.clear();
  f.seekg(res.header.data_pos, std::ios::beg);
  res.header.compression_params_pos = sizeof(res.header);
  res.header.data_pos = res.header.compression_params_pos + res.header.compression_params_size;
  if (res.getCompression() == Compressions::NONE) res.header.data_size = res.getImageSize();
  res.data = new uint8_t[res.header.data_size]();
  f.read(reinterpret_cast<char*>(res.data), res.header.data_size);
  *this = std::move(res);
}

void YUV::dump(const std::string& path) const {
  std::ofstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("Error opening file to write " + path);
  f.write(reinterpret_cast<const char*>(&header), sizeof(header));
  if (compression_params) f.write(reinterpret_cast<const char*>(compression_params), header.compression_params_size);
  f.write(reinterpret_cast<const char*>(data), header.data_size);
}

namespace {

// The region checks of include/myyuv_hip.h (region decode), for the paths
// that crop on the host.
void check_region(uint32_t w, uint32_t h, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh) {
  if (((rx | ry | rw | rh) & 15u) || rw == 0 || rh == 0 || (uint64_t)rx + rw > w || (uint64_t)ry + rh > h)
    fail(MYYUV_E_ARG);
}

// Header of the region's frame: decompress_DCT_planar's rewrite (DCT.cpp:446-453)
// with the region's size.
YUVHeader region_header(const YUVHeader& in, uint32_t rw, uint32_t rh) {
  YUVHeader h = in;
  h.compression = YUV::Compressions::NONE;
  h.compression_params_size = 0;
  h.compression_params_pos = 0;
  h.data_pos = sizeof(YUVHeader);
  h.width = rw;
  h.height = rh;
  h.data_size = (uint32_t)((uint64_t)rw * rh * 3 / 2);
  return h;
}

// yuv_to_bmp of the whole frame (region == nullptr, denom == 0), of
// region[0..3] = (rx, ry, rw, rh), or of the compressed frame's scaled decode
// (denom 2, 4 or 8; no region).
BMP to_bmp(const YUV& yuv, const uint32_t* region, uint32_t denom, uint16_t bit_count, uint32_t chroma) {
  static_assert(MYYUV_CHROMA_LINEAR == 1, "the header's default chroma mode");
  if (!yuv.isValid()) throw std::runtime_error("YUV is invalid");
  if (yuv.getFourccFormat() != YUV::FourccFormats::IYUV) throw std::runtime_error("Incorrect format");
  if (bit_count != 24 && bit_count != 32) fail(MYYUV_E_BMP_UNSUPPORTED);
  const uint32_t fw = yuv.header.width, fh = yuv.header.height;
  if (denom) {
    if (yuv.getCompression() == YUV::Compressions::NONE)
      throw std::runtime_error("Error. The image is not compressed: a scaled decode needs DCT coefficients");
    if (denom != 2 && denom != 4 && denom != 8) fail(MYYUV_E_ARG);  // (the result's size depends on it)
  }
  if (region && yuv.getCompression() == YUV::Compressions::NONE) check_region(fw, fh, region[0], region[1], region[2], region[3]);
  // (a compressed frame's region is checked by the C ABI, after the stream's header)
  const uint32_t w = region ? region[2] : (denom ? fw / denom : fw), h = region ? region[3] : (denom ? fh / denom : fh);
  // BMP::imageSize(), file_size and dump() hold the pixel array's size in 32
  // bits, and imageSize() forms w * h * bit_count before it divides: an image
  // past that cannot be a BMP (and a wrapped size would under-allocate `data`)
  const uint64_t bytes = (uint64_t)w * h * (bit_count / 8);
  if ((uint64_t)w * h * bit_count > 0xFFFFFFFFull || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) fail(MYYUV_E_ARG);
  BMP res;
  BMPHeader& bh = res.header;
  bh.width = (int32_t)w;  // bottom-up rows
  bh.height = (int32_t)h;
  bh.planes = 1;
  bh.bit_count = bit_count;
  bh.header_size = bit_count == 32 ? 124 : 40;
  bh.compression = bit_count == 32 ? 3 : 0;
  bh.data_pos = (uint32_t)(sizeof(BMPHeader) + (bit_count == 32 ? sizeof(BMPColorHeader) : 0));
  if (res.imageSize() != bytes || bytes > 0xFFFFFFFFull - bh.data_pos) fail(MYYUV_E_ARG);
  bh.file_size = bh.data_pos + (uint32_t)bytes;
  res.data = new uint8_t[bytes ? bytes : 1];
  int rc;
  if (yuv.getCompression() == YUV::Compressions::NONE) {
    if (yuv.header.data_size < (uint64_t)fw * fh * 3 / 2) throw std::runtime_error("YUV is invalid");
    if (region) {
      const YUV part = crop_region(yuv, region[0], region[1], region[2], region[3]);
      rc = myyuv_gpu_iyuv_to_bmp(t_codec.get(), part.data, bh.width, bh.height, bit_count, chroma, res.data);
    } else {
      rc = myyuv_gpu_iyuv_to_bmp(t_codec.get(), yuv.data, bh.width, bh.height, bit_count, chroma, res.data);
    }
  } else if (yuv.getCompression() == YUV::Compressions::DCT) {
    if (yuv.header.compression_params_size != 3)
      throw std::runtime_error("Error decompression: incorrect parameters count. 3 parameters required");
    int64_t bad = -1;
    if (fw > 0x7FFFFFFFu || fh > 0x7FFFFFFFu) fail(MYYUV_E_ARG);
    rc = denom  ? myyuv_gpu_dct_decompress_scaled_to_bmp(t_codec.get(), yuv.data, yuv.header.data_size, (int32_t)fw,
                                                         (int32_t)fh, yuv.compression_params, denom, bit_count,
                                                         chroma, res.data, &bad)
         : region ? myyuv_gpu_dct_decompress_region_to_bmp(t_codec.get(), yuv.data, yuv.header.data_size, (int32_t)fw,
                                                         (int32_t)fh, yuv.compression_params, region[0], region[1],
                                                         region[2], region[3], bit_count, chroma, res.data, &bad)
                : myyuv_gpu_dct_decompress_to_bmp(t_codec.get(), yuv.data, yuv.header.data_size, bh.width, bh.height,
                                                  yuv.compression_params, bit_count, chroma, res.data, &bad);
  } else {
    throw std::runtime_error("Error this decompression is unimplemented");
  }
  if (rc) fail(rc);
  return res;
}

}  // namespace

BMP yuv_to_bmp(const YUV& yuv, uint16_t bit_count, uint32_t chroma) { return to_bmp(yuv, nullptr, 0, bit_count, chroma); }

BMP yuv_to_bmp_scaled(const YUV& yuv, uint32_t denom, uint16_t bit_count, uint32_t chroma) {
  if (denom == 0) fail(MYYUV_E_ARG);
  return to_bmp(yuv, nullptr, denom, bit_count, chroma);
}

BMP yuv_to_bmp(const YUV& yuv, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh, uint16_t bit_count,
               uint32_t chroma) {
  const uint32_t region[4] = {rx, ry, rw, rh};
  return to_bmp(yuv, region, 0, bit_count, chroma);
}

YUV crop_region(const YUV& yuv, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh) {
  if (!yuv.isValid()) throw std::runtime_error("YUV is invalid");
  if (yuv.getFourccFormat() != YUV::FourccFormats::IYUV) throw std::runtime_error("Incorrect format");
  if (yuv.getCompression() != YUV::Compressions::NONE) throw std::runtime_error("Error. The image is compressed");
  const uint32_t w = yuv.header.width, h = yuv.header.height;
  if (yuv.header.data_size < (uint64_t)w * h * 3 / 2) throw std::runtime_error("YUV is invalid");
  check_region(w, h, rx, ry, rw, rh);
  YUV res;
  res.header = region_header(yuv.header, rw, rh);
  res.data = new uint8_t[res.header.data_size];
  const uint8_t* src = yuv.data;
  uint8_t* dst = res.data;
  for (int p = 0; p < 3; p++) {  // Y, then U and V at half size
    const uint32_t sh = p ? 1 : 0;
    const size_t pw = w >> sh, ph = h >> sh, cw = rw >> sh, ch = rh >> sh;
    for (size_t y = 0; y < ch; y++) std::memcpy(dst + y * cw, src + ((ry >> sh) + y) * pw + (rx >> sh), cw);
    src += pw * ph;
    dst += cw * ch;
  }
  return res;
}

// Compare (include/myyuv_hip.h).  Either side raw or DCT-compressed: two raw
// frames through myyuv_gpu_iyuv_compare; a stream and a raw frame through the
// fused myyuv_gpu_dct_compare, the stream's decoded frame never written; of
// two streams `other` is decoded first and *this takes the fused path.  The
// metric is symmetric, so which side is the reference does not matter.
myyuv_frame_metric YUV::compare(const YUV& other, std::vector<myyuv_block_metric>* map) const {
  auto side_ok = [](const YUV& y) {
    if (!y.isValidHeader() || !y.data) throw std::runtime_error("YUV is invalid");
    if (y.getFourccFormat() != FourccFormats::IYUV) throw std::runtime_error("Incorrect format");
    if (y.getCompression() == Compressions::NONE) {
      if (y.header.data_size < (uint64_t)y.header.width * y.header.height * 3 / 2)
        throw std::runtime_error("YUV is invalid");
    } else if (y.getCompression() != Compressions::DCT) {
      throw std::runtime_error("Error this decompression is unimplemented");
    } else if (y.header.compression_params_size != 3 || !y.compression_params) {
      throw std::runtime_error("Error decompression: incorrect parameters count. 3 parameters required");
    }
  };
  side_ok(*this);
  side_ok(other);
  if (header.width != other.header.width || header.height != other.header.height ||
      getFourccFormat() != other.getFourccFormat())
    throw std::runtime_error("Error comparing: the frames differ in size or format");
  const uint32_t w = header.width, h = header.height;
  const uint64_t nblk = (uint64_t)(w / 8) * (h / 8) + 2ull * (w / 16) * (h / 16);
  if (map) map->assign(nblk ? nblk : 1, myyuv_block_metric{0, 0});
  myyuv_block_metric* mp = map ? map->data() : nullptr;
  myyuv_frame_metric out;
  std::memset(&out, 0, sizeof(out));
  int64_t bad = -1;
  int rc;
  if (!isCompressed() && !other.isCompressed()) {
    rc = myyuv_gpu_iyuv_compare(t_codec.get(), data, other.data, w, h, &out, mp);
  } else if (isCompressed() && other.isCompressed()) {
    const YUV raw = other.decompress();
    rc = myyuv_gpu_dct_compare(t_codec.get(), data, header.data_size, w, h, compression_params, raw.data, &out, mp,
                               &bad);
  } else {
    const YUV& s = isCompressed() ? *this : other;
    const YUV& r = isCompressed() ? other : *this;
    rc = myyuv_gpu_dct_compare(t_codec.get(), s.data, s.header.data_size, w, h, s.compression_params, r.data, &out,
                               mp, &bad);
  }
  if (rc) fail(rc);
  if (map) map->resize(nblk);
  return out;
}

// Probe and encode to a target (include/myyuv_hip.h).
namespace {

void raw_planar_ok(const YUV& y) {
  if (y.getFormatGroup() != YUV::FormatGroup::PLANAR) throw std::runtime_error("Error compressing: YUV must be planar");
  if (y.getCompression() != YUV::Compressions::NONE)
    throw std::runtime_error("Error compressing: can't compress uncompressed YUV");
}

// compress_DCT_planar's result from a payload and its three quality bytes
YUV compressed_like(const YUV& yuv, const uint8_t q[3], const uint8_t* payload, uint32_t size) {
  YUV res;
  res.header = yuv.header;
  res.header.compression = YUV::Compressions::DCT;
  res.header.compression_params_size = 3;
  res.header.compression_params_pos = sizeof(YUVHeader);
  res.header.data_pos = sizeof(YUVHeader) + 3;
  res.header.data_size = size;
  res.compression_params = new uint8_t[3]{q[0], q[1], q[2]};
  res.data = new uint8_t[size];
  std::memcpy(res.data, payload, size);
  return res;
}

}  // namespace

myyuv_probe YUV::probe(const std::array<uint8_t, 3>& q) const {
  raw_planar_ok(*this);
  myyuv_probe out;
  const int rc = myyuv_gpu_dct_probe(t_codec.get(), data, header.width, header.height, q.data(),
                                     MYYUV_PROBE_SIZE | MYYUV_PROBE_METRIC, &out, nullptr);
  if (rc) fail(rc);
  return out;
}

YUV YUV::compress_to_size(uint32_t payload_bytes, myyuv_target_result* result) const {
  raw_planar_ok(*this);
  std::vector<uint8_t> payload(myyuv_dct_payload_bound(header.width, header.height));
  uint32_t size = 0;
  myyuv_target_result r;
  const int rc = myyuv_gpu_dct_compress_to_size(t_codec.get(), data, header.width, header.height, payload_bytes,
                                                payload.data(), (uint32_t)payload.size(), &size, &r);
  if (result) *result = r;
  if (rc) fail(rc);
  return compressed_like(*this, r.quality, payload.data(), size);
}

YUV YUV::compress_to_psnr(double db, myyuv_target_result* result) const {
  raw_planar_ok(*this);
  if (db != db) fail(MYYUV_E_ARG);
  const uint64_t n = (uint64_t)header.width * header.height;
  const uint64_t max_sse[3] = {myyuv_metric_sse_for_psnr(db, n), myyuv_metric_sse_for_psnr(db, n / 4),
                               myyuv_metric_sse_for_psnr(db, n / 4)};
  std::vector<uint8_t> payload(myyuv_dct_payload_bound(header.width, header.height));
  uint32_t size = 0;
  myyuv_target_result r;
  const int rc = myyuv_gpu_dct_compress_to_sse(t_codec.get(), data, header.width, header.height, max_sse,
                                               payload.data(), (uint32_t)payload.size(), &size, &r);
  if (result) *result = r;
  if (rc) fail(rc);
  return compressed_like(*this, r.quality, payload.data(), size);
}

namespace {

// One call with room for `first` bytes, and once more at the size the call
// reports when the file is larger: no buffer of myyuv_jpeg_bound's size.
template <class Call>
std::vector<uint8_t> jpeg_file(uint32_t first, Call call) {
  std::vector<uint8_t> out(first);
  uint32_t size = 0;
  int rc = call(out.data(), (uint32_t)out.size(), &size);
  if (rc == MYYUV_E_CAPACITY) {
    out.resize(size);
    rc = call(out.data(), (uint32_t)out.size(), &size);
  }
  if (rc) fail(rc);
  out.resize(size);
  return out;
}

}  // namespace

std::vector<uint8_t> YUV::to_jpeg() const {
  if (getFormatGroup() != FormatGroup::PLANAR) throw std::runtime_error("Error decompressing: YUV must be planar");
  if (getCompression() != Compressions::DCT)
    throw std::runtime_error("Error exporting: image is not compressed (to_jpeg needs DCT coefficients)");
  if (header.compression_params_size != 3 || !compression_params)
    throw std::runtime_error("Error decompression: incorrect parameters count. 3 parameters required");
  for (int p = 0; p < 3; p++)
    if (compression_params[p] < 1 || compression_params[p] > 100)
      throw std::runtime_error("Level of quality must be between 1 and 100");
  return jpeg_file(header.data_size + 1024, [this](uint8_t* out, uint32_t cap, uint32_t* size) {
    int64_t bad = -1;
    return myyuv_gpu_dct_to_jpeg(t_codec.get(), data, header.data_size, header.width, header.height,
                                 compression_params, out, cap, size, &bad);
  });
}

std::vector<uint8_t> YUV::to_jpeg(const std::array<uint8_t, 3>& q) const {
  raw_planar_ok(*this);
  for (uint8_t v : q)
    if (v < 1 || v > 100) throw std::runtime_error("Level of quality must be between 1 and 100");
  const uint32_t first = std::max<uint32_t>(4096, header.width / 4 * header.height);
  return jpeg_file(first, [this, &q](uint8_t* out, uint32_t cap, uint32_t* size) {
    return myyuv_gpu_iyuv_to_jpeg(t_codec.get(), data, header.width, header.height, q.data(), out, cap, size);
  });
}

YUV YUV::from_jpeg(const std::vector<uint8_t>& file, const uint8_t* q, myyuv_jpeg_info* info) {
  // the file's checks need no device: they come first
  myyuv_jpeg_info I;
  int rc = myyuv_jpeg_inspect(file.data(), (uint32_t)file.size(), &I);
  if (rc) fail(rc);
  if (info) *info = I;
  if (q)
    for (int p = 0; p < 3; p++)
      if (q[p] < 1 || q[p] > 100) throw std::runtime_error("Level of quality must be between 1 and 100");
  std::vector<uint8_t> payload(I.payload_bound ? I.payload_bound : 64);
  uint32_t size = 0, w = 0, h = 0;
  uint8_t qs[3] = {0, 0, 0};
  int64_t bad = -1;
  rc = myyuv_gpu_jpeg_to_dct(t_codec.get(), file.data(), (uint32_t)file.size(), q, payload.data(),
                             (uint32_t)payload.size(), &size, &w, &h, qs, &bad);
  if (rc) fail(rc);
  YUV res;
  res.header.fourcc_format = FourccFormats::IYUV;
  res.header.width = w;
  res.header.height = h;
  res.header.compression = Compressions::DCT;
  res.header.compression_params_size = 3;
  res.header.compression_params_pos = sizeof(YUVHeader);
  res.header.data_pos = sizeof(YUVHeader) + 3;
  res.header.data_size = size;
  res.compression_params = new uint8_t[3]{qs[0], qs[1], qs[2]};
  res.data = new uint8_t[size];
  std::memcpy(res.data, payload.data(), size);
  return res;
}

}  // namespace myyuv

namespace myyuvDCT {

// compress_DCT_planar (DCT.cpp:371-430): checks, header rewrite
// (compression=1, 3 quality bytes at 64, data at 67), payload from the GPU.
myyuv::YUV compress_DCT_planar(const myyuv::YUV& yuv, const std::array<uint8_t, 3>& params) {
  using myyuv::YUV;
  if (yuv.getFormatGroup() != YUV::FormatGroup::PLANAR)
    throw std::runtime_error("Error compressing: YUV must be planar");
  if (yuv.getCompression() != YUV::Compressions::NONE)
    throw std::runtime_error("Error compressing: can't compress uncompressed YUV");
  for (uint8_t q : params)
    if (q < 1 || q > 100) throw std::runtime_error("Level of quality must be between 1 and 100");
  const uint32_t w = yuv.header.width, h = yuv.header.height;
  std::vector<uint8_t> payload(myyuv_dct_payload_bound(w, h));
  uint32_t size = 0;
  const int rc = myyuv_gpu_dct_compress(t_codec.get(), yuv.data, w, h, params.data(), payload.data(),
                                        (uint32_t)payload.size(), &size);
  if (rc) fail(rc);
  YUV res;
  res.header = yuv.header;
  res.header.compression = YUV::Compressions::DCT;
  res.header.compression_params_size = 3;
  res.header.compression_params_pos = sizeof(myyuv::YUVHeader);
  res.header.data_pos = sizeof(myyuv::YUVHeader) + 3;
  res.header.data_size = size;
  res.compression_params = new uint8_t[3]{params[0], params[1], params[2]};
  res.data = new uint8_t[size];
  std::memcpy(res.data, payload.data(), size);
  return res;
}

// The same from BMP pixels in one GPU pass (myyuv_gpu_bmp_dct_compress): the
// raw-image header as bmp_to_yuv_map[IYUV] sets it, then the rewrite above.
myyuv::YUV compress_DCT_planar(const myyuv::BMP& bmp, const std::array<uint8_t, 3>& params) {
  using myyuv::YUV;
  if (!bmp.isValid()) throw std::runtime_error("BMP is invalid");
  for (uint8_t q : params)
    if (q < 1 || q > 100) throw std::runtime_error("Level of quality must be between 1 and 100");
  const uint32_t w = bmp.trueWidth(), h = bmp.trueHeight();
  std::vector<uint8_t> payload(myyuv_dct_payload_bound(w, h));
  uint32_t size = 0;
  const int rc = myyuv_gpu_bmp_dct_compress(t_codec.get(), bmp.data, bmp.header.width, bmp.header.height,
                                            bmp.header.bit_count, params.data(), payload.data(),
                                            (uint32_t)payload.size(), &size);
  if (rc) fail(rc);
  YUV res;
  res.header.fourcc_format = YUV::FourccFormats::IYUV;
  res.header.width = w;
  res.header.height = h;
  res.header.compression = YUV::Compressions::DCT;
  res.header.compression_params_size = 3;
  res.header.compression_params_pos = sizeof(myyuv::YUVHeader);
  res.header.data_pos = sizeof(myyuv::YUVHeader) + 3;
  res.header.data_size = size;
  res.compression_params = new uint8_t[3]{params[0], params[1], params[2]};
  res.data = new uint8_t[size];
  std::memcpy(res.data, payload.data(), size);
  return res;
}

namespace {

// Frames `idx` of `frames` (any geometries) on context h: frames of one
// geometry go through one pipelined host batch (myyuv_gpu_dct_compress_frames:
// uploads, kernels and downloads overlapped, one launch per kernel per chunk);
// each payload lands in its YUV's own new[] buffer, sized once its length is
// known.
struct PayloadSink {
  std::vector<myyuv::YUV>* out;
  const std::vector<size_t>* dst;  // batch frame -> index into *out
};
uint8_t* payload_sink(void* user, uint32_t frame, uint32_t size) {
  auto* ps = static_cast<PayloadSink*>(user);
  myyuv::YUV& res = (*ps->out)[(*ps->dst)[frame]];
  delete[] res.data;
  res.data = new uint8_t[size ? size : 1];
  return res.data;
}

void compress_share(myyuv_hip_handle h, const std::vector<const myyuv::YUV*>& frames,
                    const std::vector<size_t>& idx, const std::array<uint8_t, 3>& params,
                    std::vector<myyuv::YUV>& out) {
  using myyuv::YUV;
  std::vector<bool> done(idx.size(), false);
  for (size_t i = 0; i < idx.size(); i++) {
    if (done[i]) continue;
    const uint32_t w = frames[idx[i]]->header.width, hh = frames[idx[i]]->header.height;
    std::vector<size_t> dst;  // indices (into frames / out) of this geometry, in input order
    std::vector<const uint8_t*> src;
    for (size_t j = i; j < idx.size(); j++)
      if (!done[j] && frames[idx[j]]->header.width == w && frames[idx[j]]->header.height == hh) {
        dst.push_back(idx[j]);
        src.push_back(frames[idx[j]]->data);
        done[j] = true;
      }
    std::vector<uint32_t> sizes(dst.size());
    PayloadSink ps{&out, &dst};
    const int rc = myyuv_gpu_dct_compress_frames(h, src.data(), (uint32_t)src.size(), w, hh, params.data(),
                                                 payload_sink, &ps, sizes.data());
    if (rc) fail(rc);
    for (size_t k = 0; k < dst.size(); k++) {
      const YUV& in = *frames[dst[k]];
      YUV& res = out[dst[k]];
      res.header = in.header;  // header rewrite as compress_DCT_planar (DCT.cpp:389-396)
      res.header.compression = YUV::Compressions::DCT;
      res.header.compression_params_size = 3;
      res.header.compression_params_pos = sizeof(myyuv::YUVHeader);
      res.header.data_pos = sizeof(myyuv::YUVHeader) + 3;
      res.header.data_size = sizes[k];
      res.compression_params = new uint8_t[3]{params[0], params[1], params[2]};
    }
  }
}

void check_compressible(const std::vector<const myyuv::YUV*>& frames, const std::array<uint8_t, 3>& params) {
  using myyuv::YUV;
  for (uint8_t q : params)
    if (q < 1 || q > 100) throw std::runtime_error("Level of quality must be between 1 and 100");
  for (const YUV* y : frames) {
    if (y->getFormatGroup() != YUV::FormatGroup::PLANAR)
      throw std::runtime_error("Error compressing: YUV must be planar");
    if (y->getCompression() != YUV::Compressions::NONE)
      throw std::runtime_error("Error compressing: can't compress uncompressed YUV");
  }
}

}  // namespace

std::vector<myyuv::YUV> compress_DCT_planar_batch(const std::vector<const myyuv::YUV*>& frames,
                                                  const std::array<uint8_t, 3>& params) {
  check_compressible(frames, params);
  std::vector<myyuv::YUV> out(frames.size());
  std::vector<size_t> all(frames.size());
  for (size_t i = 0; i < frames.size(); i++) all[i] = i;
  compress_share(t_codec.get(), frames, all, params, out);
  return out;
}

// Frames dealt round-robin over `devices` (frame i -> devices[i % n], the
// multi-GPU sharding of SURVEY.md §8e), one host thread and codec context per
// entry; results in input order.  The first failure is rethrown.
std::vector<myyuv::YUV> compress_DCT_planar_batch(const std::vector<const myyuv::YUV*>& frames,
                                                  const std::array<uint8_t, 3>& params,
                                                  const std::vector<int>& devices) {
  if (devices.empty()) return compress_DCT_planar_batch(frames, params);
  check_compressible(frames, params);
  std::vector<myyuv::YUV> out(frames.size());
  const size_t n = devices.size();
  std::vector<std::exception_ptr> errs(n);
  std::vector<std::thread> th;
  for (size_t d = 0; d < n; d++) {
    th.emplace_back([&, d] {
      myyuv_hip_handle h = nullptr;
      try {
        const int rc = myyuv_hip_create(devices[d], &h);
        if (rc) fail(rc);
        std::vector<size_t> mine;
        for (size_t i = d; i < frames.size(); i += n) mine.push_back(i);
        compress_share(h, frames, mine, params, out);
      } catch (...) {
        errs[d] = std::current_exception();
      }
      if (h) myyuv_hip_destroy(h);
    });
  }
  for (auto& t : th) t.join();
  for (auto& e : errs)
    if (e) std::rethrow_exception(e);
  return out;
}

// decompress_DCT_planar (DCT.cpp:432-488): header rewrite (compression=0,
// params 0/0, data at 64, data_size = image size), planes from the GPU.
myyuv::YUV decompress_DCT_planar(const myyuv::YUV& yuv, const std::array<uint8_t, 3>& params) {
  using myyuv::YUV;
  if (yuv.getFormatGroup() != YUV::FormatGroup::PLANAR)
    throw std::runtime_error("Error decompressing: YUV must be planar");
  for (uint8_t q : params)
    if (q < 1 || q > 100) throw std::runtime_error("Level of quality must be between 1 and 100");
  YUV res;
  res.header = yuv.header;
  res.header.compression = YUV::Compressions::NONE;
  res.header.compression_params_size = 0;
  res.header.compression_params_pos = 0;
  res.header.data_pos = sizeof(myyuv::YUVHeader);
  res.header.data_size = res.getImageSize();
  res.data = new uint8_t[res.header.data_size];
  int64_t bad = -1;
  const int rc = myyuv_gpu_dct_decompress(t_codec.get(), yuv.data, yuv.header.data_size, yuv.header.width,
                                          yuv.header.height, params.data(), res.data, &bad);
  if (rc) fail(rc);
  return res;
}

// The region of a compressed frame: decompress_DCT_planar's checks and header
// with the region's size; the C ABI checks the region after the stream's
// header and decodes nothing outside it.
myyuv::YUV decompress_DCT_planar_region(const myyuv::YUV& yuv, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh) {
  using myyuv::YUV;
  if (yuv.getFormatGroup() != YUV::FormatGroup::PLANAR)
    throw std::runtime_error("Error decompressing: YUV must be planar");
  if (yuv.getCompression() != YUV::Compressions::DCT)
    throw std::runtime_error("Error this decompression is unimplemented");
  if (yuv.header.compression_params_size != 3 || !yuv.compression_params)
    throw std::runtime_error("Error decompression: incorrect parameters count. 3 parameters required");
  for (int p = 0; p < 3; p++)
    if (yuv.compression_params[p] < 1 || yuv.compression_params[p] > 100)
      throw std::runtime_error("Level of quality must be between 1 and 100");
  YUV res;
  res.header = myyuv::region_header(yuv.header, rw, rh);
  // (a region the C ABI will refuse may be larger than the frame: no buffer for it)
  const bool fits = (uint64_t)rw * rh <= (uint64_t)yuv.header.width * yuv.header.height;
  res.data = new uint8_t[fits && res.header.data_size ? res.header.data_size : 1];
  int64_t bad = -1;
  const int rc = fits ? myyuv_gpu_dct_decompress_region(t_codec.get(), yuv.data, yuv.header.data_size,
                                                        yuv.header.width, yuv.header.height, yuv.compression_params,
                                                        rx, ry, rw, rh, res.data, &bad)
                      : MYYUV_E_ARG;
  if (rc) fail(rc);
  return res;
}

// The scaled decode of a compressed frame (include/myyuv_hip.h): the checks of
// decompress_DCT_planar_region and its header rewrite with the scaled size.
// A denom other than 2, 4 or 8 is refused here (the result's size depends on
// it); the C ABI checks everything else.
myyuv::YUV decompress_DCT_planar_scaled(const myyuv::YUV& yuv, uint32_t denom) {
  using myyuv::YUV;
  if (yuv.getFormatGroup() != YUV::FormatGroup::PLANAR)
    throw std::runtime_error("Error decompressing: YUV must be planar");
  if (yuv.getCompression() != YUV::Compressions::DCT)
    throw std::runtime_error("Error this decompression is unimplemented");
  if (yuv.header.compression_params_size != 3 || !yuv.compression_params)
    throw std::runtime_error("Error decompression: incorrect parameters count. 3 parameters required");
  for (int p = 0; p < 3; p++)
    if (yuv.compression_params[p] < 1 || yuv.compression_params[p] > 100)
      throw std::runtime_error("Level of quality must be between 1 and 100");
  if (denom != 2 && denom != 4 && denom != 8) fail(MYYUV_E_ARG);
  YUV res;
  res.header = myyuv::region_header(yuv.header, yuv.header.width / denom, yuv.header.height / denom);
  res.data = new uint8_t[res.header.data_size ? res.header.data_size : 1];
  int64_t bad = -1;
  const int rc = myyuv_gpu_dct_decompress_scaled(t_codec.get(), yuv.data, yuv.header.data_size, yuv.header.width,
                                                 yuv.header.height, yuv.compression_params, denom, res.data, &bad);
  if (rc) fail(rc);
  return res;
}

namespace {

// Requantise and transform (include/myyuv_hip.h): the checks of
// decompress_DCT_planar_region on the input, the new qualities' range as
// compress_DCT_planar checks it, and compress_DCT_planar's header rewrite with
// the new quality bytes.  op < 0: requantise; otherwise MYYUV_XF_*, and the
// header's width and height change places for a swapping operation.
myyuv::YUV recode_DCT_planar(const myyuv::YUV& yuv, int op, const std::array<uint8_t, 3>& params) {
  using myyuv::YUV;
  if (yuv.getFormatGroup() != YUV::FormatGroup::PLANAR)
    throw std::runtime_error("Error decompressing: YUV must be planar");
  if (yuv.getCompression() != YUV::Compressions::DCT)
    throw std::runtime_error("Error this decompression is unimplemented");
  if (yuv.header.compression_params_size != 3 || !yuv.compression_params)
    throw std::runtime_error("Error decompression: incorrect parameters count. 3 parameters required");
  for (int p = 0; p < 3; p++)
    if (yuv.compression_params[p] < 1 || yuv.compression_params[p] > 100)
      throw std::runtime_error("Level of quality must be between 1 and 100");
  for (uint8_t q : params)
    if (q < 1 || q > 100) throw std::runtime_error("Level of quality must be between 1 and 100");
  const uint32_t w = yuv.header.width, h = yuv.header.height;
  std::vector<uint8_t> payload(myyuv_dct_payload_bound(w, h));
  uint32_t size = 0;
  int64_t bad = -1;
  const int rc =
      op < 0 ? myyuv_gpu_dct_requantize(t_codec.get(), yuv.data, yuv.header.data_size, w, h, yuv.compression_params,
                                        params.data(), payload.data(), (uint32_t)payload.size(), &size, &bad)
             : myyuv_gpu_dct_transform(t_codec.get(), yuv.data, yuv.header.data_size, w, h, yuv.compression_params,
                                       (uint32_t)op, params.data(), payload.data(), (uint32_t)payload.size(), &size,
                                       &bad);
  if (rc) fail(rc);
  YUV res;
  res.header = yuv.header;
  if (op >= 0 && MYYUV_XF_SWAPS(op)) {
    res.header.width = h;
    res.header.height = w;
  }
  res.header.compression = YUV::Compressions::DCT;
  res.header.compression_params_size = 3;
  res.header.compression_params_pos = sizeof(myyuv::YUVHeader);
  res.header.data_pos = sizeof(myyuv::YUVHeader) + 3;
  res.header.data_size = size;
  res.compression_params = new uint8_t[3]{params[0], params[1], params[2]};
  res.data = new uint8_t[size ? size : 1];
  std::memcpy(res.data, payload.data(), size);
  return res;
}

}  // namespace

myyuv::YUV requantize_DCT_planar(const myyuv::YUV& yuv, const std::array<uint8_t, 3>& params) {
  return recode_DCT_planar(yuv, -1, params);
}

myyuv::YUV transform_DCT_planar(const myyuv::YUV& yuv, uint32_t op, const std::array<uint8_t, 3>& params) {
  if (op > 7) throw std::runtime_error("Error transforming: unknown operation");
  return recode_DCT_planar(yuv, (int)op, params);
}

// Downscale (include/myyuv_hip.h): requantize_DCT_planar's checks on the input
// and on the new qualities; a denom other than 2, 4 or 8 is refused here (the
// result's size depends on it), the C ABI checks everything else.  The header
// is compress_DCT_planar's for the scaled size and the destination qualities.
myyuv::YUV downscale_DCT_planar(const myyuv::YUV& yuv, uint32_t denom, const std::array<uint8_t, 3>& params) {
  using myyuv::YUV;
  if (yuv.getFormatGroup() != YUV::FormatGroup::PLANAR)
    throw std::runtime_error("Error decompressing: YUV must be planar");
  if (yuv.getCompression() != YUV::Compressions::DCT)
    throw std::runtime_error("Error this decompression is unimplemented");
  if (yuv.header.compression_params_size != 3 || !yuv.compression_params)
    throw std::runtime_error("Error decompression: incorrect parameters count. 3 parameters required");
  for (int p = 0; p < 3; p++)
    if (yuv.compression_params[p] < 1 || yuv.compression_params[p] > 100)
      throw std::runtime_error("Level of quality must be between 1 and 100");
  for (uint8_t q : params)
    if (q < 1 || q > 100) throw std::runtime_error("Level of quality must be between 1 and 100");
  if (denom != 2 && denom != 4 && denom != 8) fail(MYYUV_E_ARG);
  const uint32_t w = yuv.header.width, h = yuv.header.height;
  std::vector<uint8_t> payload(myyuv_dct_payload_bound(w / denom, h / denom));
  uint32_t size = 0;
  int64_t bad = -1;
  const int rc = myyuv_gpu_dct_downscale(t_codec.get(), yuv.data, yuv.header.data_size, w, h, yuv.compression_params,
                                         denom, params.data(), payload.data(), (uint32_t)payload.size(), &size, &bad);
  if (rc) fail(rc);
  YUV res;
  res.header = yuv.header;
  res.header.width = w / denom;
  res.header.height = h / denom;
  res.header.compression = YUV::Compressions::DCT;
  res.header.compression_params_size = 3;
  res.header.compression_params_pos = sizeof(myyuv::YUVHeader);
  res.header.data_pos = sizeof(myyuv::YUVHeader) + 3;
  res.header.data_size = size;
  res.compression_params = new uint8_t[3]{params[0], params[1], params[2]};
  res.data = new uint8_t[size ? size : 1];
  std::memcpy(res.data, payload.data(), size);
  return res;
}

myyuv::YUV downscale_DCT_planar(const myyuv::YUV& yuv, uint32_t denom) {
  std::array<uint8_t, 3> q = {0, 0, 0};  // (a source without three parameters: refused by the checks above)
  if (yuv.header.compression_params_size == 3 && yuv.compression_params)
    q = {yuv.compression_params[0], yuv.compression_params[1], yuv.compression_params[2]};
  return downscale_DCT_planar(yuv, denom, q);
}

namespace {

// The input checks of decompress_DCT_planar_region, and the header of a
// compressed w x h result that keeps the source's quality bytes.
void check_dct_input(const myyuv::YUV& yuv) {
  using myyuv::YUV;
  if (yuv.getFormatGroup() != YUV::FormatGroup::PLANAR)
    throw std::runtime_error("Error decompressing: YUV must be planar");
  if (yuv.getCompression() != YUV::Compressions::DCT)
    throw std::runtime_error("Error this decompression is unimplemented");
  if (yuv.header.compression_params_size != 3 || !yuv.compression_params)
    throw std::runtime_error("Error decompression: incorrect parameters count. 3 parameters required");
}

myyuv::YUV gathered(const myyuv::YUV& like, uint32_t w, uint32_t h, const std::vector<uint8_t>& payload,
                    uint32_t size) {
  using myyuv::YUV;
  YUV res;
  res.header = like.header;
  res.header.width = w;
  res.header.height = h;
  res.header.compression = YUV::Compressions::DCT;
  res.header.compression_params_size = 3;
  res.header.compression_params_pos = sizeof(myyuv::YUVHeader);
  res.header.data_pos = sizeof(myyuv::YUVHeader) + 3;
  res.header.data_size = size;
  res.compression_params =
      new uint8_t[3]{like.compression_params[0], like.compression_params[1], like.compression_params[2]};
  res.data = new uint8_t[size ? size : 1];
  std::memcpy(res.data, payload.data(), size);
  return res;
}

}  // namespace

// Crop (include/myyuv_hip.h): the rectangle of a compressed frame, still
// compressed, with the source's params; the C ABI checks the rectangle.
myyuv::YUV crop_DCT_planar(const myyuv::YUV& yuv, uint32_t x, uint32_t y, uint32_t w, uint32_t h) {
  check_dct_input(yuv);
  std::vector<uint8_t> payload((size_t)yuv.header.data_size + 36);  // (a part of the source never exceeds it)
  uint32_t size = 0;
  int64_t bad = -1;
  const int rc = myyuv_gpu_dct_crop(t_codec.get(), yuv.data, yuv.header.data_size, yuv.header.width,
                                    yuv.header.height, x, y, w, h, payload.data(), (uint32_t)payload.size(), &size,
                                    &bad);
  if (rc) fail(rc);
  return gathered(yuv, w, h, payload, size);
}

// Join (include/myyuv_hip.h): cols x rows compressed tiles, row-major, as one
// compressed frame.  The tiles' sizes, formats and params must be equal: a
// stream of mixed qualities is one no single quality decodes.
myyuv::YUV join_DCT_planar(const std::vector<const myyuv::YUV*>& tiles, uint32_t cols, uint32_t rows) {
  if (cols == 0 || rows == 0 || (uint64_t)cols * rows != tiles.size())
    throw std::runtime_error("Error joining: cols * rows tiles are required");
  std::vector<const uint8_t*> ptrs;
  std::vector<uint32_t> sizes;
  uint64_t total = 36;
  for (const myyuv::YUV* t : tiles) {
    if (!t) throw std::runtime_error("Error joining: cols * rows tiles are required");
    check_dct_input(*t);
    const myyuv::YUV& a = *tiles[0];
    if (t->header.width != a.header.width || t->header.height != a.header.height)
      throw std::runtime_error("Error joining: tiles differ in size");
    if (t->header.fourcc_format != a.header.fourcc_format)
      throw std::runtime_error("Error joining: tiles differ in format");
    if (std::memcmp(t->compression_params, a.compression_params, 3) != 0)
      throw std::runtime_error("Error joining: tiles differ in compression params");
    ptrs.push_back(t->data);
    sizes.push_back(t->header.data_size);
    total += t->header.data_size;
  }
  if (total > 0xFFFFFFF0ull) fail(MYYUV_E_ARG);
  const uint32_t tw = tiles[0]->header.width, th = tiles[0]->header.height;
  std::vector<uint8_t> payload((size_t)total);
  uint32_t size = 0;
  int64_t bad = -1;
  const int rc = myyuv_gpu_dct_join(t_codec.get(), ptrs.data(), sizes.data(), cols, rows, tw, th, payload.data(),
                                    (uint32_t)payload.size(), &size, &bad);
  if (rc) fail(rc);
  return gathered(*tiles[0], cols * tw, rows * th, payload, size);
}

// Many compressed frames per call. Each frame is checked as YUV::decompress
// -> decompress_map[DCT][IYUV] -> decompress_DCT_planar would, in input order
// (frames that are not DCT / IYUV, or fail a check, take that single-frame
// path and its error); the DCT frames of one geometry and quality triple
// then go through one pipelined host batch (myyuv_gpu_dct_decompress_frames)
// straight into their results' planes.
std::vector<myyuv::YUV> decompress_DCT_planar_batch(const std::vector<const myyuv::YUV*>& frames) {
  using myyuv::YUV;
  std::vector<YUV> out(frames.size());
  std::vector<size_t> todo;
  for (size_t i = 0; i < frames.size(); i++) {
    const YUV& y = *frames[i];
    bool batchable = y.getCompression() == YUV::Compressions::DCT && y.getFourccFormat() == YUV::FourccFormats::IYUV &&
                     y.header.compression_params_size == 3 && y.compression_params &&
                     y.getFormatGroup() == YUV::FormatGroup::PLANAR;
    for (int p = 0; batchable && p < 3; p++) batchable = y.compression_params[p] >= 1 && y.compression_params[p] <= 100;
    if (batchable)
      todo.push_back(i);
    else
      out[i] = y.decompress();
  }
  std::vector<bool> done(todo.size(), false);
  for (size_t i = 0; i < todo.size(); i++) {
    if (done[i]) continue;
    const YUV& y0 = *frames[todo[i]];
    const uint32_t w = y0.header.width, hh = y0.header.height;
    const uint8_t* q = y0.compression_params;
    std::vector<size_t> grp;
    for (size_t j = i; j < todo.size(); j++) {
      const YUV& y = *frames[todo[j]];
      if (!done[j] && y.header.width == w && y.header.height == hh && std::memcmp(y.compression_params, q, 3) == 0) {
        grp.push_back(todo[j]);
        done[j] = true;
      }
    }
    std::vector<const uint8_t*> src;
    std::vector<uint32_t> sizes;
    std::vector<uint8_t*> dstp;
    for (size_t k : grp) {
      const YUV& y = *frames[k];
      YUV& res = out[k];  // header rewrite as decompress_DCT_planar (DCT.cpp:446-453)
      res.header = y.header;
      res.header.compression = YUV::Compressions::NONE;
      res.header.compression_params_size = 0;
      res.header.compression_params_pos = 0;
      res.header.data_pos = sizeof(myyuv::YUVHeader);
      res.header.data_size = res.getImageSize();
      res.data = new uint8_t[res.header.data_size];
      src.push_back(y.data);
      sizes.push_back(y.header.data_size);
      dstp.push_back(res.data);
    }
    int64_t bad = -1;
    const int rc = myyuv_gpu_dct_decompress_frames(t_codec.get(), src.data(), sizes.data(), (uint32_t)grp.size(), w,
                                                   hh, q, dstp.data(), &bad);
    if (rc) fail(rc);
  }
  return out;
}

}  // namespace myyuvDCT

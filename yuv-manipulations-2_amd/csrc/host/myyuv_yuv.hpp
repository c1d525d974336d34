// myyuv_yuv.hpp — C++ host surface of the MI355X codec, API-compatible with the
// reference's myyuv::YUV (myyuv_lib/myyuv_yuv.hpp:13-350) for everything on the
// DCT path: the 64-byte header, load/dump, plane geometry, and the codec
// registry (compress_map / decompress_map, myyuv_yuv.hpp:111,116) whose
// [DCT][IYUV] entries here run the HIP kernels through the C ABI
// (include/myyuv_hip.h), and BMP input (bmp_to_yuv_map[IYUV], YUV(const BMP&),
// myyuv_yuv.hpp:106,143,343), whose colour conversion runs on the GPU too
// (K7).  Out of scope: per-pixel access (getPixel).
#pragma once

#include <array>
#include <cstdint>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "myyuv_bmp.hpp"
#include "myyuv_hip.h"

namespace myyuv {

#pragma pack(push, 1)
// On-disk header of a .myyuv file (64 bytes, little endian).
struct YUVHeader {
  uint8_t type[2] = {'Y', 'U'};
  uint32_t fourcc_format = 0;
  uint32_t data_size = 0;            // payload bytes
  uint16_t compression = 0;          // 0 = none, 1 = DCT
  uint32_t compression_params_size = 0;
  uint32_t compression_params_pos = 0;
  uint32_t width = 0;
  uint32_t height = 0;
  uint32_t data_pos = 0;
  uint8_t unused[32] = {0};
};
#pragma pack(pop)
static_assert(sizeof(YUVHeader) == 64, "YUVHeader must be 64 bytes");

class YUV {
 public:
  YUVHeader header;
  uint8_t* compression_params = nullptr;  // owned, new[]
  uint8_t* data = nullptr;                // owned, new[]

  enum class FormatGroup { UNKNOWN = 0, PACKED, PLANAR, SEMI_PLANAR };
  using FourccFormat = uint32_t;
  struct FourccFormats {
    static constexpr const FourccFormat UNKNOWN = 0;
    static constexpr const FourccFormat IYUV = 0x56555949;
  };
  using Compression = uint16_t;
  struct Compressions {
    static constexpr const Compression NONE = 0;
    static constexpr const Compression DCT = 1;
  };
  static constexpr const uint32_t max_planes = 4;
  static constexpr const uint8_t no_plane = 0xff;

  static std::unordered_map<FourccFormat, FormatGroup> yuv_format_group_map;
  static std::unordered_map<FourccFormat, std::array<uint8_t, max_planes>> yuv_order_planes_map;
  static std::unordered_map<FourccFormat, std::array<uint32_t, 2>> yuv_resolution_fraction_map;
  static std::unordered_map<FourccFormat, std::function<YUV(const BMP&)>> bmp_to_yuv_map;
  static std::unordered_map<Compression,
                            std::unordered_map<FourccFormat, std::function<YUV(const YUV&, const void*, uint32_t)>>>
      compress_map;
  static std::unordered_map<Compression, std::unordered_map<FourccFormat, std::function<YUV(const YUV&)>>>
      decompress_map;

  YUV() {}
  explicit YUV(const std::string& path);
  explicit YUV(const BMP& bmp, FourccFormat format);
  YUV(const YUV& yuv);
  YUV& operator=(const YUV& yuv);
  YUV(YUV&& yuv) noexcept;
  YUV& operator=(YUV&& yuv) noexcept;
  ~YUV();

  bool isValid() const noexcept;
  bool isValidHeader() const noexcept;
  static bool isImplementedFormat(FourccFormat format, Compression compression = Compressions::NONE) noexcept;
  FourccFormat getFourccFormat() const noexcept { return header.fourcc_format; }
  Compression getCompression() const noexcept { return header.compression; }
  uint32_t getWidth() const noexcept { return header.width; }
  uint32_t getHeight() const noexcept { return header.height; }
  uint32_t getDataSize() const noexcept { return header.data_size; }
  std::array<uint32_t, 2> getResolutionFraction() const;
  std::array<uint32_t, 2> getWidthHeightChannel(uint8_t channel) const;
  std::array<uint32_t, max_planes> getFormatSizeBits() const;
  std::array<uint8_t, max_planes> getYUVPlanesOrder() const;
  uint32_t getImageSize() const;
  std::array<const uint8_t*, max_planes> getYUVPlanes() const;
  std::array<uint8_t*, max_planes> getYUVPlanes();
  FormatGroup getFormatGroup() const noexcept { return getFormatGroup(getFourccFormat()); }
  static FormatGroup getFormatGroup(FourccFormat format) noexcept;
  YUV compress(Compression compression, const void* params, uint32_t params_size) const;
  YUV decompress() const;
  bool isCompressed() const noexcept { return getCompression() != Compressions::NONE; }
  // PSNR's and block SSIM's integers against `other` (include/myyuv_hip.h,
  // Compare): the three plane records, and with `map` every block's pair in
  // the codec's block order.  Either side may be raw or DCT-compressed; a
  // compressed side is never decoded to memory when the other is raw.  Frames
  // of different size or format: std::runtime_error("Error comparing: the
  // frames differ in size or format").
  myyuv_frame_metric compare(const YUV& other, std::vector<myyuv_block_metric>* map = nullptr) const;
  // Probe and encode to a target (include/myyuv_hip.h) of an uncompressed
  // planar frame.  probe: what the qualities q would cost and give, both
  // parts, no stream written.  compress_to_size: the compressed frame the size
  // bisection finds for a budget of payload_bytes; compress_to_psnr: the one
  // whose every plane keeps at least db dB (NaN: std::runtime_error).  The
  // result's three parameter bytes are the chosen qualities; *result, when
  // given, is filled on success and on failure.  A target out of reach:
  // std::runtime_error("target not reachable").
  myyuv_probe probe(const std::array<uint8_t, 3>& q) const;
  YUV compress_to_size(uint32_t payload_bytes, myyuv_target_result* result = nullptr) const;
  YUV compress_to_psnr(double db, myyuv_target_result* result = nullptr) const;
  // Export to JPEG (include/myyuv_hip.h): the baseline JPEG file of a
  // DCT-compressed planar frame, written from its coefficients.  An
  // uncompressed frame: std::runtime_error("Error exporting: image is not
  // compressed (to_jpeg needs DCT coefficients)"); a malformed stream: the
  // decompressor's messages.  With qualities, on an UNCOMPRESSED planar frame:
  // the file of compress at q, the stream never leaving the device.
  std::vector<uint8_t> to_jpeg() const;
  std::vector<uint8_t> to_jpeg(const std::array<uint8_t, 3>& q) const;
  // Import from JPEG (include/myyuv_hip.h): the DCT-compressed planar frame
  // of a baseline 4:2:0 JPEG file's coefficients, Wp x Hp (the file's
  // MCU-padded grid).  q null: the file's tables are kept (they must be a
  // quality's); else three qualities the coefficients are rescaled to.  A file
  // the import refuses: std::runtime_error with myyuv_hip_error_message's text,
  // before any device is touched.  info, if given: myyuv_jpeg_inspect's.
  static YUV from_jpeg(const std::vector<uint8_t>& file, const uint8_t* q = nullptr, myyuv_jpeg_info* info = nullptr);
  void load(const std::string& path);
  void load(const BMP& bmp, FourccFormat format);
  void dump(const std::string& path) const;
};

// IYUV -> BMP on the GPU (K8; the conversion the reference's viewers draw
// with, defined in include/myyuv_hip.h): a bottom-up BMP (width, height > 0)
// of bit_count 24 or 32 with the headers BMP::dump writes.  chroma: 0 nearest
// sample, 1 bilinear (MYYUV_CHROMA_NEAREST / MYYUV_CHROMA_LINEAR).  An
// uncompressed frame goes through myyuv_gpu_iyuv_to_bmp, a DCT-compressed one
// through myyuv_gpu_dct_decompress_to_bmp (decoded and converted on the device).
BMP yuv_to_bmp(const YUV& yuv, uint16_t bit_count = 32, uint32_t chroma = 1 /* MYYUV_CHROMA_LINEAR */);
// The same for the region (rx, ry, rw, rh) of the frame (luma pixels, top-down,
// multiples of 16, inside the frame: include/myyuv_hip.h, region decode): a
// rw x rh BMP, by definition the conversion of the region's frame.  A
// DCT-compressed frame goes through myyuv_gpu_dct_decompress_region_to_bmp
// (only the region is decoded), an uncompressed one is cropped on the host.
BMP yuv_to_bmp(const YUV& yuv, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh, uint16_t bit_count = 32,
               uint32_t chroma = 1 /* MYYUV_CHROMA_LINEAR */);
// The same for the scaled decode of a DCT-compressed frame (denom 2, 4 or 8:
// include/myyuv_hip.h, scaled decode): a (width/denom) x (height/denom) BMP
// through myyuv_gpu_dct_decompress_scaled_to_bmp.  An uncompressed frame is
// refused (std::runtime_error): there are no coefficients to scale from.
BMP yuv_to_bmp_scaled(const YUV& yuv, uint32_t denom, uint16_t bit_count = 32,
                      uint32_t chroma = 1 /* MYYUV_CHROMA_LINEAR */);
// The region of an UNCOMPRESSED planar frame, rows copied on the host: the
// frame myyuvDCT::decompress_DCT_planar_region returns for the compressed
// form of the same pixels (same constraints, same header, same bytes).
YUV crop_region(const YUV& yuv, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh);

}  // namespace myyuv

namespace myyuvDCT {
// myyuv_DCT/DCT.hpp:16,25 — same signatures, HIP implementation.
myyuv::YUV compress_DCT_planar(const myyuv::YUV& yuv, const std::array<uint8_t, 3>& params);
myyuv::YUV decompress_DCT_planar(const myyuv::YUV& yuv, const std::array<uint8_t, 3>& params);
// Compress from BMP (include/myyuv_hip.h): the same YUV (header, params, data)
// as compress_DCT_planar(YUV(bmp, IYUV), params), through
// myyuv_gpu_bmp_dct_compress: the IYUV frame exists neither here nor on the
// device.  YUV(bmp, IYUV)'s check and message for an invalid BMP, then
// compress_DCT_planar's for the qualities.
myyuv::YUV compress_DCT_planar(const myyuv::BMP& bmp, const std::array<uint8_t, 3>& params);
// Region decode (include/myyuv_hip.h): the rw x rh frame cropped from the full
// decode at (rx, ry), of which only the region's chunks are read.  The quality
// bytes are the frame's compression parameters; the header is
// decompress_DCT_planar's with width = rw, height = rh, data_size = rw*rh*3/2.
myyuv::YUV decompress_DCT_planar_region(const myyuv::YUV& yuv, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh);
// Scaled decode (include/myyuv_hip.h): the (width/denom) x (height/denom)
// frame, denom 2, 4 or 8, from the low-frequency corner of every block.
// decompress_DCT_planar's checks; its header with the scaled size.
myyuv::YUV decompress_DCT_planar_scaled(const myyuv::YUV& yuv, uint32_t denom);
// Requantise (include/myyuv_hip.h): the DCT-compressed frame re-encoded at the
// qualities `params` on its coefficients, no pixels in between.  The source
// qualities are the frame's compression parameters.  decompress_DCT_planar's
// checks and messages for the input (an input that is not DCT-compressed is
// refused); compress_DCT_planar's header with the three new quality bytes.
myyuv::YUV requantize_DCT_planar(const myyuv::YUV& yuv, const std::array<uint8_t, 3>& params);
// Transform (include/myyuv_hip.h): the DCT-compressed frame mirrored, rotated
// or transposed by `op` (MYYUV_XF_*) on its coefficients and re-encoded at the
// qualities `params`, no pixels in between.  Checks, messages and header as
// requantize_DCT_planar; width and height are swapped for a swapping operation.
myyuv::YUV transform_DCT_planar(const myyuv::YUV& yuv, uint32_t op, const std::array<uint8_t, 3>& params);
// Downscale (include/myyuv_hip.h): the DCT-compressed (width/denom) x
// (height/denom) frame, denom 2, 4 or 8, of a DCT-compressed frame, the small
// frame never in memory: compress_DCT_planar(decompress_DCT_planar_scaled(yuv,
// denom), params) bit for bit.  Without `params` the source's own qualities.
// requantize_DCT_planar's checks on the input; compress_DCT_planar's header for
// the scaled size and the destination qualities.
myyuv::YUV downscale_DCT_planar(const myyuv::YUV& yuv, uint32_t denom);
myyuv::YUV downscale_DCT_planar(const myyuv::YUV& yuv, uint32_t denom, const std::array<uint8_t, 3>& params);
// Crop (include/myyuv_hip.h): the w x h rectangle at (x, y) of a DCT-compressed
// frame, still compressed: its blocks' chunk bytes, gathered on the GPU.
// requantize_DCT_planar's checks on the input; compress_DCT_planar's header
// with the new size and the source's quality bytes.
myyuv::YUV crop_DCT_planar(const myyuv::YUV& yuv, uint32_t x, uint32_t y, uint32_t w, uint32_t h);
// Join (include/myyuv_hip.h): cols x rows DCT-compressed tiles (row-major) as
// one compressed frame.  Throws when the tiles' sizes, formats or params
// differ, or their count is not cols * rows.
myyuv::YUV join_DCT_planar(const std::vector<const myyuv::YUV*>& tiles, uint32_t cols, uint32_t rows);
// Many frames per call: frames of one geometry share
// one batched launch of every kernel; result i is compress_DCT_planar(*frames[i]).
std::vector<myyuv::YUV> compress_DCT_planar_batch(const std::vector<const myyuv::YUV*>& frames,
                                                  const std::array<uint8_t, 3>& params);
// The same over several devices: frame i on devices[i % n] (frames sharded
// one per GPU round-robin), one host thread and context per
// entry (an id may repeat: several contexts on one device).
std::vector<myyuv::YUV> compress_DCT_planar_batch(const std::vector<const myyuv::YUV*>& frames,
                                                  const std::array<uint8_t, 3>& params,
                                                  const std::vector<int>& devices);
// Many compressed frames per call: result i is frames[i]->decompress(); the
// DCT frames of one geometry and quality go through one pipelined host batch.
std::vector<myyuv::YUV> decompress_DCT_planar_batch(const std::vector<const myyuv::YUV*>& frames);
}  // namespace myyuvDCT

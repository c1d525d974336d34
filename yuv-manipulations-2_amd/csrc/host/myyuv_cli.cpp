// myyuv_cli.cpp — drop-in for the reference CLI's YUV commands
// (myyuv_cli/main.cpp:138-253) on the MI355X codec:
//   myyuv_cli in.myyuv -info
//   myyuv_cli in.myyuv -compress DCT q [q [q]] -o out.myyuv
//   myyuv_cli in.myyuv -decompress -o out.myyuv
// Same argument rules, quality fill (the last value repeats, main.cpp:64-75),
// same integer-millisecond timing line and "Success!" (main.cpp:11-41, 241),
// same failure mode (usage, then the exception propagates).  BMP input
// (main.cpp:100-136):
//   myyuv_cli in.bmp -info
//   myyuv_cli in.bmp -to_yuv IYUV -o out.myyuv   (conversion on the GPU, K7)
// both steps at once (compress from BMP, include/myyuv_hip.h: the file
// -to_yuv IYUV followed by -compress DCT writes, no IYUV frame in between):
//   myyuv_cli in.bmp -compress DCT q [q [q]] -o out.myyuv
// the way back, which the reference leaves to its viewers (K8; a compressed
// input is decoded and converted on the device):
//   myyuv_cli in.myyuv -to_bmp [24|32] [-chroma nearest|linear] -o out.bmp
// a region of the frame only (region decode, include/myyuv_hip.h: of a
// compressed input only the region's chunks are decoded; an uncompressed
// input is cropped on the host):
//   myyuv_cli in.myyuv -decompress -crop X Y W H -o out.myyuv
//   myyuv_cli in.myyuv -to_bmp [24|32] [-chroma nearest|linear] -crop X Y W H -o out.bmp
// a 1/2, 1/4 or 1/8-size frame of a compressed input (scaled decode,
// include/myyuv_hip.h: the N x N inverse DCT of every block's low-frequency
// corner, on the GPU; not combined with -crop):
//   myyuv_cli in.myyuv -decompress -scale 1/2|1/4|1/8 -o out.myyuv
//   myyuv_cli in.myyuv -to_bmp [24|32] [-chroma nearest|linear] -scale 1/2|1/4|1/8 -o out.bmp
// a compressed input re-encoded at another quality on its coefficients
// (requantise, include/myyuv_hip.h: no pixels in between; the qualities parse
// and fill as -compress DCT's):
//   myyuv_cli in.myyuv -requantize q [q [q]] -o out.myyuv
// a compressed input as a baseline JPEG file written from its coefficients
// (export to JPEG, include/myyuv_hip.h); with -q an uncompressed input,
// compressed at those qualities and exported without the stream leaving the
// device:
//   myyuv_cli in.myyuv -to_jpeg -o out.jpg
//   myyuv_cli raw.myyuv -to_jpeg -q q [q [q]] -o out.jpg
// a baseline 4:2:0 JPEG file read into a compressed image on its coefficients
// (import from JPEG, include/myyuv_hip.h; -q: rescaled to those qualities,
// otherwise the file's tables are kept and must be a quality's):
//   myyuv_cli in.jpg -from_jpeg [-q q [q [q]]] -o out.myyuv
// a compressed input mirrored, rotated or transposed on its coefficients
// (transform, include/myyuv_hip.h; -q: re-encoded at those qualities on the
// way, otherwise at its own):
//   myyuv_cli in.myyuv -transform flip_h|flip_v|rot180|transpose|transverse|rot90|rot270 [-q q [q [q]]] -o out.myyuv
// a compressed input at 1/2, 1/4 or 1/8 size, still compressed (downscale,
// include/myyuv_hip.h: the stream compress would write for the scaled decode,
// the small frame never in memory; -q: at those qualities, otherwise its own):
//   myyuv_cli in.myyuv -downscale 1/2|1/4|1/8 [-q q [q [q]]] -o out.myyuv
// a rectangle of a compressed input, still compressed, and a grid of
// compressed tiles as one compressed image (crop and join, include/myyuv_hip.h:
// byte gathers of the chunks, nothing decoded; -crop directly after the image
// is this command, after -decompress or -to_bmp it is their option):
//   myyuv_cli in.myyuv -crop X Y W H -o out.myyuv
//   myyuv_cli -join COLS ROWS -o out.myyuv tile.myyuv...   (COLS * ROWS files, row-major)
// how far two images of one size are from each other (compare,
// include/myyuv_hip.h: PSNR and 8x8-block SSIM per plane, on the GPU; a
// compressed side against a raw one is never decoded to memory):
//   myyuv_cli a.myyuv -compare b.myyuv [-o report.txt]
// the quality found for a target instead of given (probe and encode to a
// target, include/myyuv_hip.h: BYTES is the output file's size; each prints
// `quality Y U V : size N : psnr y u v dB : P probes` first), and what given
// qualities would cost and give, nothing written:
//   myyuv_cli in.myyuv -compress DCT -target_size BYTES -o out.myyuv
//   myyuv_cli in.myyuv -compress DCT -target_psnr DB -o out.myyuv
//   myyuv_cli in.myyuv -probe q [q [q]]
// and, beyond the reference CLI, many frames per invocation (SURVEY.md §8f
// row 2; frames of one geometry share batched kernel launches):
//   myyuv_cli -batch-compress DCT Q [Q [Q]] [-devices D0,D1,...] -o OUTDIR IN.myyuv...
//     (-devices: frames dealt round-robin over those GPUs, one host thread each)
//   myyuv_cli -batch-decompress -o OUTDIR IN.myyuv...
// each output is OUTDIR/<input file name>, byte-identical to the per-file
// command's.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "myyuv_yuv.hpp"

namespace {

float elapsed_ms(const std::function<void()>& f) {
  const auto t0 = std::chrono::high_resolution_clock::now();
  f();
  const auto t1 = std::chrono::high_resolution_clock::now();
  return (float)std::chrono::duration_cast<std::chrono::milliseconds>(t1 - t0).count();
}

void usage() {
  std::cout << "myyuv_cli (MI355X DCT codec): inspect and DCT-compress/decompress .myyuv images.\n"
            << "Usage:\n"
            << "  myyuv_cli IMAGE.myyuv -info\n"
            << "  myyuv_cli IMAGE.myyuv -compress DCT Q [Q [Q]] -o OUT.myyuv   (Q in 1..100, per plane Y U V)\n"
            << "  myyuv_cli IMAGE.myyuv -compress DCT -target_size BYTES -o OUT.myyuv\n"
            << "  myyuv_cli IMAGE.myyuv -compress DCT -target_psnr DB -o OUT.myyuv\n"
            << "      (the quality found on the GPU: OUT.myyuv of at most BYTES, or every plane at least DB dB)\n"
            << "  myyuv_cli IMAGE.myyuv -probe Q [Q [Q]]\n"
            << "      (the size and the PSNR those qualities would give; nothing is written)\n"
            << "  myyuv_cli IMAGE.myyuv -decompress [-crop X Y W H] -o OUT.myyuv\n"
            << "  myyuv_cli IMAGE.myyuv -to_bmp [24|32] [-chroma nearest|linear] [-crop X Y W H] -o OUT.bmp\n"
            << "      (-crop: only that region, luma pixels from the top-left, multiples of 16)\n"
            << "  myyuv_cli IMAGE.myyuv -decompress -scale 1/2|1/4|1/8 -o OUT.myyuv\n"
            << "  myyuv_cli IMAGE.myyuv -to_bmp [24|32] [-chroma nearest|linear] -scale 1/2|1/4|1/8 -o OUT.bmp\n"
            << "      (-scale: a compressed image at that size, straight from its DCT coefficients)\n"
            << "  myyuv_cli IMAGE.myyuv -requantize Q [Q [Q]] -o OUT.myyuv\n"
            << "      (a compressed image at another quality, straight from its DCT coefficients)\n"
            << "  myyuv_cli IMAGE.myyuv -to_jpeg [-q Q [Q [Q]]] -o OUT.jpg\n"
            << "      (a baseline JPEG straight from a compressed image's DCT coefficients; -q: an uncompressed\n"
            << "       image, compressed at those qualities and exported on the GPU)\n"
            << "  myyuv_cli IMAGE.jpg -from_jpeg [-q Q [Q [Q]]] -o OUT.myyuv\n"
            << "      (a compressed image straight from a baseline 4:2:0 JPEG's DCT coefficients; -q: rescaled to\n"
            << "       those qualities, otherwise the file's own tables are kept)\n"
            << "  myyuv_cli IMAGE.myyuv -transform flip_h|flip_v|rot180|transpose|transverse|rot90|rot270"
               " [-q Q [Q [Q]]] -o OUT.myyuv\n"
            << "      (a compressed image mirrored, rotated or transposed, straight from its DCT coefficients)\n"
            << "  myyuv_cli IMAGE.myyuv -downscale 1/2|1/4|1/8 [-q Q [Q [Q]]] -o OUT.myyuv\n"
            << "      (a compressed image at that size, still compressed, straight from its DCT coefficients)\n"
            << "  myyuv_cli IMAGE.myyuv -crop X Y W H -o OUT.myyuv\n"
            << "      (a compressed image's rectangle, still compressed: its chunks, untouched)\n"
            << "  myyuv_cli -join COLS ROWS -o OUT.myyuv TILE.myyuv...\n"
            << "      (COLS x ROWS compressed tiles of one size and quality, row-major, as one compressed image)\n"
            << "  myyuv_cli IMAGE.myyuv -compare OTHER.myyuv [-o REPORT.txt]\n"
            << "      (PSNR and 8x8-block SSIM per plane between two images of one size, compressed or not)\n"
            << "  myyuv_cli IMAGE.bmp -info\n"
            << "  myyuv_cli IMAGE.bmp -to_yuv IYUV -o OUT.myyuv\n"
            << "  myyuv_cli IMAGE.bmp -compress DCT Q [Q [Q]] -o OUT.myyuv\n"
            << "      (-to_yuv IYUV and -compress DCT in one pass on the GPU, the same file)\n"
            << "  myyuv_cli -batch-compress DCT Q [Q [Q]] [-devices D0,D1,...] -o OUTDIR IMAGE.myyuv...\n"
            << "  myyuv_cli -batch-decompress -o OUTDIR IMAGE.myyuv...\n"
            << "\nYUV formats:\nIYUV\n\nCompression formats for YUV:\nDCT\n"
            << "\nExample:\n  myyuv_cli image.myyuv -compress DCT 50 -o image-DCT-50.myyuv\n";
}

constexpr const char* kCropHelp = "Invalid argument, -crop must be followed by four numbers `X Y W H`\n";

// `-crop X Y W H` at args[a]: four unsigned decimal numbers into r, a moved
// past them.  false: fewer than four, or one that is not a 32-bit number.
bool parse_crop(const std::vector<std::string>& args, size_t& a, uint32_t r[4]) {
  if (a + 4 >= args.size()) return false;
  for (int i = 0; i < 4; i++) {
    const std::string& v = args[a + 1 + i];
    if (v.empty() || v.size() > 10 || v.find_first_not_of("0123456789") != std::string::npos) return false;
    const unsigned long long x = std::stoull(v);
    if (x > 0xFFFFFFFFull) return false;
    r[i] = (uint32_t)x;
  }
  a += 5;
  return true;
}

constexpr const char* kScaleHelp = "Invalid argument, -scale must be followed by `1/2`, `1/4` or `1/8`\n";
constexpr const char* kScaleCropHelp = "Invalid arguments, -scale and -crop cannot be combined\n";
constexpr const char* kScaleRawHelp = "Nothing to scale, image is not compressed (-scale needs DCT coefficients)\n";

// `-scale 1/N` among the options of the command at args[a] (before `-o`):
// taken out of args, N into denom (0: no -scale).  Returns a message to
// print before the usage (exit 1), or nullptr.
const char* take_scale(std::vector<std::string>& args, size_t a, uint32_t& denom) {
  denom = 0;
  size_t k = a + 1;
  bool crop = false;
  for (; k < args.size() && args[k] != "-o" && args[k] != "-scale"; k++) crop = crop || args[k] == "-crop";
  if (k >= args.size() || args[k] != "-scale") return nullptr;
  if (k + 1 >= args.size()) return kScaleHelp;
  const std::string& v = args[k + 1];
  if (v == "1/2")
    denom = 2;
  else if (v == "1/4")
    denom = 4;
  else if (v == "1/8")
    denom = 8;
  else
    return kScaleHelp;
  for (size_t j = k + 2; j < args.size() && args[j] != "-o"; j++) crop = crop || args[j] == "-crop";
  if (crop) return kScaleCropHelp;
  args.erase(args.begin() + k, args.begin() + k + 2);
  return nullptr;
}

// One to three DCT qualities, the last one repeated (main.cpp:64-75).
void dct_qualities(const std::vector<std::string>& params, uint8_t q[3]) {
  if (params.size() > 3)
    throw std::runtime_error("Error. Too many compression parameters. Can't be more than 3 parameters.");
  if (params.empty()) throw std::runtime_error("Error. Too few compression parameters. Must be at least one.");
  for (size_t i = 0; i < 3; i++) {
    const int v = std::stoi(params[i < params.size() ? i : params.size() - 1]);
    if (v < 1 || v > 100)
      throw std::runtime_error("Error. Compression parameters for DCT must range between [1..100].");
    q[i] = (uint8_t)v;
  }
}

myyuv::YUV compress_dct(const myyuv::YUV& yuv, const std::vector<std::string>& params) {
  uint8_t q[3];
  dct_qualities(params, q);
  return yuv.compress(myyuv::YUV::Compressions::DCT, q, 3);
}

constexpr const char* kCompareHelp =
    "Invalid argument, -compare must be followed by an image and at most `-o /path/to/report.txt`\n";

// The report of `IMAGE -compare OTHER` (IMAGE is the reference side; the
// figures are symmetric): a line per plane, one for all samples, and the
// block with the lowest SSIM (ties: the first in plane, then block order).
std::string compare_report(const myyuv::YUV& a, const myyuv::YUV& b) {
  std::vector<myyuv_block_metric> map;
  const myyuv_frame_metric m = a.compare(b, &map);
  const uint32_t w = a.getWidth(), h = a.getHeight();
  const uint64_t samples[3] = {(uint64_t)w * h, (uint64_t)w * h / 4, (uint64_t)w * h / 4};
  char line[256];
  auto psnr_text = [](uint64_t sse, uint64_t n) {
    char t[64];
    if (sse == 0)
      std::snprintf(t, sizeof t, "inf");
    else
      std::snprintf(t, sizeof t, "%.6f", myyuv_metric_psnr(sse, n));
    return std::string(t);
  };
  std::string text;
  uint64_t sse = 0, nb = 0;
  int64_t ss = 0;
  for (int p = 0; p < 3; p++) {
    const myyuv_plane_metric& r = m.plane[p];
    std::snprintf(line, sizeof line, "%c: psnr %s dB ssim %.6f sse %llu max %u\n", "YUV"[p],
                  psnr_text(r.sse, samples[p]).c_str(), myyuv_metric_ssim(r.ssim_sum, r.nblocks),
                  (unsigned long long)r.sse, r.max_abs);
    text += line;
    sse += r.sse;
    ss += r.ssim_sum;
    nb += r.nblocks;
  }
  std::snprintf(line, sizeof line, "all: psnr %s dB ssim %.6f\n", psnr_text(sse, (uint64_t)w * h * 3 / 2).c_str(),
                myyuv_metric_ssim(ss, nb));
  text += line;
  size_t k = 0;
  for (size_t i = 1; i < map.size(); i++)
    if (map[i].ssim < map[k].ssim) k = i;
  const size_t ny = (size_t)(w / 8) * (h / 8), nc = (size_t)(w / 16) * (h / 16);
  const int p = k < ny ? 0 : (k < ny + nc ? 1 : 2);
  const size_t local = k - (p == 0 ? 0 : (p == 1 ? ny : ny + nc));
  const size_t bw = p == 0 ? w / 8 : w / 16;
  std::snprintf(line, sizeof line, "worst block: plane %c x %zu y %zu sse %u ssim %.6f\n", "YUV"[p], (local % bw) * 8,
                (local / bw) * 8, map[k].sse, (double)map[k].ssim / 16777216.0);
  text += line;
  return text;
}

// `quality Y U V : size N : psnr y u v dB : P probes` of a probe record: N the
// .myyuv file's size at those qualities (64-byte header, 3 parameter bytes,
// the payload), the planes' PSNR as -compare prints it.
std::string target_line(const uint8_t q[3], const myyuv_probe& at, uint32_t w, uint32_t h, uint32_t probes) {
  const uint64_t samples[3] = {(uint64_t)w * h, (uint64_t)w * h / 4, (uint64_t)w * h / 4};
  std::string text = "quality " + std::to_string(q[0]) + " " + std::to_string(q[1]) + " " + std::to_string(q[2]) +
                     " : size " + std::to_string((uint64_t)at.payload_bytes + sizeof(myyuv::YUVHeader) + 3) + " : psnr";
  for (int p = 0; p < 3; p++) {
    char t[64];
    if (at.metric.plane[p].sse == 0)
      std::snprintf(t, sizeof t, " inf");
    else
      std::snprintf(t, sizeof t, " %.6f", myyuv_metric_psnr(at.metric.plane[p].sse, samples[p]));
    text += t;
  }
  return text + " dB : " + std::to_string(probes) + " probes\n";
}

constexpr const char* kTargetHelp =
    "Invalid argument, -target_size BYTES or -target_psnr DB must be followed by `-o /path/to/new_image.myyuv`\n";

// `-compress DCT -target_size BYTES -o OUT` / `-target_psnr DB -o OUT` at
// args[a]: BYTES is the output file's size (header and parameter bytes
// included).  A target out of reach: one fixed line, exit 1, no file.
int run_target(const myyuv::YUV& yuv, size_t a, const std::vector<std::string>& args) {
  const bool by_size = args[a] == "-target_size";
  if (args.size() != a + 4 || args[a + 2] != "-o") {
    std::cout << kTargetHelp;
    usage();
    return 1;
  }
  const std::string& v = args[a + 1];
  uint32_t budget = 0;
  double db = 0;
  if (by_size) {
    if (v.empty() || v.size() > 10 || v.find_first_not_of("0123456789") != std::string::npos) {
      std::cout << kTargetHelp;
      usage();
      return 1;
    }
    const unsigned long long bytes = std::stoull(v), head = sizeof(myyuv::YUVHeader) + 3;
    budget = bytes < head ? 0u : (bytes - head > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(bytes - head));
  } else {
    size_t used = 0;
    try {
      db = std::stod(v, &used);
    } catch (const std::exception&) {
      used = 0;
    }
    if (used != v.size() || db != db) {
      std::cout << kTargetHelp;
      usage();
      return 1;
    }
  }
  myyuv::YUV out;
  myyuv_target_result res;
  std::memset(&res, 0, sizeof(res));
  bool unreachable = false;
  const float ms = elapsed_ms([&] {
    try {
      out = by_size ? yuv.compress_to_size(budget, &res) : yuv.compress_to_psnr(db, &res);
    } catch (const std::runtime_error& e) {
      if (std::string(e.what()) != myyuv_hip_error_message(MYYUV_E_TARGET)) throw;
      unreachable = true;
    }
  });
  if (unreachable) {
    std::cout << "Error compressing: " << myyuv_hip_error_message(MYYUV_E_TARGET) << '\n';
    return 1;
  }
  std::cout << target_line(res.quality, res.at, yuv.getWidth(), yuv.getHeight(), res.probes);
  std::cout << "YUV DCT compression (" << (by_size ? " -target_size " : " -target_psnr ") << v << " ) : " << ms
            << " ms\n";
  out.dump(args[a + 3]);
  return 0;
}

int run_yuv(const myyuv::YUV& yuv, size_t a, const std::vector<std::string>& args_in) {
  std::vector<std::string> args = args_in;
  const std::string cmd = args[a];
  uint32_t denom = 0;  // -scale 1/denom (0: none), taken out of args
  if (cmd == "-decompress" || cmd == "-to_bmp") {
    if (const char* msg = take_scale(args, a, denom)) {
      std::cout << msg;
      usage();
      return 1;
    }
    if (denom && !yuv.isCompressed()) {
      std::cout << kScaleRawHelp;
      return 1;
    }
  }
  if (cmd == "-info") {
    const auto& h = yuv.header;
    std::cout << "Type: " << h.type[0] << h.type[1] << '\n'
              << "FourCC Format: 0x" << std::hex << h.fourcc_format << std::dec << '\n'
              << "File size: " << (sizeof(h) + h.compression_params_size + h.data_size) << '\n'
              << "Data size: " << h.data_size << '\n'
              << "Compression: " << h.compression << '\n'
              << "Compression params size: " << h.compression_params_size << '\n'
              << "Width: " << h.width << '\n'
              << "Height: " << h.height << '\n'
              << "Valid: " << yuv.isValid() << '\n';
    return 0;
  }
  if (cmd == "-compress") {
    a++;
    if (a >= args.size()) {
      std::cout << "Invalid arguments. Specify compression algorithm, compression parameters and output.\n";
      usage();
      return 1;
    }
    const std::string algo = args[a++];
    if (algo != "DCT") throw std::runtime_error("Compression not registered: " + algo);
    if (a < args.size() && (args[a] == "-target_size" || args[a] == "-target_psnr")) return run_target(yuv, a, args);
    std::vector<std::string> params;
    while (a < args.size() && args[a] != "-o") params.push_back(args[a++]);
    a++;
    if (a >= args.size()) {
      std::cout << "Invalid argument, last arguments must be `-o /path/to/new_image.myyuv`\n";
      usage();
      return 1;
    }
    std::string label = " ";
    for (const auto& p : params) label += p + " ";
    myyuv::YUV out;
    const float ms = elapsed_ms([&] { out = compress_dct(yuv, params); });
    std::cout << "YUV DCT compression (" << label << ") : " << ms << " ms\n";
    out.dump(args[a]);
    return 0;
  }
  if (cmd == "-probe") {  // Q [Q [Q]]: what those qualities would cost and give, nothing written
    const std::vector<std::string> params(args.begin() + a + 1, args.end());
    uint8_t q[3];
    dct_qualities(params, q);
    myyuv_probe at;
    const float ms = elapsed_ms([&] { at = yuv.probe({q[0], q[1], q[2]}); });
    std::cout << target_line(q, at, yuv.getWidth(), yuv.getHeight(), 1);
    std::cout << "YUV DCT probe : " << ms << " ms\n";
    return 0;
  }
  if (cmd == "-requantize") {  // Q [Q [Q]] -o OUT.myyuv: the qualities as -compress DCT's
    if (!yuv.isCompressed()) {
      std::cout << "Nothing to requantize, image is not compressed (-requantize needs DCT coefficients)\n";
      return 1;
    }
    a++;
    std::vector<std::string> params;
    while (a < args.size() && args[a] != "-o") params.push_back(args[a++]);
    a++;
    if (a >= args.size() || args.size() != a + 1) {
      std::cout << "Invalid argument, last arguments must be `-o /path/to/new_image.myyuv`\n";
      usage();
      return 1;
    }
    std::string label = " ";
    for (const auto& p : params) label += p + " ";
    myyuv::YUV out;
    const float ms = elapsed_ms([&] {
      uint8_t q[3];
      dct_qualities(params, q);
      out = myyuvDCT::requantize_DCT_planar(yuv, {q[0], q[1], q[2]});
    });
    std::cout << "YUV DCT requantization (" << label << ") : " << ms << " ms\n";
    out.dump(args[a]);
    return 0;
  }
  if (cmd == "-to_jpeg") {  // [-q Q [Q [Q]]] -o OUT.jpg: -q for a raw input (and only then), as -compress DCT's
    a++;
    const bool with_q = a < args.size() && args[a] == "-q";
    std::vector<std::string> params;
    if (with_q) a++;
    while (a < args.size() && args[a] != "-o") params.push_back(args[a++]);
    a++;
    if (a >= args.size() || args.size() != a + 1 || (!with_q && !params.empty())) {
      std::cout << "Invalid argument, last arguments must be `-o /path/to/new_image.jpg`\n";
      usage();
      return 1;
    }
    if (yuv.isCompressed() && with_q) {
      std::cout << "Invalid argument, -to_jpeg takes -q for an uncompressed image only (a compressed one is "
                   "exported at its own qualities; -requantize changes them)\n";
      return 1;
    }
    if (!yuv.isCompressed() && !with_q) {
      std::cout << "Invalid argument, -to_jpeg of an uncompressed image needs `-q Q [Q [Q]]`\n";
      usage();
      return 1;
    }
    std::vector<uint8_t> file;
    const float ms = elapsed_ms([&] {
      if (with_q) {
        uint8_t q[3];
        dct_qualities(params, q);
        file = yuv.to_jpeg({q[0], q[1], q[2]});  // compressed and exported on the device
      } else {
        file = yuv.to_jpeg();
      }
    });
    std::cout << "YUV DCT to JPEG : " << ms << " ms\n";
    std::ofstream f(args[a], std::ios::binary);
    f.write(reinterpret_cast<const char*>(file.data()), (std::streamsize)file.size());
    if (!f) throw std::runtime_error("Error writing " + args[a]);
    return 0;
  }
  if (cmd == "-transform") {  // OP [-q Q [Q [Q]]] -o OUT.myyuv: the qualities as -compress DCT's
    if (!yuv.isCompressed()) {
      std::cout << "Nothing to transform, image is not compressed (-transform needs DCT coefficients)\n";
      return 1;
    }
    a++;
    static const char* const names[8] = {nullptr,     "flip_h", "flip_v", "rot180",
                                         "transpose", "rot90",  "rot270", "transverse"};
    uint32_t op = 0;
    for (uint32_t k = 1; k < 8 && a < args.size(); k++)
      if (args[a] == names[k]) op = k;
    if (!op) {
      std::cout << "Invalid argument, -transform takes flip_h, flip_v, rot180, transpose, transverse, rot90 or "
                   "rot270\n";
      usage();
      return 1;
    }
    a++;
    const bool with_q = a < args.size() && args[a] == "-q";
    std::vector<std::string> params;
    if (with_q) a++;
    while (a < args.size() && args[a] != "-o") params.push_back(args[a++]);
    a++;
    if (a >= args.size() || args.size() != a + 1 || (!with_q && !params.empty())) {
      std::cout << "Invalid argument, last arguments must be `-o /path/to/new_image.myyuv`\n";
      usage();
      return 1;
    }
    std::string label = std::string(" ") + names[op] + " ";
    for (const auto& p : params) label += p + " ";
    myyuv::YUV out;
    const float ms = elapsed_ms([&] {
      uint8_t q[3];
      if (with_q) {
        dct_qualities(params, q);
      } else {  // the image's own (transform_DCT_planar checks their count and range)
        for (int p = 0; p < 3; p++)
          q[p] = yuv.header.compression_params_size == 3 && yuv.compression_params ? yuv.compression_params[p] : 0;
      }
      out = myyuvDCT::transform_DCT_planar(yuv, op, {q[0], q[1], q[2]});
    });
    std::cout << "YUV DCT transform (" << label << ") : " << ms << " ms\n";
    out.dump(args[a]);
    return 0;
  }
  if (cmd == "-downscale") {  // 1/2|1/4|1/8 [-q Q [Q [Q]]] -o OUT.myyuv: the qualities as -compress DCT's
    a++;
    uint32_t den = 0;
    if (a < args.size()) den = args[a] == "1/2" ? 2u : (args[a] == "1/4" ? 4u : (args[a] == "1/8" ? 8u : 0u));
    if (!den) {
      std::cout << "Invalid argument, -downscale must be followed by `1/2`, `1/4` or `1/8`\n";
      usage();
      return 1;
    }
    if (!yuv.isCompressed()) {
      std::cout << "Nothing to downscale, image is not compressed (-downscale needs DCT coefficients)\n";
      return 1;
    }
    a++;
    const bool with_q = a < args.size() && args[a] == "-q";
    std::vector<std::string> params;
    if (with_q) a++;
    while (a < args.size() && args[a] != "-o") params.push_back(args[a++]);
    a++;
    if (a >= args.size() || args.size() != a + 1 || (!with_q && !params.empty())) {
      std::cout << "Invalid argument, last arguments must be `-o /path/to/new_image.myyuv`\n";
      usage();
      return 1;
    }
    std::string label = " 1/" + std::to_string(den) + " ";
    for (const auto& p : params) label += p + " ";
    myyuv::YUV out;
    const float ms = elapsed_ms([&] {
      if (with_q) {
        uint8_t q[3];
        dct_qualities(params, q);
        out = myyuvDCT::downscale_DCT_planar(yuv, den, {q[0], q[1], q[2]});
      } else {  // the image's own (downscale_DCT_planar checks their count and range)
        out = myyuvDCT::downscale_DCT_planar(yuv, den);
      }
    });
    std::cout << "YUV DCT downscale (" << label << ") : " << ms << " ms\n";
    out.dump(args[a]);
    return 0;
  }
  if (cmd == "-crop") {  // X Y W H -o OUT.myyuv: the rectangle, still compressed
    if (!yuv.isCompressed()) {
      std::cout << "Nothing to crop, image is not compressed (-crop keeps DCT chunks; use -decompress -crop)\n";
      return 1;
    }
    uint32_t r[4] = {0, 0, 0, 0};
    if (!parse_crop(args, a, r)) {
      std::cout << kCropHelp;
      usage();
      return 1;
    }
    if (args.size() != a + 2 || args[a] != "-o") {
      std::cout << "Invalid argument, last arguments must be `-o /path/to/new_image.myyuv`\n";
      usage();
      return 1;
    }
    myyuv::YUV out;
    const float ms = elapsed_ms([&] { out = myyuvDCT::crop_DCT_planar(yuv, r[0], r[1], r[2], r[3]); });
    std::cout << "YUV DCT crop (" << r[0] << " " << r[1] << " " << r[2] << " " << r[3] << ") : " << ms << " ms\n";
    out.dump(args[a + 1]);
    return 0;
  }
  if (cmd == "-compare") {  // B.myyuv [-o REPORT.txt]: how far this image is from B
    if (args.size() != a + 2 && !(args.size() == a + 4 && args[a + 2] == "-o")) {
      std::cout << kCompareHelp;
      usage();
      return 1;
    }
    std::string text;
    try {
      const myyuv::YUV other(args[a + 1]);
      if (other.getWidth() != yuv.getWidth() || other.getHeight() != yuv.getHeight() ||
          other.getFourccFormat() != yuv.getFourccFormat()) {
        std::cout << "Nothing to compare, the images differ in size or format\n";
        return 1;
      }
      text = compare_report(yuv, other);
    } catch (const std::exception& e) {  // an unreadable B, a stream that does not decode
      std::cout << "Error comparing: " << e.what() << '\n';
      return 1;
    }
    std::cout << text;
    if (args.size() == a + 4) {
      std::ofstream f(args[a + 3], std::ios::binary);
      f << text;
      if (!f) throw std::runtime_error("Error opening file to write " + args[a + 3]);
    }
    return 0;
  }
  if (cmd == "-decompress") {
    // [-crop X Y W H]: the region only (a compressed image: region decode on
    // the GPU; an uncompressed one: its rows copied on the host)
    const bool crop = a + 1 < args.size() && args[a + 1] == "-crop";
    if (!crop && !yuv.isCompressed()) {
      std::cout << "Nothing to decompress, image is not compressed\n";
      return 1;
    }
    a++;
    uint32_t r[4] = {0, 0, 0, 0};
    if (crop && !parse_crop(args, a, r)) {
      std::cout << kCropHelp;
      usage();
      return 1;
    }
    if (args.size() != a + 2) {
      std::cout << "Invalid arguments amount. " << (a + 2) << " is required\n";
      usage();
      return 1;
    }
    if (args[a] != "-o") {
      std::cout << a << " argument must be `-o` instead of " << args[a] << '\n';
      usage();
      return 1;
    }
    myyuv::YUV out;
    const float ms = elapsed_ms([&] {
      if (denom)
        out = myyuvDCT::decompress_DCT_planar_scaled(yuv, denom);
      else if (!crop)
        out = yuv.decompress();
      else if (yuv.isCompressed())
        out = myyuvDCT::decompress_DCT_planar_region(yuv, r[0], r[1], r[2], r[3]);
      else
        out = myyuv::crop_region(yuv, r[0], r[1], r[2], r[3]);
    });
    if (denom)
      std::cout << "YUV DCT scaled decompression (1/" << denom << ") : " << ms << " ms\n";
    else if (crop)
      std::cout << "YUV crop (" << r[0] << " " << r[1] << " " << r[2] << " " << r[3] << ") : " << ms << " ms\n";
    else
      std::cout << "YUV DCT decompression : " << ms << " ms\n";
    out.dump(args[a + 1]);
    return 0;
  }
  if (cmd == "-to_bmp") {  // [24|32] [-chroma nearest|linear] -o OUT.bmp; the viewer's defaults
    a++;
    uint16_t bits = 32;
    uint32_t chroma = 1;  // MYYUV_CHROMA_LINEAR
    std::string mode = "linear";
    if (a < args.size() && args[a] != "-o" && args[a] != "-chroma" && args[a] != "-crop") {
      if (args[a] != "24" && args[a] != "32") {
        std::cout << "Invalid bit count " << args[a] << ", must be 24 or 32\n";
        usage();
        return 1;
      }
      bits = (uint16_t)std::stoi(args[a++]);
    }
    if (a < args.size() && args[a] == "-chroma") {
      if (a + 1 >= args.size() || (args[a + 1] != "nearest" && args[a + 1] != "linear")) {
        std::cout << "Invalid argument, -chroma must be followed by `nearest` or `linear`\n";
        usage();
        return 1;
      }
      mode = args[a + 1];
      chroma = mode == "linear" ? 1 : 0;
      a += 2;
    }
    uint32_t r[4] = {0, 0, 0, 0};
    const bool crop = a < args.size() && args[a] == "-crop";
    if (crop && !parse_crop(args, a, r)) {
      std::cout << kCropHelp;
      usage();
      return 1;
    }
    if (args.size() != a + 2 || args[a] != "-o") {
      std::cout << "Invalid argument, last arguments must be `-o /path/to/new_image.bmp`\n";
      usage();
      return 1;
    }
    myyuv::BMP out;
    const float ms = elapsed_ms([&] {
      out = denom  ? myyuv::yuv_to_bmp_scaled(yuv, denom, bits, chroma)
            : crop ? myyuv::yuv_to_bmp(yuv, r[0], r[1], r[2], r[3], bits, chroma)
                   : myyuv::yuv_to_bmp(yuv, bits, chroma);
    });
    std::cout << "YUV to BMP (" << bits << " " << mode << (denom ? " 1/" + std::to_string(denom) : std::string())
              << ") : " << ms << " ms\n";
    out.dump(args[a + 1]);
    return 0;
  }
  std::cout << "Invalid command " << cmd << '\n';
  usage();
  return 1;
}

int run_bmp(const myyuv::BMP& bmp, size_t a, const std::vector<std::string>& args) {
  const std::string& cmd = args[a];
  if (cmd == "-info") {
    const auto& h = bmp.header;
    std::cout << "Type: " << h.type[0] << h.type[1] << '\n'
              << "File size: " << h.file_size << '\n'
              << "Data size: " << h.width * h.height * h.bit_count / 8 << '\n'
              << "Width: " << h.width << '\n'
              << "Height: " << h.height << '\n'
              << "Bit count: " << h.bit_count << '\n'
              << "Valid: " << bmp.isValid() << '\n';
    return 0;
  }
  if (cmd == "-to_yuv") {
    if (args.size() != a + 4) {
      std::cout << "Invalid arguments amount. " << (a + 4) << " is required\n";
      usage();
      return 1;
    }
    if (args[a + 1] != "IYUV") throw std::runtime_error("Format is not registered: " + args[a + 1]);
    if (args[a + 2] != "-o") {
      std::cout << (a + 2) << " argument must be `-o` instead of " << args[a + 2] << '\n';
      usage();
      return 1;
    }
    myyuv::YUV out;
    const float ms = elapsed_ms([&] { out = myyuv::YUV(bmp, myyuv::YUV::FourccFormats::IYUV); });
    std::cout << "BMP to YUV (" << args[a + 1] << ") : " << ms << " ms\n";
    out.dump(args[a + 3]);
    return 0;
  }
  if (cmd == "-compress") {  // DCT Q [Q [Q]] -o OUT.myyuv: -to_yuv IYUV and -compress DCT in one GPU pass
    size_t k = a + 1;
    const bool dct = k < args.size() && args[k] == "DCT";
    std::vector<std::string> params;
    for (k++; dct && k < args.size() && args[k] != "-o"; k++) params.push_back(args[k]);
    if (!dct || args.size() != k + 2) {
      std::cout << "Invalid argument, -compress must be followed by `DCT Q [Q [Q]] -o /path/to/new_image.myyuv`\n";
      usage();
      return 1;
    }
    std::string label = " ";
    for (const auto& p : params) label += p + " ";
    myyuv::YUV out;
    const float ms = elapsed_ms([&] {
      uint8_t q[3];
      dct_qualities(params, q);
      out = myyuvDCT::compress_DCT_planar(bmp, {q[0], q[1], q[2]});
    });
    std::cout << "BMP DCT compression (" << label << ") : " << ms << " ms\n";
    out.dump(args[k + 1]);
    return 0;
  }
  std::cout << "Invalid command " << cmd << '\n';
  usage();
  return 1;
}

std::string base_name(const std::string& path) {
  const size_t k = path.find_last_of('/');
  return k == std::string::npos ? path : path.substr(k + 1);
}

// -batch-compress DCT Q [Q [Q]] -o OUTDIR FILES... / -batch-decompress -o OUTDIR FILES...
int run_batch(const std::vector<std::string>& args) {
  const bool comp = args[1] == "-batch-compress";
  size_t a = 2;
  std::vector<std::string> params;
  std::vector<int> devices;
  if (comp) {
    if (a >= args.size() || args[a] != "DCT")
      throw std::runtime_error("Compression not registered: " + (a < args.size() ? args[a] : std::string()));
    a++;
    while (a < args.size() && args[a] != "-o") {
      if (args[a] == "-devices" && a + 1 < args.size()) {  // frames dealt round-robin over these GPUs
        std::string list = args[a + 1];
        for (size_t k = 0; k <= list.size();) {
          const size_t e = list.find(',', k);
          devices.push_back(std::stoi(list.substr(k, e == std::string::npos ? std::string::npos : e - k)));
          if (e == std::string::npos) break;
          k = e + 1;
        }
        a += 2;
        continue;
      }
      params.push_back(args[a++]);
    }
  }
  if (a + 2 >= args.size() || args[a] != "-o") {
    std::cout << "Invalid arguments. Expected -o OUTDIR followed by input files\n";
    usage();
    return 1;
  }
  const std::string outdir = args[a + 1];
  std::vector<myyuv::YUV> in;
  std::vector<std::string> names;
  for (size_t i = a + 2; i < args.size(); i++) {
    names.push_back(base_name(args[i]));
    // outputs are OUTDIR/<input file name>: two inputs with one name would
    // overwrite each other
    for (size_t j = 0; j + 1 < names.size(); j++)
      if (names[j] == names.back())
        throw std::runtime_error("Error. Two batch inputs share the file name " + names.back());
  }
  for (size_t i = a + 2; i < args.size(); i++) in.emplace_back(args[i]);
  std::vector<myyuv::YUV> out;
  const float ms = elapsed_ms([&] {
    if (comp) {
      uint8_t q[3];
      if (params.empty()) throw std::runtime_error("Error. Too few compression parameters. Must be at least one.");
      if (params.size() > 3)
        throw std::runtime_error("Error. Too many compression parameters. Can't be more than 3 parameters.");
      for (size_t i = 0; i < 3; i++) {
        const int v = std::stoi(params[i < params.size() ? i : params.size() - 1]);
        if (v < 1 || v > 100)
          throw std::runtime_error("Error. Compression parameters for DCT must range between [1..100].");
        q[i] = (uint8_t)v;
      }
      std::vector<const myyuv::YUV*> ptrs;
      for (const auto& y : in) ptrs.push_back(&y);
      out = myyuvDCT::compress_DCT_planar_batch(ptrs, {q[0], q[1], q[2]}, devices);
    } else {
      std::vector<const myyuv::YUV*> ptrs;
      for (const auto& y : in) ptrs.push_back(&y);
      out = myyuvDCT::decompress_DCT_planar_batch(ptrs);
    }
  });
  std::cout << (comp ? "YUV DCT batch compression" : "YUV DCT batch decompression") << " (" << in.size()
            << " frames) : " << ms << " ms\n";
  for (size_t i = 0; i < out.size(); i++) out[i].dump(outdir + "/" + names[i]);
  return 0;
}

// -join COLS ROWS -o OUT.myyuv TILE.myyuv...: COLS * ROWS compressed tiles of
// one size and quality, row-major, as one compressed image
int run_join(const std::vector<std::string>& args) {
  auto number = [](const std::string& v, uint32_t& x) {
    if (v.empty() || v.size() > 5 || v.find_first_not_of("0123456789") != std::string::npos) return false;
    x = (uint32_t)std::stoul(v);
    return x > 0;
  };
  uint32_t cols = 0, rows = 0;
  if (args.size() < 4 || !number(args[2], cols) || !number(args[3], rows)) {
    std::cout << "Invalid argument, -join must be followed by two numbers `COLS ROWS`\n";
    usage();
    return 1;
  }
  if (args.size() < 7 || args[4] != "-o") {
    std::cout << "Invalid arguments. Expected -o OUT.myyuv followed by the tiles\n";
    usage();
    return 1;
  }
  if (args.size() - 6 != (size_t)cols * rows) {
    std::cout << "Invalid arguments amount. " << (uint64_t)cols * rows << " tiles are required, " << args.size() - 6
              << " given\n";
    usage();
    return 1;
  }
  std::vector<myyuv::YUV> in;
  for (size_t i = 6; i < args.size(); i++) in.emplace_back(args[i]);
  for (const auto& y : in)
    if (!y.isCompressed()) {
      std::cout << "Nothing to join, a tile is not compressed (-join keeps DCT chunks)\n";
      return 1;
    }
  std::vector<const myyuv::YUV*> ptrs;
  for (const auto& y : in) ptrs.push_back(&y);
  myyuv::YUV out;
  const float ms = elapsed_ms([&] { out = myyuvDCT::join_DCT_planar(ptrs, cols, rows); });
  std::cout << "YUV DCT join (" << cols << " " << rows << ") : " << ms << " ms\n";
  out.dump(args[5]);
  return 0;
}

// IMAGE.jpg -from_jpeg [-q Q [Q [Q]]] -o OUT.myyuv: the qualities as -compress DCT's
int run_jpeg(const std::string& path, const std::vector<std::string>& args) {
  size_t a = 2;
  if (args[a] != "-from_jpeg") {
    std::cout << "Invalid argument, a JPEG image takes `-from_jpeg` only\n";
    usage();
    return 1;
  }
  a++;
  const bool with_q = a < args.size() && args[a] == "-q";
  std::vector<std::string> params;
  if (with_q) a++;
  while (a < args.size() && args[a] != "-o") params.push_back(args[a++]);
  a++;
  if (a >= args.size() || args.size() != a + 1 || (!with_q && !params.empty())) {
    std::cout << "Invalid argument, last arguments must be `-o /path/to/new_image.myyuv`\n";
    usage();
    return 1;
  }
  uint8_t q[3];
  if (with_q) dct_qualities(params, q);
  std::ifstream f(path, std::ios::binary);
  const std::vector<uint8_t> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (!f && !f.eof()) throw std::runtime_error("Error reading " + path);
  myyuv::YUV out;
  myyuv_jpeg_info info;
  const float ms = elapsed_ms([&] { out = myyuv::YUV::from_jpeg(file, with_q ? q : nullptr, &info); });
  std::cout << "JPEG to YUV DCT : " << ms << " ms\n";
  if (info.width != info.padded_width || info.height != info.padded_height)
    std::cout << "Notice: " << info.width << "x" << info.height << " padded to " << info.padded_width << "x"
              << info.padded_height << " (the file's own MCU grid)\n";
  out.dump(args[a]);
  return 0;
}

int run(int argc, char* argv[]) {
  if (argc <= 2) {
    usage();
    return 0;
  }
  const std::vector<std::string> args(argv, argv + argc);
  if (args[1] == "-join") {
    const int rc = run_join(args);
    if (rc == 0) std::cout << "Success!\n";
    return rc;
  }
  if (args[1] == "-batch-compress" || args[1] == "-batch-decompress") {
    const int rc = run_batch(args);
    if (rc == 0) std::cout << "Success!\n";
    return rc;
  }
  const std::string& path = args[1];
  char magic[2] = {0, 0};
  {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("Error opening file to read " + path);
    f.read(magic, 2);
  }
  int rc;
  if (magic[0] == 'Y' && magic[1] == 'U') {
    rc = run_yuv(myyuv::YUV(path), 2, args);
  } else if (magic[0] == 'B' && magic[1] == 'M') {
    rc = run_bmp(myyuv::BMP(path), 2, args);
  } else if ((uint8_t)magic[0] == 0xFF && (uint8_t)magic[1] == 0xD8) {
    rc = run_jpeg(path, args);
  } else {
    throw std::runtime_error("Unknown image format (magic) " + path);
  }
  if (rc == 0) std::cout << "Success!\n";
  return rc;
}

}  // namespace

int main(int argc, char* argv[]) {
  try {
    return run(argc, argv);
  } catch (...) {
    usage();
    throw;
  }
}

/*
 * myyuv_hip.h — C ABI of the MI355X (gfx950) DCT codec: the drop-in boundary
 * for the reference's DCT compress/decompress path.
 *
 * The reference binds this path in two places (paths relative to
 * /root/reference/myyuv_lib/):
 *   - myyuv_yuv.hpp:111,116 / myyuv_yuv.cpp:130-160: YUV::compress_map[DCT][IYUV]
 *     and YUV::decompress_map[DCT][IYUV] (std::function plugin table), and
 *   - myyuv_DCT/DCT.hpp:16,25 (extern-declared at myyuv_yuv.cpp:9-14):
 *     myyuvDCT::compress_DCT_planar / decompress_DCT_planar.
 * Each entry point below says which of those it replaces.  The C++ adapter
 * that re-registers the maps through this ABI is
 * yuv-manipulations-2_amd/csrc/host/myyuv_yuv.cpp.
 *
 * Byte format: the payload handled here is exactly the DCTYUV stream the
 * reference writes after the 64-byte YUVHeader and the 3 quality bytes
 * (DCT.cpp:112-197, Huffman.cpp:279-326): u32 plane_size[3],
 * then per plane u32 nblocks, u32 content_size, u8 chunk_size[nblocks],
 * u8 content[content_size].  Frames are IYUV (4:2:0 planar, Y then U then V).
 *
 * Plain pointers and sizes only; no torch or HIP types in the signatures
 * (streams are passed as void* = hipStream_t).  All functions return 0 or a
 * MYYUV_E_* code; myyuv_hip_strerror() gives the reference's message for it.
 */
#ifndef MYYUV_HIP_H
#define MYYUV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error codes.  The string for each (myyuv_hip_strerror) is the exact
 * std::runtime_error text the reference throws at the cited line. */
#define MYYUV_OK 0
#define MYYUV_E_ARG 1             /* null pointer / bad handle (no reference counterpart) */
#define MYYUV_E_QUALITY 2         /* DCT.cpp:380,440 "Level of quality must be between 1 and 100" */
#define MYYUV_E_WIDTH 3           /* DCT.cpp:281,339 "Error. width % 8 must be 0" */
#define MYYUV_E_HEIGHT 4          /* DCT.cpp:284,342 "Error. height % 8 must be 0" */
#define MYYUV_E_CAPACITY 5        /* output buffer smaller than the payload (no reference counterpart) */
#define MYYUV_E_DCTYUV_SIZE 6     /* DCT.cpp:133,144 "DCTYUV load bad size" */
#define MYYUV_E_PLANE_SIZE 7      /* DCT.cpp:42,54 "DCTYUVPlane load bad size" */
#define MYYUV_E_PLANE_NBLK 8      /* DCT.cpp:48 "DCTYUVPlane load chunks_sizes_size bad size" */
#define MYYUV_E_PLANE_CONTENT 9   /* DCT.cpp:51 "DCTYUVPlane load content_size bad size" */
#define MYYUV_E_BAD_CODE 10       /* Huffman.cpp:121,130 "Huffman bad code" */
#define MYYUV_E_UNKNOWN_SYMBOL 11 /* Huffman.cpp:139 "Huffman unknown symbol" */
#define MYYUV_E_BAD_CHUNK 12      /* malformed chunk header/table (reference: assert / UB) */
#define MYYUV_E_HIP 13            /* HIP runtime failure */
#define MYYUV_E_NO_DEVICE 14      /* no gfx950 device / HIP unavailable */
#define MYYUV_E_BMP_INVALID 15    /* myyuv_yuv.cpp:514 "BMP is invalid" (width % 4, bit_count 0) */
#define MYYUV_E_BMP_SIGN 16       /* myyuv_bmp.cpp:98 "Unaccounted width and height sign" */
#define MYYUV_E_BMP_UNSUPPORTED 17 /* odd height or not 24/32 bpp (reference: assert, myyuv_yuv.cpp:92,97) */

typedef struct myyuv_hip_ctx* myyuv_hip_handle;

/* Context: one per (host thread, device).  Owns a HIP stream and the per-call
 * workspace (grown on demand, never freed inside a call); the host-buffer
 * entry points copy straight from / into the caller's pageable buffers.
 * Reentrant across contexts, as the
 * reference is (SURVEY.md §8b "Threading").  Calls through ONE context share
 * its workspace, so they run in call order even on different streams: a call
 * on a stream other than the previous call's makes its stream wait for the
 * previous call's work (an event recorded at the end of every call).  For
 * concurrency, use one context per stream.
 *
 * Kernel arrangements, read from the environment when the context is created
 * (every arrangement gives the same bytes, codes and block indices):
 *   MYYUV_ENCODER  split (default): K1 -> K2 through HBM; fused: one pass.
 *   MYYUV_DECODER  fused (default): K5 + K6 in one kernel, the coefficients
 *                  kept on chip.  A launch of at least MYYUV_DEC_SPAN_MIN
 *                  64-block groups (frames x groups per frame) runs a wave per
 *                  256-block span, which finishes one-symbol chunks in closed
 *                  form and decodes the rest in passes of 64; a smaller one
 *                  (a single frame has too few spans to fill the device) a
 *                  wave per 64-block group.
 *                  span / group: always the one / the other.
 *                  split: K5 -> K6 through HBM.
 *   MYYUV_DEC_SPAN_MIN  the threshold above, in groups; its default is the
 *                  measured crossover.
 * Region, scaled, requantise, transform, downscale and compare decode are the same
 * kernels under every MYYUV_DECODER. */
int myyuv_hip_create(int device, myyuv_hip_handle* out);
void myyuv_hip_destroy(myyuv_hip_handle h);
const char* myyuv_hip_strerror(int code);
/* The text of every code.  myyuv_hip_strerror's table is closed at code 17
 * (its callers were built against "Unknown error" for everything above);
 * codes added since have their text here, and the codes up to 17 give
 * myyuv_hip_strerror's.  New callers use this one. */
const char* myyuv_hip_error_message(int code);

/* Upper bound of the DCTYUV payload for a WxH IYUV frame (worst-case 160 B per
 * 8x8 block + headers); size the compress output buffer with it. */
uint32_t myyuv_dct_payload_bound(uint32_t width, uint32_t height);

/* Host-buffer compress: replaces myyuvDCT::compress_DCT_planar's data path
 * (DCT.cpp:371-430), i.e. what YUV::compress_map[DCT][IYUV] runs
 * (myyuv_yuv.cpp:132-142).  iyuv = W*H*3/2 bytes (Y, U, V planes as in
 * YUV::getYUVPlanes, myyuv_yuv.cpp:383-423).  Writes the DCTYUV payload to
 * `payload` (capacity `cap`) and its size to *payload_size.  The caller (C++
 * adapter) writes the 64-B header and the 3 quality bytes. */
int myyuv_gpu_dct_compress(myyuv_hip_handle h, const uint8_t* iyuv, uint32_t width,
                           uint32_t height, const uint8_t quality[3], uint8_t* payload,
                           uint32_t cap, uint32_t* payload_size);

/* Host-buffer decompress: replaces myyuvDCT::decompress_DCT_planar's data path
 * (DCT.cpp:432-488), what YUV::decompress_map[DCT][IYUV] runs
 * (myyuv_yuv.cpp:148-158).  Writes W*H*3/2 bytes to `iyuv`.  On a decode error
 * returns its code; *bad_block (optional) receives the global block index
 * (plane-major, row-major blocks) of the first failing block, -1 for header
 * errors.
 *
 * Order of checks (every decompress call; the CPU restatement
 * oracle/myyuv_oracle.c follows it, the reference is undefined past its own
 * load checks):
 *   1. the handle and pointers (MYYUV_E_ARG), then the quality;
 *   2. the whole stream header, before any chunk is looked at: size <= 12 and
 *      12 + ps0 + ps1 + ps2 > size (6), then plane by plane ps <= 8 (7),
 *      chunk-size count 0 (8), content_size 0 (9), 8 + count + content_size >
 *      ps (7), all in 64-bit arithmetic; then the % 8 dimension checks (3, 4);
 *      then, plane by plane, a chunk-size count below the plane's block count
 *      (8).  *bad_block = -1 for all of these;
 *   3. plane by plane: the plane-content check (the chunk sizes of the
 *      plane's blocks sum to more than content_size:
 *      MYYUV_E_PLANE_CONTENT), which fails the plane as a whole, before any
 *      of its chunks; then the plane's chunks in block order (10, 11, 12).
 *      The lowest failing block is reported, whichever kernel lane found it.
 * *bad_block for MYYUV_E_PLANE_CONTENT from step 3 is the first block of the
 * failing plane (the count of blocks in the planes before it), and -1 when
 * that is block 0 of the call's first frame: the device's error key 0 means
 * "no block".  A chunk error in an earlier plane comes first; a chunk error in
 * the same plane, at whatever block, does not.
 *
 * Table limits (step 3's chunk checks, MYYUV_E_BAD_CHUNK): a chunk's Huffman
 * table may hold at most 64 entries per code length, in any number of
 * groups; the total over all lengths is limited only by table_bytes (the
 * reference's Huffman::fromDump has no limit; a message has at most 64
 * symbols, so more than 64 entries of one length cannot all be used). */
int myyuv_gpu_dct_decompress(myyuv_hip_handle h, const uint8_t* payload, uint32_t size,
                             uint32_t width, uint32_t height, const uint8_t quality[3],
                             uint8_t* iyuv, int64_t* bad_block);

/* Device-resident variants (HBM in, HBM out), asynchronous on `stream`
 * (hipStream_t; NULL = the context's stream).  Used by the batch driver and
 * the benchmark: no host synchronisation, no allocation once the workspace
 * has grown to the frame size (call myyuv_hip_reserve first to pre-size it).
 *   compress:   d_iyuv (W*H*3/2 B) -> d_payload (cap B), *d_payload_size (u32, device)
 *   decompress: d_payload + *d_payload_size (device u32) -> d_iyuv
 * Errors found on the device are collected in the context and returned by
 * myyuv_hip_sync_status.  The decompress calls (these, the batch, region and
 * scaled ones) read a stream inside min(size word, cap) only: a size word
 * above cap decodes as the stream cut at cap, and bytes past the size word
 * never matter.  Every stream check of myyuv_gpu_dct_decompress's step 2
 * runs on the device here, in the same order. */
int myyuv_hip_reserve(myyuv_hip_handle h, uint32_t width, uint32_t height);
int myyuv_gpu_dct_compress_device(myyuv_hip_handle h, const void* d_iyuv, uint32_t width,
                                  uint32_t height, const uint8_t quality[3], void* d_payload,
                                  uint32_t cap, uint32_t* d_payload_size, void* stream);
int myyuv_gpu_dct_decompress_device(myyuv_hip_handle h, const void* d_payload,
                                    const uint32_t* d_payload_size, uint32_t cap, uint32_t width,
                                    uint32_t height, const uint8_t quality[3], void* d_iyuv,
                                    void* stream);
/* Batches: `nframes` frames of one geometry per launch of each kernel (the
 * batch configuration of SURVEY.md §8d; fills the GPU where one 4K frame
 * cannot).  Frame f at d_iyuv + f*W*H*3/2; payload f at d_payload + f*cap
 * (cap a multiple of 4 when nframes > 1), its size at d_payload_sizes[f].
 * A device-side error reports the batch-global block index
 * (f * blocks_per_frame + block) of the first failing block; a header error
 * of frame f > 0 reports f * blocks_per_frame.  Each frame's bytes are those
 * of the single-frame call.
 * Workspace (myyuv_hip_reserve_batch reserves it up front; the calls grow it
 * on demand): about 471 B per 8x8 block of the batch — the encoder's stage
 * (160 B: a tile's chunks, kMaxChunk per block, rounded up to whole 4-tile
 * K2 windows) and overflow slots (160 B per block: any block may exceed 8
 * distinct symbols, as nearly all of a noise frame's do, so the slots cannot
 * be sized from a typical list), the coefficients (128 B), the chunk offsets
 * (u32 srcoff, 4 B), the decoder's group offsets (4 B), the overflow worklist
 * (8 B: the CAP-16 tier's list and its rest list), the sizes and row masks
 * (2 B), K1's per-block words for K2 (4 B) and its exact-path list (0.25 B).
 * A 4032x3008 frame (284,256 blocks) takes ~134 MB: the bench's 32-frame
 * launch groups ~4.3 GB per context, its 4 contexts ~17 GB; a 16-frame
 * 8192x8192 batch ~11.9 GB (of 288 GB). */
int myyuv_hip_reserve_batch(myyuv_hip_handle h, uint32_t width, uint32_t height, uint32_t nframes);
int myyuv_gpu_dct_compress_batch_device(myyuv_hip_handle h, const void* d_iyuv, uint32_t nframes,
                                        uint32_t width, uint32_t height, const uint8_t quality[3],
                                        void* d_payload, uint32_t cap, uint32_t* d_payload_sizes,
                                        void* stream);
int myyuv_gpu_dct_decompress_batch_device(myyuv_hip_handle h, const void* d_payload,
                                          const uint32_t* d_payload_sizes, uint32_t cap,
                                          uint32_t nframes, uint32_t width, uint32_t height,
                                          const uint8_t quality[3], void* d_iyuv, void* stream);
/* BMP -> IYUV: replaces YUV(const BMP&, IYUV), i.e.
 * YUV::bmp_to_yuv_map[IYUV] (myyuv_yuv.cpp:88-128) over BMP::colorData
 * (myyuv_bmp.cpp:77-101).  `bmp_data` is BMP::data — the pixel array as stored
 * in the file (BGR or BGRA, bit_count 24 or 32, |width| % 4 == 0 so rows are
 * unpadded); `width` / `height` are the header's signed fields, whose signs
 * select colorData's orientation (height > 0: bottom-up rows; width < 0:
 * pixel order reversed).  Writes |width|*|height|*3/2 IYUV bytes.  The C++
 * adapter checks the rest of BMP::isValidHeader and writes the YUV header. */
int myyuv_gpu_bmp_to_iyuv(myyuv_hip_handle h, const uint8_t* bmp_data, int32_t width,
                          int32_t height, uint16_t bit_count, uint8_t* iyuv);
/* Device-resident variant, asynchronous on `stream` (NULL = the context's);
 * argument errors are returned at once. */
int myyuv_gpu_bmp_to_iyuv_device(myyuv_hip_handle h, const void* d_bmp_data, int32_t width,
                                 int32_t height, uint16_t bit_count, void* d_iyuv, void* stream);

/* IYUV -> BMP: the inverse of the above, and the headless form of what the
 * reference's viewers do when they draw a frame (myyuv_opengl/viewer/
 * frag_yuv.glsl over GL_LINEAR, clamp-to-edge plane textures,
 * myyuv_opengl_shared.cpp:109-121; myyuv_sdl3/main.cpp:39-50).  No reference
 * program emits these bytes, so the definition is stated here: the shader's
 * arithmetic in fp32, left to right, no FMA contraction, then the UNORM8
 * framebuffer write.  For luma pixel (x, y) of a WxH frame, rows top-down,
 * Wc = W/2, Hc = H/2:
 *   chroma NEAREST: su = 16 * U[y>>1][x>>1]; sv likewise.
 *   chroma LINEAR (GL_LINEAR + CLAMP_TO_EDGE at 1:1):
 *     cx = x>>1, nx = clamp(x odd ? cx+1 : cx-1, 0, Wc-1); cy, ny likewise in
 *     y, clamped to [0, Hc-1];
 *     su = 9*U[cy][cx] + 3*U[cy][nx] + 3*U[ny][cx] + U[ny][nx]  (0..4080); sv
 *     likewise.  The clamp is per frame: in a batch a neighbour never comes
 *     from another frame or plane.
 *   yf = (float)Y / 255.0f
 *   uf = (float)su / 4080.0f - 0.5f;  vf = (float)sv / 4080.0f - 0.5f
 *   r = yf + 1.403f*vf;  g = (yf - 0.714f*vf) - 0.344f*uf;  b = yf + 1.773f*uf
 *   byte = (uint8_t)floorf(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f + 0.5f)
 * Faithful to the shader, mid-grey is not neutral: (Y, U, V) = (128, 128, 128)
 * gives (B, G, R) = (129, 127, 129).  Under LINEAR green depends on the order
 * of the two subtractions and on their products not being fused; the kernel
 * keeps both.
 * Output: the pixel array of a BMP whose header carries `width` / `height`
 * (signed, the conventions and checks of myyuv_gpu_bmp_to_iyuv: the inverse
 * of BMP::colorData, myyuv_bmp.cpp:80-103, so feeding the result back with
 * the same signs sees the pixels top-down); B, G, R per pixel for bit_count
 * 24 and B, G, R, 0xFF for 32; |width|*|height|*bit_count/8 bytes.  `iyuv`
 * is |width|*|height|*3/2 bytes.  Errors: MYYUV_E_BMP_INVALID (|width| % 4,
 * bit_count 0: BMP::isValidHeader must accept the result), MYYUV_E_BMP_SIGN,
 * MYYUV_E_BMP_UNSUPPORTED (odd height, not 24/32 bpp), MYYUV_E_ARG (a chroma
 * mode other than the two below; more than 4 GiB of BGRA). */
#define MYYUV_CHROMA_NEAREST 0
#define MYYUV_CHROMA_LINEAR 1
int myyuv_gpu_iyuv_to_bmp(myyuv_hip_handle h, const uint8_t* iyuv, int32_t width, int32_t height,
                          uint16_t bit_count, uint32_t chroma, uint8_t* bmp_data);
/* Device-resident variant for `nframes` frames of one geometry (frame f at
 * d_iyuv + f*W*H*3/2 -> d_bmp_data + f*W*H*bit_count/8), asynchronous on
 * `stream` (NULL = the context's), no allocation; argument errors are
 * returned at once.  d_iyuv is 4-byte aligned, d_bmp_data 16-byte (32 bpp) or
 * 4-byte (24 bpp) aligned: a misaligned pointer, like nframes == 0, is
 * MYYUV_E_ARG (after the errors listed above).
 * These two calls check every other argument before the handle (a null
 * handle is MYYUV_E_ARG last), so the argument errors can be had without a
 * device; the two decompress_to_bmp calls below check the handle first, as
 * the decompress calls do. */
int myyuv_gpu_iyuv_to_bmp_device(myyuv_hip_handle h, const void* d_iyuv, uint32_t nframes, int32_t width,
                                 int32_t height, uint16_t bit_count, uint32_t chroma, void* d_bmp_data,
                                 void* stream);
/* Decode and convert, the IYUV frame staying in HBM: myyuv_gpu_dct_decompress
 * (same stream checks, errors and *bad_block, in the same order) followed by
 * myyuv_gpu_iyuv_to_bmp (its argument errors come after the stream header's
 * and before the % 8 dimension checks, which |width| and |height| must pass
 * too). */
int myyuv_gpu_dct_decompress_to_bmp(myyuv_hip_handle h, const uint8_t* payload, uint32_t size, int32_t width,
                                    int32_t height, const uint8_t quality[3], uint16_t bit_count,
                                    uint32_t chroma, uint8_t* bmp_data, int64_t* bad_block);

/* Region decode: a rectangle of a compressed frame without decoding the rest.
 * For a WxH frame and a region (rx, ry, rw, rh) in luma pixels, top-down frame
 * coordinates, the result is the rw x rh IYUV frame
 *   Y' = Y[ry : ry+rh, rx : rx+rw]
 *   U' = U[ry/2 : (ry+rh)/2, rx/2 : (rx+rw)/2], V' likewise
 * of the full decode, laid out as any IYUV frame (Y', U', V'; rw*rh*3/2
 * bytes): byte for byte the crop of myyuv_gpu_dct_decompress's output.
 * rx, ry, rw and rh are multiples of 16 (the reference's compress
 * precondition for frames: every plane's rectangle is whole 8x8 blocks and
 * the result is itself a compressible frame), rw, rh > 0, rx+rw <= W and
 * ry+rh <= H (no 32-bit wrap); anything else is MYYUV_E_ARG.
 * Checks and errors: the handle, pointer, quality, stream-header and % 8
 * dimension checks of myyuv_gpu_dct_decompress, in its order, then the
 * region's.  The chunk-size table of the whole frame is still scanned (its
 * prefix sums place the region's chunks), so header errors are unchanged; of
 * the chunks only the region's are read.  A malformed chunk OUTSIDE the region
 * is therefore not reported and the region decodes: that is the point of the
 * call, not an omission.  A malformed chunk inside it gives the full decode's
 * code, *bad_block its index in the FULL frame's numbering (plane-major,
 * row-major), the lowest such index when there are several; the
 * plane-content check (MYYUV_E_PLANE_CONTENT) applies to the region's blocks.
 * Workspace: 4 B per block of the full frame (the scan), nothing of the
 * 471 B per block the other calls reserve.  The host-buffer forms copy the
 * whole payload to the device and rw*rh*3/2 (or the region's BMP) bytes back. */
int myyuv_gpu_dct_decompress_region(myyuv_hip_handle h, const uint8_t* payload, uint32_t size,
                                    uint32_t width, uint32_t height, const uint8_t quality[3],
                                    uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh,
                                    uint8_t* iyuv, int64_t* bad_block);
/* Device-resident batch: stream f at d_payload + f*cap (cap a multiple of 4
 * when nframes > 1, its size at d_payload_sizes[f]) -> region frame f at
 * d_iyuv + f*rw*rh*3/2; one region for all frames; asynchronous on `stream`
 * (NULL = the context's); argument errors are returned at once, device-side
 * errors through myyuv_hip_sync_status (batch-global block index
 * f * blocks_per_frame + block, blocks of the full frame). */
int myyuv_gpu_dct_decompress_region_device(myyuv_hip_handle h, const void* d_payload,
                                           const uint32_t* d_payload_sizes, uint32_t cap, uint32_t nframes,
                                           uint32_t width, uint32_t height, const uint8_t quality[3],
                                           uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh,
                                           void* d_iyuv, void* stream);
/* Region decode and K8 on the device: by definition myyuv_gpu_iyuv_to_bmp of
 * the region's frame.  width / height are signed as in
 * myyuv_gpu_dct_decompress_to_bmp: their magnitudes are the frame's size,
 * their signs the orientation of the BMP written; the region is unsigned,
 * in top-down frame coordinates; the output is rw x rh pixels
 * (rw*rh*bit_count/8 bytes).  Under MYYUV_CHROMA_NEAREST this is the crop of
 * the full frame's picture.  Under MYYUV_CHROMA_LINEAR the chroma clamp is
 * at the REGION's edge, so the outermost ring of pixels can differ from the
 * full picture's.  Errors as myyuv_gpu_dct_decompress_to_bmp, then the
 * region's. */
int myyuv_gpu_dct_decompress_region_to_bmp(myyuv_hip_handle h, const uint8_t* payload, uint32_t size,
                                           int32_t width, int32_t height, const uint8_t quality[3],
                                           uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh,
                                           uint16_t bit_count, uint32_t chroma, uint8_t* bmp_data,
                                           int64_t* bad_block);

/* Scaled decode: a 1/2, 1/4 or 1/8-size frame straight from the DCT stream,
 * as JPEG-family decoders do inside the inverse transform (libjpeg's
 * scale_denom): an N x N inverse DCT of the low-frequency corner gives an
 * N x N picture of each 8x8 block.  No reference program emits these bytes, so
 * the definition is stated here, bit for bit.
 *
 * denom in {2, 4, 8} and N = 8 / denom in {4, 2, 1}.
 *
 * For a WxH frame the result is an IYUV frame of (W/denom)x(H/denom): Y', U',
 * V', in W*H*3/2 / denom^2 bytes.  Block (by, bx) of plane p fills rows
 * by*N .. by*N+N-1 and columns bx*N .. bx*N+N-1 of plane p'.  Plane p' is
 * (pw/8*N) wide.  Every frame the full decoder accepts has whole blocks in
 * every plane, so every such frame is accepted for every denom.
 *
 * Per block, with z[u][v] the decoded int16 coefficient in natural order and
 * Q the plane's table as the full decoder builds it:
 *   - Z[u][v] = (float)z[u][v] * Q[u][v] for u, v < N.  Coefficients outside
 *     the corner are ignored.
 *   - B_N is the N-point basis with the 8-point norm: B_N[k][i] =
 *     fp32(sqrt(N/8) * a_k * cos((2i+1)k*pi/2N)), a_0 = sqrt(1/N), a_k =
 *     sqrt(2/N).  As literals, computed in double and rounded once:
 *       c = 0x1.6a09e6p-2f.  This is the reference's DCT_matrix8[0],
 *         0.3535533845424652.
 *       B_1 = {c}.
 *       B_2 = {c, c; c, -c}.
 *       With s = 0x1.d906bcp-2f and t = 0x1.87de2ap-3f,
 *       B_4 = {c, c, c, c; s, t, -t, -s; c, -c, -c, c; t, -s, s, -t}.
 *   - U = B_N^T * Z then R = U * B_N, in the reference's loop order and
 *     arithmetic (squareMatrixMulT2<N>, squareMatrixMul<N>).  Every sum starts
 *     at +0.0f, loops run i, k, j, products and sums are rounded separately,
 *     and there is no FMA.
 *   - pixel = clamp((int)roundf(R[i][j]) + 128, 0, 255), as in restoreDCTPlane.
 *
 * For N = 1 this is literally the full decoder's DC-only arithmetic.  A frame
 * whose blocks are all DC-only therefore has a 1/8 decode equal to any one
 * pixel of each block of its full decode.
 *
 * The arithmetic is yuv-manipulations-2_amd/csrc/idct_scaled.h, shared by the
 * kernel and the host check.  The whole chunk of every block is decoded for
 * every denom, so a malformed stream gives exactly myyuv_gpu_dct_decompress's
 * code and *bad_block.
 * Checks and errors: those of myyuv_gpu_dct_decompress, in its order, then
 * denom not in {2, 4, 8}: MYYUV_E_ARG.
 * Workspace: 132 B per 8x8 block of the batch — the scan (4 B) and the
 * coefficient buffer (128 B), which only blocks with a Huffman table the
 * encoder never writes pass through; nothing else of the 471 B per block the
 * full calls reserve.  The host-buffer forms copy the whole payload to the
 * device and the scaled frame (or its BMP) back. */
int myyuv_gpu_dct_decompress_scaled(myyuv_hip_handle h, const uint8_t* payload, uint32_t size,
                                    uint32_t width, uint32_t height, const uint8_t quality[3],
                                    uint32_t denom, uint8_t* iyuv, int64_t* bad_block);
/* Device-resident batch: stream f at d_payload + f*cap (cap a multiple of 4
 * when nframes > 1, its size at d_payload_sizes[f]) -> scaled frame f at
 * d_iyuv + f*(W*H*3/2/denom^2); d_payload and d_iyuv 4-byte aligned;
 * asynchronous on `stream` (NULL = the context's); argument errors are
 * returned at once, device-side errors through myyuv_hip_sync_status
 * (batch-global block index f * blocks_per_frame + block). */
int myyuv_gpu_dct_decompress_scaled_device(myyuv_hip_handle h, const void* d_payload,
                                           const uint32_t* d_payload_sizes, uint32_t cap, uint32_t nframes,
                                           uint32_t width, uint32_t height, const uint8_t quality[3],
                                           uint32_t denom, void* d_iyuv, void* stream);
/* Scaled decode and K8 on the device, the scaled frame staying in HBM: by
 * definition myyuv_gpu_iyuv_to_bmp of the scaled frame, with the signed
 * header fields width/denom and height/denom (width / height: signed as in
 * myyuv_gpu_dct_decompress_to_bmp, magnitudes the full frame's size); the
 * output is (|width|/denom)*(|height|/denom)*bit_count/8 bytes.  Checks: the
 * handle, pointers, chroma mode, quality, stream header and the % 8 dimension
 * checks on |width| and |height|, then denom, then K8's own argument errors
 * for the SCALED size (e.g. MYYUV_E_BMP_INVALID when |width|/denom is not a
 * multiple of 4). */
int myyuv_gpu_dct_decompress_scaled_to_bmp(myyuv_hip_handle h, const uint8_t* payload, uint32_t size,
                                           int32_t width, int32_t height, const uint8_t quality[3],
                                           uint32_t denom, uint16_t bit_count, uint32_t chroma,
                                           uint8_t* bmp_data, int64_t* bad_block);

/* Requantise: re-encode a DCT stream at another quality without going through
 * pixels — the quality ladder (store a q90 master, hand out its q50 stream).
 * Every block of the format stands alone (no DC prediction, a Huffman table
 * per chunk), so the work is done on coefficients: each block is
 * Huffman-decoded, its 64 coefficients are rescaled from the source quality's
 * table to the destination's, and the blocks are encoded again.  No inverse
 * or forward transform runs, no frame exists in HBM, and no second generation
 * of pixel rounding and clamping is added.  No reference program emits these
 * bytes, so the definition is stated here, bit for bit.
 *
 * For every block of every plane p, z[u][v] is the decoded int16 coefficient
 * in natural order; Qs and Qd are plane p's tables for q_src[p] and q_dst[p]
 * as the codec builds them (make_qtable: integers 1..255 held as floats):
 *   t        = ((float)z[u][v] * Qs[u][v]) / Qd[u][v]   fp32 multiply, then IEEE fp32 divide
 *   z'[u][v] = clamp((int)roundf(t), -1024, 1023)       half away from zero, as applyDCTBlock
 *   - The product is an exact integer below 2^24.
 *   - The divide is the correctly rounded one, not a multiply by 1/Q: the
 *     rule of the compressor's exact path.
 *   - The clamp is part of the definition: 1023 * 255 / 1 does not fit the
 *     chunk format's 11 bits.
 * The output stream is the reference encoder's stream of the blocks z' (what
 * myyuv_gpu_huff_encode_blocks writes for them, laid out as
 * myyuv_gpu_dct_compress lays a frame's chunks out).  Plane order, block
 * order and the planes' block counts are the source's.
 *
 * Two consequences:
 *   - Qd == Qs gives z' == z, so a stream the reference encoder (or this one)
 *     wrote comes back byte for byte.  A valid stream with Huffman tables the
 *     encoder never writes comes back as the encoder's stream of the same
 *     coefficients.
 *   - The result is in general NOT the bytes of compress(decompress(x),
 *     q_dst): that is intended, not an omission.
 *
 * The arithmetic is yuv-manipulations-2_amd/csrc/requant.h, shared by the
 * kernel and the host check.
 * Checks and errors: those of myyuv_gpu_dct_decompress, in its order, with
 * q_src as the quality (`out` and `out_size` among the pointers); then q_dst
 * (MYYUV_E_QUALITY).  A source-stream error gives exactly
 * myyuv_gpu_dct_decompress's code and *bad_block; the frame's output bytes
 * are then unspecified, but stay inside `cap`.  A result larger than `cap` is
 * MYYUV_E_CAPACITY, as compress reports it, with *out_size the size needed;
 * size `cap` with myyuv_dct_payload_bound.  `payload` and `out` must not
 * overlap.
 * Workspace: the compress calls' (about 471 B per 8x8 block); no frame
 * buffer.  The host-buffer form copies the source stream to the device and the
 * result back. */
int myyuv_gpu_dct_requantize(myyuv_hip_handle h, const uint8_t* payload, uint32_t size, uint32_t width,
                             uint32_t height, const uint8_t q_src[3], const uint8_t q_dst[3], uint8_t* out,
                             uint32_t cap, uint32_t* out_size, int64_t* bad_block);
/* Device-resident batch: stream f at d_payload + f*cap_in (its size at
 * d_payload_sizes[f], read inside min(size word, cap_in) as every decompress
 * call reads it) -> stream f at d_out + f*cap_out, its size at
 * d_out_sizes[f]; asynchronous on `stream` (NULL = the context's).  After the
 * checks above (the stream's own run on the device): d_payload and d_out
 * 4-byte aligned, cap_in and cap_out multiples of 4 when nframes > 1, and the
 * two arrays [d_payload, d_payload + nframes*cap_in) and [d_out, d_out +
 * nframes*cap_out) must not overlap: MYYUV_E_ARG, returned at once.
 * Device-side errors come through myyuv_hip_sync_status: a source stream's
 * with the batch-global block index, a frame larger than cap_out as
 * MYYUV_E_CAPACITY (no block; it takes precedence over any other error of
 * the batch, and nothing is written past cap_out).  A frame with a
 * source-stream error does not disturb the other frames of the batch: each
 * equals its single-frame result. */
int myyuv_gpu_dct_requantize_device(myyuv_hip_handle h, const void* d_payload, const uint32_t* d_payload_sizes,
                                    uint32_t cap_in, uint32_t nframes, uint32_t width, uint32_t height,
                                    const uint8_t q_src[3], const uint8_t q_dst[3], void* d_out, uint32_t cap_out,
                                    uint32_t* d_out_sizes, void* stream);

/* Downscale: the DCT stream of the 1/2, 1/4 or 1/8-size frame from a DCT
 * stream — the thumbnail or preview stream of a stored master, in one call and
 * without a frame in between.  For denom in {2, 4, 8}, bit for bit:
 *
 *   downscale(x, q_src, denom, q_dst) == compress(decompress_scaled(x, q_src, denom), q_dst)
 *
 * decompress_scaled is exactly "Scaled decode" above: the N x N inverse
 * transform of every block's low-frequency corner, N = 8 / denom, then roundf,
 * + 128, clamp to u8.  compress is exactly myyuv_gpu_dct_compress of that
 * (W/denom) x (H/denom) IYUV frame at q_dst.
 *   - The pixel clamp is part of the definition: decompress(downscale(x)) is
 *     the q_dst generation of the picture decompress_scaled(x) shows.
 *   - The result is the reference encoder's stream of a frame that never
 *     exists in HBM: an output block is the N x N pictures of a denom x denom
 *     square of source blocks, put together on chip and transformed there.
 *   - q_dst may differ from q_src per plane.
 *   - No new arithmetic: the scaled inverse is idct_scaled.h's, the forward
 *     transform and the quantisation are the compressor's (its proven fast
 *     path, else its exact path).
 * The work map (which source blocks make which output block) is
 * yuv-manipulations-2_amd/csrc/downscale.h, shared by the kernel and the host
 * check.
 * Checks and errors, in this order: those of myyuv_gpu_dct_decompress, in its
 * order, with q_src as the quality (`out` and `out_size` among the pointers);
 * then q_dst (MYYUV_E_QUALITY); then denom not in {2, 4, 8}: MYYUV_E_ARG; then
 * the scaled size as compress checks a frame of (W/denom) x (H/denom):
 * MYYUV_E_WIDTH / MYYUV_E_HEIGHT unless W and H are multiples of 16 denom.
 * A source-stream error gives exactly myyuv_gpu_dct_decompress's code and
 * *bad_block (the whole chunk of every block is decoded at every denom, as the
 * scaled decode does); the frame's output bytes are then unspecified, but stay
 * inside `cap`.  A result larger than `cap` is MYYUV_E_CAPACITY, as compress
 * reports it, with *out_size the size needed; size `cap` with
 * myyuv_dct_payload_bound(W/denom, H/denom).  `payload` and `out` must not
 * overlap.
 * Workspace: the scan's 4 B per source block, the compress calls' for the
 * scaled frame's geometry, and the two sets of tables; no frame buffer.  The
 * host-buffer form copies the source stream to the device and the result
 * back. */
int myyuv_gpu_dct_downscale(myyuv_hip_handle h, const uint8_t* payload, uint32_t size, uint32_t width,
                            uint32_t height, const uint8_t q_src[3], uint32_t denom, const uint8_t q_dst[3],
                            uint8_t* out, uint32_t cap, uint32_t* out_size, int64_t* bad_block);
/* Device-resident batch, as myyuv_gpu_dct_requantize_device: stream f at
 * d_payload + f*cap_in (its size at d_payload_sizes[f]) -> stream f at d_out +
 * f*cap_out, its size at d_out_sizes[f]; asynchronous on `stream` (NULL = the
 * context's).  The same alignment and overlap rules (MYYUV_E_ARG, returned at
 * once, after the checks above).  Device-side errors come through
 * myyuv_hip_sync_status: a source stream's with the batch-global SOURCE block
 * index, a frame larger than cap_out as MYYUV_E_CAPACITY (no block; it takes
 * precedence over any other error of the batch, and nothing is written past
 * cap_out).  A frame with a source-stream error does not disturb the other
 * frames of the batch: each equals its single-frame result. */
int myyuv_gpu_dct_downscale_device(myyuv_hip_handle h, const void* d_payload, const uint32_t* d_payload_sizes,
                                   uint32_t cap_in, uint32_t nframes, uint32_t width, uint32_t height,
                                   const uint8_t q_src[3], uint32_t denom, const uint8_t q_dst[3], void* d_out,
                                   uint32_t cap_out, uint32_t* d_out_sizes, void* stream);

/* Transform: mirror, rotate or transpose a DCT stream on its coefficients
 * (what jpegtran does for JPEG), optionally at another quality, without going
 * through pixels.  Every block of the format stands alone, so each block is
 * Huffman-decoded, moved inside the block (a transpose of the coefficients,
 * sign changes for the mirrors), rescaled as Requantise rescales it, placed at
 * its mirrored / transposed block position and encoded again.  No transform
 * runs and no frame exists in HBM.  No reference program emits these bytes, so
 * the definition is stated here, bit for bit.
 *
 * `op` is a 3-bit code: bit 0 = mirror x (mx), bit 1 = mirror y (my), bit 2 =
 * swap (transpose first, then the mirrors): */
#define MYYUV_XF_NONE 0       /* no change */
#define MYYUV_XF_FLIP_H 1     /* mirror x */
#define MYYUV_XF_FLIP_V 2     /* mirror y */
#define MYYUV_XF_ROT180 3     /* both mirrors */
#define MYYUV_XF_TRANSPOSE 4  /* swap: out[y][x] = in[x][y] */
#define MYYUV_XF_ROT90 5      /* clockwise, numpy's rot90(a, -1): out[y][x] = in[H-1-x][y] */
#define MYYUV_XF_ROT270 6     /* counter-clockwise: out[y][x] = in[x][W-1-y] */
#define MYYUV_XF_TRANSVERSE 7 /* the anti-diagonal: out[y][x] = in[H-1-x][W-1-y] */
#define MYYUV_XF_SWAPS(op) ((op) & 4)
/* The output frame is height x width when MYYUV_XF_SWAPS(op), width x height
 * otherwise; both satisfy the dimension checks whenever the source does, and
 * the block, tile and unit counts of every plane are equal in both.
 *
 * For every plane p, the source block at (bx, by) of bw x bh blocks has the
 * decoded coefficients z[u][v], natural order n = 8u + v, u the vertical
 * frequency and v the horizontal; Qs and Qd are plane p's tables for q_src[p]
 * and q_dst[p].
 *   (u', v')    = swap ? (v, u) : (u, v)                        destination position
 *   z1          = requant_coef(z[u][v], Qs[u][v], Qd[u'][v'])   Requantise's arithmetic, unchanged;
 *                                                               the identity when the two entries are equal
 *   z'[u'][v']  = clamp(s * z1, -1024, 1023)                    s = -1 iff (mx and v' odd) xor (my and u' odd)
 *   (bx1, by1, bw1, bh1) = swap ? (by, bx, bh, bw) : (bx, by, bw, bh)
 *   bx' = mx ? bw1 - 1 - bx1 : bx1,  by' = my ? bh1 - 1 - by1 : by1
 *   the destination block is by' * bw1 + bx' of the same plane.
 * The clamp after the sign matters for one value only: -(-1024) = 1024 does
 * not fit the chunk format's 11 bits and becomes 1023.
 * The output stream is the reference encoder's stream of the blocks z' in the
 * destination's block order, laid out as for Requantise.
 *
 * Consequences:
 *   - op = 0 is exactly myyuv_gpu_dct_requantize.
 *   - With q_dst == q_src the three operations that do not swap change no
 *     magnitude: they are involutions on every stream the encoder wrote
 *     (applied twice, the source bytes come back), except for an AC
 *     coefficient of -1024.
 *   - The swapping operations are exact in the same sense for chroma always
 *     (the chroma table is a symmetric matrix) and for luma if and only if its
 *     table is symmetric (quality 100: all 1; quality 1: all 255).  Elsewhere a
 *     luma coefficient is rescaled between Q[u][v] and Q[v][u], which costs
 *     about what decode - rotate - encode costs in fidelity: there the gain of
 *     a swapping operation is speed and the frame that never exists, not
 *     fidelity.
 *   - Decoded pixels of the result are NOT promised to equal the moved pixels
 *     of the source's decode: the contract is bit for bit on coefficients.
 *     (The inverse transform's basis is only almost symmetric, so on noise a
 *     few pixels in ten thousand differ by one.)
 *
 * The in-block arithmetic and the block map are
 * yuv-manipulations-2_amd/csrc/coef_xform.h, shared by the kernel and the host
 * check.
 * Checks and errors: op > 7 is MYYUV_E_ARG, together with the null-pointer
 * checks.  Everything else, its order, *bad_block (in the SOURCE's block
 * numbering), `cap` and MYYUV_E_CAPACITY are exactly myyuv_gpu_dct_requantize's,
 * with `width` and `height` the source's.  Workspace: Requantise's, plus a
 * scratch coefficient image (128 B per block) for streams with Huffman tables
 * the encoder never writes. */
int myyuv_gpu_dct_transform(myyuv_hip_handle h, const uint8_t* payload, uint32_t size, uint32_t width,
                            uint32_t height, const uint8_t q_src[3], uint32_t op, const uint8_t q_dst[3],
                            uint8_t* out, uint32_t cap, uint32_t* out_size, int64_t* bad_block);
/* Device-resident batch: as myyuv_gpu_dct_requantize_device (same layout,
 * alignment and overlap rules, same error reporting), every frame transformed
 * by `op`. */
int myyuv_gpu_dct_transform_device(myyuv_hip_handle h, const void* d_payload, const uint32_t* d_payload_sizes,
                                   uint32_t cap_in, uint32_t nframes, uint32_t width, uint32_t height,
                                   const uint8_t q_src[3], uint32_t op, const uint8_t q_dst[3], void* d_out,
                                   uint32_t cap_out, uint32_t* d_out_sizes, void* stream);

/* Crop and join: cut a rectangle out of a DCT stream, or lay a grid of equally
 * sized streams side by side as one, without leaving the compressed form
 * (jpegtran -crop, and -drop in its useful form).  Every block of the format
 * stands alone (see Requantise) and every chunk is byte-aligned with a u8 size,
 * so both are exact byte gathers: nothing is Huffman-decoded, there is no
 * arithmetic, and no quantisation table is read.  No reference program emits
 * these bytes, so the definition is stated here, bit for bit.
 *
 * For plane p, d = 8 (Y) or 16 (U, V): luma pixels per block of the plane.  A
 * source frame W x H has bw = W/d blocks per row of plane p; size_p[k] is the
 * plane's size table and chunk_p[k] its chunk k: size_p[k] bytes at the
 * exclusive prefix sum of the sizes inside the plane's content.
 *
 * Crop (rx, ry, rw, rh), in luma pixels, top-down: all multiples of 16, rw,
 * rh > 0, rx+rw <= W, ry+rh <= H (no 32-bit wrap) — region decode's rules.
 * The output is the DCTYUV stream of an rw x rh frame:
 *   - plane p has (rw/d) * (rh/d) blocks;
 *   - block (by', bx') of plane p, row-major, takes the size byte and the
 *     chunk bytes of the source plane's block (ry/d + by') * bw + rx/d + bx',
 *     verbatim;
 *   - plane_size[3], nblocks and content_size are written as DCTYUV::dump
 *     writes them (plane_size = 8 + nblocks + content_size, no slack).
 *
 * Join (cols, rows, tile_w, tile_h and cols * rows streams of tile_w x tile_h
 * frames, tile t = ty * cols + tx): tile_w, tile_h multiples of 16, cols,
 * rows >= 1.  The output is the stream of a (cols*tile_w) x (rows*tile_h)
 * frame; with bw_t = tile_w/d, bh_t = tile_h/d:
 *   - block (by', bx') of plane p is block (by' mod bh_t) * bw_t + (bx' mod
 *     bw_t) of plane p of tile (by' div bh_t) * cols + bx' div bw_t, verbatim.
 *
 * Chunks are NOT examined.  Consequences:
 *   - The crop of a whole frame returns the source stream's bytes when the
 *     source is laid out as DCTYUV::dump lays it out (plane_size[p] == 8 +
 *     nblocks + content_size, the sizes summing to content_size).  Slack the
 *     source declares beyond that is not carried over.
 *   - For a stream the reference encoder wrote, crop equals
 *     compress(pixel-crop(frame)), and join equals compress(assembled frame) at
 *     the tiles' quality, byte for byte.
 *   - A malformed chunk is carried over unreported, as region decode does not
 *     report one outside its rectangle.
 *   - Cropping tile t's rectangle out of a join returns tile t's stream.
 *   - There is no quality argument.  A join of tiles compressed at different
 *     qualities is a valid stream that no single quality decodes correctly;
 *     the C ABI cannot know and does not check.  The CLI and the C++ mirror
 *     check it, from the containers' params.
 *
 * Checks and errors, in order:
 *   1. the handle, pointer, stream-header and % 8 dimension checks of
 *      myyuv_gpu_dct_decompress, in its order (`out` and `out_size` among the
 *      pointers); there is no quality check.  Join needs cols, rows >= 1 and
 *      cols * rows <= 65,535 here already (MYYUV_E_ARG): they say how many
 *      streams there are;
 *   2. the rectangle or the grid: MYYUV_E_ARG.  Join: also when cols*tile_w or
 *      rows*tile_h wraps 32 bits, or when myyuv_gpu_dct_compress would refuse
 *      the output frame for its size;
 *   3. a source's stream-header error gives myyuv_gpu_dct_decompress's code,
 *      *bad_block the batch-global index f * blocks_per_frame of that stream's
 *      first block as the device batches report it (-1 for f = 0); for join f
 *      is the tile index.  The lowest f wins;
 *   4. a selected chunk that ends beyond its plane's declared content_size:
 *      MYYUV_E_PLANE_CONTENT, reported exactly as region decode reports it:
 *      *bad_block is the first block of the failing plane in the source's
 *      batch-global numbering (-1 when that is block 0), the lowest one when
 *      several fail.  Crop: an overrun outside the rectangle is not reported;
 *   5. a result larger than `cap`: MYYUV_E_CAPACITY, *out_size the size needed
 *      (as Requantise).  Nothing is written outside [out, out + cap);
 *   6. `payload` (every tile) and `out` must not overlap: MYYUV_E_ARG.
 * After an error of 3 or 4 the output bytes are unspecified, inside `cap`.
 * The index map is yuv-manipulations-2_amd/csrc/stream_gather.h, shared by the
 * kernels and the host check.
 * Workspace: the scans (4 B per source block and 4 B per output block, plus
 * tile words) and 1 B per output block; nothing of the 471 B per block the
 * codec calls reserve.  The host-buffer forms copy the whole source stream(s)
 * to the device and the result back. */
int myyuv_gpu_dct_crop(myyuv_hip_handle h, const uint8_t* payload, uint32_t size, uint32_t width, uint32_t height,
                       uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh, uint8_t* out, uint32_t cap,
                       uint32_t* out_size, int64_t* bad_block);
/* Device-resident batch, one rectangle for all frames: stream f at d_payload +
 * f*cap_in (its size at d_payload_sizes[f], read inside min(size word,
 * cap_in)) -> stream f at d_out + f*cap_out, its size at d_out_sizes[f];
 * asynchronous on `stream` (NULL = the context's).  myyuv_gpu_dct_requantize_device's
 * rules: d_payload and d_out 4-byte aligned, cap_in and cap_out multiples of 4
 * when nframes > 1, the two arrays must not overlap (MYYUV_E_ARG, returned at
 * once, after the dimension and rectangle checks).  Device-side errors come
 * through myyuv_hip_sync_status: a source stream's with the batch-global
 * block index, a frame larger than cap_out as MYYUV_E_CAPACITY (no block; it
 * takes precedence; nothing of that frame but d_out_sizes[f] is written).  A
 * frame with a source error does not disturb the others. */
int myyuv_gpu_dct_crop_device(myyuv_hip_handle h, const void* d_payload, const uint32_t* d_payload_sizes,
                              uint32_t cap_in, uint32_t nframes, uint32_t width, uint32_t height, uint32_t rx,
                              uint32_t ry, uint32_t rw, uint32_t rh, void* d_out, uint32_t cap_out,
                              uint32_t* d_out_sizes, void* stream);
/* payloads[t] / sizes[t]: tile t's stream, t = ty * cols + tx. */
int myyuv_gpu_dct_join(myyuv_hip_handle h, const uint8_t* const* payloads, const uint32_t* sizes, uint32_t cols,
                       uint32_t rows, uint32_t tile_w, uint32_t tile_h, uint8_t* out, uint32_t cap,
                       uint32_t* out_size, int64_t* bad_block);
/* Device-resident form, one output frame per call: tile t at d_payload +
 * t*cap_in (cap_in a multiple of 4 when cols * rows > 1), its size at
 * d_payload_sizes[t] -> the stream at d_out (capacity cap_out), its size at
 * *d_out_size.  Otherwise as myyuv_gpu_dct_crop_device. */
int myyuv_gpu_dct_join_device(myyuv_hip_handle h, const void* d_payload, const uint32_t* d_payload_sizes,
                              uint32_t cap_in, uint32_t cols, uint32_t rows, uint32_t tile_w, uint32_t tile_h,
                              void* d_out, uint32_t cap_out, uint32_t* d_out_size, void* stream);

/* Compare: how far a frame is from another — PSNR's squared error and a block
 * SSIM — between two raw IYUV frames, or between a DCT stream and a raw frame
 * without the stream's decoded frame ever existing in HBM: the fused decoder
 * loads the reference frame's rows where the full decode stores its own and
 * keeps integer sums.  No reference program emits these figures, so the
 * definition is stated here, bit for bit.  Every figure the device produces is
 * an integer; there is no floating point in the kernels.
 *
 * Per plane the block grid is the codec's own: 8x8 blocks, row-major,
 * k = (y/8) * bw + x/8.  With x the 64 reference samples and y the 64 test
 * samples (u8) of block k:
 *   sse_k  = sum (x - y)^2                                 (<= 64 * 255^2 = 4,161,600)
 *   max_k  = max |x - y|
 *   Sx = sum x, Sy = sum y, Sxx = sum x^2, Syy = sum y^2, Sxy = sum x y      (u32)
 *   C1 = 26634 (= round(4096 (0.01 * 255)^2)),  C2 = 239708 (= round(4096 (0.03 * 255)^2))
 *   A1 = 2 Sx Sy + C1              A2 = 2 (64 Sxy - Sx Sy) + C2       (A2 may be negative)
 *   B1 = Sx^2 + Sy^2 + C1          B2 = 64 (Sxx + Syy) - Sx^2 - Sy^2 + C2
 *   ssim_k = floor(A1 A2 2^24 / (B1 B2))        floor towards minus infinity; int32 in [-2^24, 2^24]
 * This is SSIM over non-overlapping 8x8 windows, the means and variances kept
 * as exact integers scaled by 64 and 4096.  B1 < 2^29 and B2 < 2^27, so
 * B1 B2 < 2^56; |A1 A2| <= B1 B2 always (2ab <= a^2 + b^2 in both factors);
 * identical blocks give exactly 2^24.  Everything is symmetric in x and y.
 * The arithmetic is yuv-manipulations-2_amd/csrc/metric.h, shared by the
 * kernels and the host check.
 *
 * A plane's record sums its blocks: sse, ssim_sum = sum ssim_k, nblocks, and
 * max_abs = max max_k.  The optional map holds every block's pair, in the
 * codec's block order (planes Y, U, V; frame f's block g at f * blocks_per_frame
 * + g).  The integers are the contract; the two functions below turn them
 * into the usual numbers on the host. */
typedef struct { uint64_t sse; int64_t ssim_sum; uint32_t nblocks; uint32_t max_abs; } myyuv_plane_metric;
typedef struct { myyuv_plane_metric plane[3]; } myyuv_frame_metric;      /* Y, U, V */
typedef struct { uint32_t sse; int32_t ssim; } myyuv_block_metric;
/* 10 log10(255^2 nsamples / sse), +inf at sse == 0. */
double myyuv_metric_psnr(uint64_t sse, uint64_t nsamples);
/* ssim_sum / (nblocks 2^24). */
double myyuv_metric_ssim(int64_t ssim_sum, uint64_t nblocks);
/* Two raw frames (W*H*3/2 bytes each), host buffers.  map_or_null: one entry
 * per block of the frame.  Checks: the handle and pointers (MYYUV_E_ARG), then
 * the % 8 dimension checks of myyuv_gpu_dct_decompress.  On any error *out is
 * left zeroed. */
int myyuv_gpu_iyuv_compare(myyuv_hip_handle h, const uint8_t* ref, const uint8_t* test, uint32_t width,
                           uint32_t height, myyuv_frame_metric* out, myyuv_block_metric* map_or_null);
/* Device-resident batch: test frame f at d_test + f*W*H*3/2 against reference
 * frame f at d_ref + f*W*H*3/2 (ref_frames == nframes) or against the one
 * frame at d_ref (ref_frames == 1) -> d_out[f], and d_map[f * blocks_per_frame
 * + g] when d_map is not null; asynchronous on `stream` (NULL = the
 * context's).  d_ref, d_test, d_out and d_map are 8-byte aligned.  Every
 * record of d_out is written whole by every call (the kernels keep per-group
 * totals in the workspace, 16 B per 64 blocks, and a small kernel adds them
 * up: there is no accumulator to clear).  Argument errors (a null pointer,
 * ref_frames not in {1, nframes}, nframes == 0, alignment: MYYUV_E_ARG; the
 * dimensions) are returned at once, before any device is touched. */
int myyuv_gpu_iyuv_compare_device(myyuv_hip_handle h, const void* d_ref, const void* d_test, uint32_t nframes,
                                  uint32_t ref_frames, uint32_t width, uint32_t height,
                                  myyuv_frame_metric* d_out, myyuv_block_metric* d_map_or_null, void* stream);
/* A DCT stream (test) against a raw frame (reference), host buffers.  Checks
 * and errors: those of myyuv_gpu_dct_decompress, in its order (ref_iyuv and
 * out among the pointers).  The whole chunk of every block is decoded, so a
 * malformed stream gives exactly myyuv_gpu_dct_decompress's code and
 * *bad_block.  On any error *out is left zeroed (the map is unspecified).
 * Workspace: the scaled decode's (132 B per block: the scan and the
 * coefficient buffer for irregular tables), plus 16 B per 64 blocks of
 * per-group totals, the records and the map.  The
 * host-buffer form copies the stream and the reference frame to the device and
 * 72 B (and the map) back. */
int myyuv_gpu_dct_compare(myyuv_hip_handle h, const uint8_t* payload, uint32_t size, uint32_t width,
                          uint32_t height, const uint8_t quality[3], const uint8_t* ref_iyuv,
                          myyuv_frame_metric* out, myyuv_block_metric* map_or_null, int64_t* bad_block);
/* Device-resident batch: stream f at d_payload + f*cap (cap a multiple of 4
 * when nframes > 1, its size at d_payload_sizes[f]) against reference frame f
 * (ref_frames == nframes) or frame 0 (ref_frames == 1) of d_ref -> d_out[f] and
 * the map as above; d_payload 4-byte, d_ref, d_out and d_map 8-byte aligned;
 * asynchronous on `stream` (NULL = the context's).  Every record of d_out is
 * written whole by every call.  Argument errors are returned at once (a null
 * handle or pointer, ref_frames not in {1, nframes}: MYYUV_E_ARG, before any
 * device is touched), device-side errors through myyuv_hip_sync_status
 * (batch-global block index f * blocks_per_frame + block); the records of a
 * batch that reported one are unspecified.  Both decoder arrangements
 * (MYYUV_DECODER) run the same fused kernel. */
int myyuv_gpu_dct_compare_device(myyuv_hip_handle h, const void* d_payload, const uint32_t* d_payload_sizes,
                                 uint32_t cap, uint32_t nframes, uint32_t width, uint32_t height,
                                 const uint8_t quality[3], const void* d_ref, uint32_t ref_frames,
                                 myyuv_frame_metric* d_out, myyuv_block_metric* d_map_or_null, void* stream);

/* Probe: what a quality triple would cost and what it would give, without a
 * stream being written.
 *   MYYUV_PROBE_SIZE    K1 (+ its exact path) -> K2 (+ overflow tiers) -> the
 *     tile scan; the stream writer does not run.  plane_bytes[p] is the
 *     stream's plane_size[p] (8 + blocks + content), payload_bytes = 12 + their
 *     sum: exactly *payload_size of myyuv_gpu_dct_compress at that quality.
 *   MYYUV_PROBE_METRIC  K1 (+ its exact path) -> coef_compare -> metric_reduce;
 *     no Huffman stage runs.  coef_compare is K6's transform over the
 *     coefficient image K1 leaves in the workspace, with the source frame's
 *     rows loaded where K6 stores its own.  `metric` (and the map) is exactly
 *     what myyuv_gpu_dct_compare reports for that payload against `iyuv`.
 * With both bits K1 runs once.  The fields of a part that was not asked for
 * are zero; every record is written whole by every call.  Checks: those of
 * myyuv_gpu_dct_compress, in its order, then `what` in {1, 2, 3}
 * (MYYUV_E_ARG).  Under MYYUV_ENCODER=fused the size part runs the fused
 * encoder and the metric part K1 and its exact path all the same (the fused
 * encoder leaves no coefficient image to rely on). */
#define MYYUV_PROBE_SIZE 1u
#define MYYUV_PROBE_METRIC 2u
typedef struct {
  uint32_t plane_bytes[3];
  uint32_t payload_bytes;
  myyuv_frame_metric metric;
} myyuv_probe; /* 88 B */
int myyuv_gpu_dct_probe(myyuv_hip_handle h, const uint8_t* iyuv, uint32_t width, uint32_t height,
                        const uint8_t quality[3], uint32_t what, myyuv_probe* out,
                        myyuv_block_metric* map_or_null);
/* Device-resident batch: frame f at d_iyuv + f*W*H*3/2 -> d_out[f], and
 * d_map[f * blocks_per_frame + g] when d_map is not null and the metric part
 * is asked for; asynchronous on `stream` (NULL = the context's).  d_iyuv,
 * d_out and d_map are 8-byte aligned.  Argument errors are returned at once. */
int myyuv_gpu_dct_probe_device(myyuv_hip_handle h, const void* d_iyuv, uint32_t nframes, uint32_t width,
                               uint32_t height, const uint8_t quality[3], uint32_t what, myyuv_probe* d_out,
                               myyuv_block_metric* d_map_or_null, void* stream);

/* Encode to a target: a byte budget, or a squared-error ceiling per plane.
 * The search (yuv-manipulations-2_amd/csrc/rate_search.h, plain C++, shared
 * with the host check) probes qualities and is defined here bit for bit; it
 * is this bisection, not "the best quality" (sizes and errors are not always
 * monotone in the quality).  mid = (lo + hi) / 2, integer division.
 *
 * Size: one quality q for the three planes, budget B payload bytes.
 *   1. probe 100; size(100) <= B: the result is 100.
 *   2. probe 1; size(1) > B: MYYUV_E_TARGET, the probe at 1 reported.
 *   3. lo = 1, hi = 100; while hi - lo > 1: size(mid) <= B ? lo = mid : hi = mid.
 *      The result is lo.
 * At most 9 probes; size(q) <= B and (q == 100 or size(q + 1) > B).
 *
 * Distortion: per plane p the ceiling max_sse[p]; plane p "meets" at a probe
 * when its sse <= max_sse[p].
 *   1. probe (100, 100, 100); a plane that does not meet fails the call:
 *      MYYUV_E_TARGET, bit p of failed_planes set, the probe at 100 reported.
 *   2. probe (1, 1, 1); a plane that meets gets 1.
 *   3. every other plane: lo = 1, hi = 100; while hi - lo > 1: the plane meets
 *      at mid ? hi = mid : lo = mid.  The result is hi.
 * The planes bisect in lockstep: a probe carries each plane's current mid, a
 * finished plane its result; at most 9 probes serve the three planes.
 *
 * After the search one ordinary compress at the chosen qualities writes the
 * payload: byte for byte myyuv_gpu_dct_compress at result->quality.
 * result->quality holds the chosen qualities, or under MYYUV_E_TARGET those
 * of the failing probe, when `payload` and `*payload_size` are left
 * untouched.  result->at is the probe of result->quality with both parts:
 * the part the search steers by as its probes reported it (every chosen
 * quality was probed), the other part from one launch after the search.
 * result->probes counts the search's probes.  Checks: those
 * of myyuv_gpu_dct_compress (result among the pointers; no quality).  The
 * frame goes to the device once.  The search reads 88 B back per step, so the
 * _device forms block until the payload is written, unlike every other device
 * call here: the chosen quality is a host-side result.  d_iyuv is 8-byte,
 * d_payload 4-byte aligned; *d_payload_size is written on the device. */
#define MYYUV_E_TARGET 18 /* "target not reachable" (no reference counterpart; myyuv_hip_error_message) */
typedef struct {
  uint8_t quality[3];
  uint8_t failed_planes;
  uint32_t probes;
  myyuv_probe at;
} myyuv_target_result;
int myyuv_gpu_dct_compress_to_size(myyuv_hip_handle h, const uint8_t* iyuv, uint32_t width, uint32_t height,
                                   uint32_t max_payload_bytes, uint8_t* payload, uint32_t cap,
                                   uint32_t* payload_size, myyuv_target_result* result);
int myyuv_gpu_dct_compress_to_sse(myyuv_hip_handle h, const uint8_t* iyuv, uint32_t width, uint32_t height,
                                  const uint64_t max_sse[3], uint8_t* payload, uint32_t cap,
                                  uint32_t* payload_size, myyuv_target_result* result);
int myyuv_gpu_dct_compress_to_size_device(myyuv_hip_handle h, const void* d_iyuv, uint32_t width, uint32_t height,
                                          uint32_t max_payload_bytes, void* d_payload, uint32_t cap,
                                          uint32_t* d_payload_size, myyuv_target_result* result, void* stream);
int myyuv_gpu_dct_compress_to_sse_device(myyuv_hip_handle h, const void* d_iyuv, uint32_t width, uint32_t height,
                                         const uint64_t max_sse[3], void* d_payload, uint32_t cap,
                                         uint32_t* d_payload_size, myyuv_target_result* result, void* stream);
/* The largest s with myyuv_metric_psnr(s, nsamples) >= db (by the formula,
 * then stepped against myyuv_metric_psnr itself): db <= 0 gives
 * 65025 * nsamples, +inf gives 0.  NaN gives 0 here; the callers that take a
 * dB figure reject it (MYYUV_E_ARG). */
uint64_t myyuv_metric_sse_for_psnr(double db, uint64_t nsamples);

/* Compress from BMP: the DCT stream of a BMP pixel array in one pass, the way
 * INTO a stream for pictures that arrive as BGR(A).  For `bmp_data`, `width`,
 * `height` and `bit_count` as myyuv_gpu_bmp_to_iyuv takes them (signed header
 * fields, BGR or BGRA as stored) the result is, byte for byte,
 *   compress(bmp_to_iyuv(bmp_data, width, height, bit_count), |width|, |height|, quality)
 * that is myyuv_gpu_dct_compress applied to myyuv_gpu_bmp_to_iyuv's output; no
 * new arithmetic is defined.  One kernel (MYYUV_K_BMP_FDCT) converts a strip
 * of pixels and transforms its blocks, so the IYUV frame exists nowhere: the
 * device holds the pixels, the encoder's workspace (myyuv_hip_reserve /
 * myyuv_hip_reserve_batch for |width| x |height|) and the stream.  The call
 * runs that kernel and the split encoder's later kernels under every
 * MYYUV_ENCODER.
 * Checks and errors, in this order: the handle and the pointers
 * (MYYUV_E_ARG); then what the chain's first failing call would return:
 *   1. myyuv_gpu_bmp_to_iyuv's: MYYUV_E_BMP_INVALID (|width| % 4, bit_count
 *      0), MYYUV_E_BMP_SIGN (a zero or doubly negative size),
 *      MYYUV_E_BMP_UNSUPPORTED (odd height, not 24 / 32 bpp), MYYUV_E_ARG (more
 *      than 4 GiB of BGRA);
 *   2. myyuv_gpu_dct_compress's for (|width|, |height|, quality, cap):
 *      MYYUV_E_QUALITY, then per plane (Y, U, V) MYYUV_E_WIDTH before
 *      MYYUV_E_HEIGHT (so both must be multiples of 16; a frame beyond the
 *      kernels' 32-bit offsets is MYYUV_E_ARG before them), and last, once the
 *      size is known, MYYUV_E_CAPACITY with *payload_size set. */
int myyuv_gpu_bmp_dct_compress(myyuv_hip_handle h, const uint8_t* bmp_data, int32_t width, int32_t height,
                               uint16_t bit_count, const uint8_t quality[3], uint8_t* payload, uint32_t cap,
                               uint32_t* payload_size);
/* Device-resident batch: pixel array f at d_bmp_data + f*|width|*|height|*
 * bit_count/8 -> payload f at d_payload + f*cap (cap a multiple of 4 when
 * nframes > 1), its size at d_payload_sizes[f]; asynchronous on `stream` (NULL
 * = the context's), no allocation once the workspace has grown.  d_bmp_data is
 * 16-byte (32 bpp) or 4-byte (24 bpp) aligned, as myyuv_gpu_iyuv_to_bmp_device
 * asks of its pixel array, and d_payload 4-byte aligned: a misaligned pointer,
 * like nframes == 0, is MYYUV_E_ARG, after step 1's errors (the alignment
 * depends on bit_count) and before step 2's.  A payload beyond `cap` is a
 * device-side error (MYYUV_E_CAPACITY through myyuv_hip_sync_status), as in
 * myyuv_gpu_dct_compress_batch_device. */
int myyuv_gpu_bmp_dct_compress_device(myyuv_hip_handle h, const void* d_bmp_data, uint32_t nframes, int32_t width,
                                      int32_t height, uint16_t bit_count, const uint8_t quality[3], void* d_payload,
                                      uint32_t cap, uint32_t* d_payload_sizes, void* stream);

/* Export to JPEG: a DCT stream written as a baseline JPEG file (JFIF) on its
 * coefficients — the way OUT of the container for every program that does not
 * read it.  The codec is baseline JPEG in all but its entropy coder and its
 * container: the orthonormal 8x8 DCT of px - 128, roundf(Y / Q) with the
 * Annex K tables scaled by the quality, JPEG's zig-zag scan, 4:2:0 planes with
 * centred chroma, full-range BT.601.  So the stream's quantised coefficients
 * are the file's: no transform runs, nothing is rounded again, and no frame
 * exists in HBM.  No reference program emits these bytes, so the definition is
 * stated here, bit for bit.
 *
 * A stream of a W x H frame (multiples of 16, each at most 65,535: a larger
 * one is MYYUV_E_JPEG_DIM) with qualities q[3] becomes, in this order:
 *   SOI
 *   APP0   "JFIF\0", version 1.01, density units 0, 1:1, no thumbnail
 *   DQT    three segments, one per plane p: Pq 0, Tq p, the 64 entries of
 *          make_qtable(q[p], p != 0) (integers 1..255) as bytes in zig-zag order
 *   SOF0   precision 8, H, W, 3 components (id 1, 0x22, Tq 0), (2, 0x11, 1),
 *          (3, 0x11, 2)
 *   DHT    four segments with the tables of ITU-T T.81 Annex K.3 - K.6: DC luma
 *          (Tc/Th 0x00), AC luma (0x10), DC chroma (0x01), AC chroma (0x11)
 *   DRI    Ri = 64
 *   three NON-INTERLEAVED scans, Y, Cb, Cr, each: SOS (Ns 1, the component,
 *          tables 0/0 for Y and 1/1 for Cb and Cr, Ss 0, Se 63, Ah/Al 0), then
 *          its restart intervals with RSTm between them (not after the last),
 *          m = 0, 1, ..., 7, 0, ... from 0 in every scan
 *   EOI
 * In a non-interleaved scan an MCU is one block and the blocks run in raster
 * order, the stream's own block order, so a restart interval is 64
 * consecutive blocks of one plane (fewer at the plane's end).  Within an
 * interval every block is coded as baseline prescribes:
 *   - the DC difference against the previous block of the interval (0 at the
 *     interval's start): category = bit length of |diff|, 0..11 (differences
 *     reach +-2047), the DC table's code of the category, then `category`
 *     bits of the difference, diff - 1 for a negative one;
 *   - for every nonzero AC coefficient in zig-zag order, after r zeros: ZRL
 *     (0xF0) for each full 16 of r, the AC table's code of (r mod 16) << 4 |
 *     category, then the value bits as above.  An AC coefficient of -1024
 *     would need category 11, which baseline lacks: it is written as -1023.
 *     This is part of the definition; K1 cannot produce such a coefficient,
 *     only crafted streams hold one;
 *   - EOB (0x00) unless coefficient 63 is nonzero.
 * Bits go most significant first; the interval's last byte is filled with
 * 1-bits; every 0xFF byte of entropy data is followed by 0x00.
 *
 * myyuv_jpeg_bound(W, H) is a size no file of a W x H frame exceeds: the
 * header bytes, and per block twice 208 B (the longest block has 1,660 bits:
 * 11 + 11 for the DC, 63 x (16 + 10); stuffing at most doubles it) plus the
 * restart markers.  Files of pictures are far smaller, about half the stream.
 *
 * The arithmetic is yuv-manipulations-2_amd/csrc/jpeg_export.h, shared by the
 * kernel and the host check.
 * Checks and errors: those of myyuv_gpu_dct_decompress, in its order, with q
 * as the quality (`out` and `out_size` among the pointers); then
 * MYYUV_E_JPEG_DIM.  A stream error gives exactly myyuv_gpu_dct_decompress's
 * code and *bad_block (the failing block counts as all-zero in the file, whose
 * bytes are then unspecified but stay inside `cap`).  A file larger than `cap`
 * is MYYUV_E_CAPACITY with *out_size the size needed, and nothing is written.
 * `payload` and `out` must not overlap.
 * Workspace: the decoder's coefficient image and scan, and 8 B per 64 blocks;
 * the host-buffer form sizes its device copy of the file by the file's size. */
#define MYYUV_E_JPEG_DIM 20 /* (19 stays unassigned) "JPEG width and height must not exceed 65535" (myyuv_hip_error_message) */
uint64_t myyuv_jpeg_bound(uint32_t width, uint32_t height);
int myyuv_gpu_dct_to_jpeg(myyuv_hip_handle h, const uint8_t* payload, uint32_t size, uint32_t width,
                          uint32_t height, const uint8_t quality[3], uint8_t* out, uint32_t cap,
                          uint32_t* out_size, int64_t* bad_block);
/* The same from a raw IYUV frame: myyuv_gpu_dct_compress at `quality`, then
 * the export of that stream, byte for byte; the stream stays on the device.
 * Checks: myyuv_gpu_dct_compress's, then MYYUV_E_JPEG_DIM; `cap` and
 * MYYUV_E_CAPACITY as above. */
int myyuv_gpu_iyuv_to_jpeg(myyuv_hip_handle h, const uint8_t* iyuv, uint32_t width, uint32_t height,
                           const uint8_t quality[3], uint8_t* out, uint32_t cap, uint32_t* out_size);
/* Device-resident batch: stream f at d_payload + f*cap_in (its size at
 * d_payload_sizes[f]) -> the whole file, SOI to EOI, at d_out + f*cap_out, its
 * size at d_out_sizes[f]; asynchronous on `stream` (NULL = the context's).
 * d_payload is 4-byte aligned and cap_in a multiple of 4 when nframes > 1
 * (d_out and cap_out are free), and the two arrays must not overlap:
 * MYYUV_E_ARG, returned at once.  Device-side errors come through
 * myyuv_hip_sync_status: a stream's with the batch-global block index, a file
 * larger than cap_out as MYYUV_E_CAPACITY (no block; it takes precedence over
 * any other error of the batch; d_out_sizes[f] holds the size needed and
 * nothing of that file is written).  No byte past a file's end is written. */
int myyuv_gpu_dct_to_jpeg_device(myyuv_hip_handle h, const void* d_payload, const uint32_t* d_payload_sizes,
                                 uint32_t cap_in, uint32_t nframes, uint32_t width, uint32_t height,
                                 const uint8_t quality[3], void* d_out, uint32_t cap_out, uint32_t* d_out_sizes,
                                 void* stream);

/* Import from JPEG: a baseline 4:2:0 JPEG file read into a DCT stream on its
 * coefficients — the way IN, the reverse of the export above.  The codec is
 * baseline JPEG in all but its entropy coder and its container, so a file's
 * quantised coefficients are a stream's: the file's Huffman code is decoded on
 * the GPU, no transform runs, and with the file's own tables kept nothing is
 * rounded again.  No reference program does this, so the definition is stated
 * here, bit for bit.
 *
 * Accepted files run SOI ... EOI (bytes after EOI are ignored) and hold
 *   - exactly one frame, SOF0, precision 8, three components with sampling
 *     factors (2,2), (1,1), (1,1) in this order (component ids are free),
 *     width and height 1..65535;
 *   - 8-bit quantisation tables (Pq 0, entries 1..255) and Huffman tables,
 *     each defined before the scan that uses it (a later definition of the
 *     same slot serves the later scans; several tables in one segment are
 *     fine);
 *   - either ONE interleaved scan (Ns 3, the components in frame order): MCU =
 *     Y00 Y01 Y10 Y11 Cb Cr, MCUs in raster order over the ceil(W/16) x
 *     ceil(H/16) grid (what cameras and libjpeg write), or THREE
 *     non-interleaved scans (Ns 1) in any component order: MCU = one block, in
 *     raster order over the component's own ceil(W/8) x ceil(H/8) (luma) or
 *     ceil(W/16) x ceil(H/16) (chroma) blocks (what the export above writes);
 *     every scan Ss 0, Se 63, Ah/Al 0;
 *   - DRI of any value, none and 0 included, and it may change between scans;
 *   - APPn and COM segments, which are skipped (JFIF, EXIF and ICC are not
 *     carried over), and fill bytes (repeated 0xFF) before any marker.
 * What baseline allows but the container cannot hold is
 * MYYUV_E_JPEG_UNSUPPORTED: SOF1-3 and SOF5-15 (and DAC), a component count
 * other than 3, any other sampling, 16-bit tables, DNL (or a frame height of
 * 0), a second frame, a scan of two components, an Adobe APP14 segment whose
 * transform is not 1.  Structural damage is MYYUV_E_JPEG_SYNTAX: no SOI, a
 * truncated segment, a table entry of 0, BITS that oversubscribe the code
 * space or name more than 256 symbols, no SOF before SOS, a scan naming an
 * undefined table or component or not Ss 0 / Se 63 / Ah/Al 0, a component
 * covered twice or not at all, a restart count other than ceil(MCUs / Ri) - 1,
 * an RSTm out of sequence (m counts 0..7 from 0 in every scan), a missing EOI.
 * The first such finding in file order is the one reported.
 *
 * The frame.  The stream's frame is Wp x Hp, Wp = 16 ceil(W/16), Hp = 16
 * ceil(H/16): the file's own MCU-padded block grid, so every block of the file
 * is the stream's block at the same position.  Pixels beyond W x H are
 * whatever the file's encoder padded with.  Blocks of the grid that no scan
 * holds (non-interleaved scans of a picture whose last MCU column or row is
 * half empty) are all-zero.  Wp and Hp beyond what a stream's frame may be
 * are reported as myyuv_gpu_dct_compress reports them.
 *
 * The coefficients.  Within a restart interval (the whole scan where Ri = 0),
 * per ITU-T T.81 F.2.2: DC = predictor + EXTEND(value), the predictor per
 * component and 0 at every interval's start; AC by run/size with ZRL and EOB;
 * zig-zag positions to natural ones by the export's table.  These are errors,
 * MYYUV_E_JPEG_DATA with *bad_block the lowest failing block's index in the
 * stream's block order (Y raster, then U, then V): a DC category above 11, a
 * DC outside [-1024, 1023], an AC size of 0 with a run other than 0 or 15, an
 * AC size above 10, a run (or a ZRL, after which a coefficient must follow)
 * that passes position 63, a bit pattern that is no code of the table, a block
 * that needs bits beyond its interval's last byte.  The failing block and the
 * rest of its interval count as all-zero; the stream's bytes are then
 * unspecified but stay inside `cap` (the export's rule for a bad block,
 * mirrored).  Bytes or bits left over at an interval's end are ignored, as
 * libjpeg does.
 *
 * The quality.  quality == NULL means KEEP: each plane's table must equal
 * make_qtable(q, p != 0) for some q in 1..100, the plane takes the smallest
 * such q (the luma map q -> table is injective; the chroma one coincides only
 * for q = 1, 2, 3, all entries 255) and the coefficients pass through
 * unchanged; a plane with no such q is MYYUV_E_JPEG_TABLES.  With `quality`
 * (each 1..100, else MYYUV_E_QUALITY) every coefficient z of plane p becomes
 * myyuv_requant::requant_coef(z, Qfile[n], make_qtable(quality[p])[n])
 * (csrc/requant.h: one more rounding, as requantise adds; a plane whose table
 * is already the destination's passes through bit-exact).  q_out[3] are the
 * qualities the stream is to be decoded with.
 *
 * The stream is what K2 and the stream writer emit for those coefficients,
 * byte for byte: for a file the export wrote from an encoder-written stream s,
 * import(export(s)) is s, with the qualities export was given (1 for a chroma
 * quality of 1..3).
 *
 * How it runs (part of the contract, MYYUV_JPEG_SEGMENTS_MIN = 64): a file
 * whose scans have at least 64 restart intervals in all, none of them without
 * a restart interval, is decoded on the GPU, one lane per interval; any other
 * file is Huffman-decoded on the host by the same code (csrc/jpeg_import.h)
 * and its coefficient image uploaded.  Both give the same stream.
 *
 * myyuv_jpeg_inspect needs no handle and no device: it walks the markers and
 * reports the sizes, the layout and, per plane, the quality KEEP would take
 * (0: none).  payload_bound is myyuv_dct_payload_bound(Wp, Hp), 0 when the
 * frame is beyond a stream's.
 * Checks of myyuv_gpu_jpeg_to_dct, in order: pointers (MYYUV_E_ARG; quality
 * and bad_block may be NULL), the file (UNSUPPORTED / SYNTAX in file order),
 * the quality (MYYUV_E_QUALITY, or MYYUV_E_JPEG_TABLES for KEEP), the frame,
 * the data, the capacity: a stream larger than `cap` is MYYUV_E_CAPACITY with
 * *out_size the size needed, and nothing is written.  *width and *height are
 * Wp and Hp (myyuv_jpeg_inspect has W and H).
 * The device form takes the same file twice: `d_file` on the device (4-byte
 * aligned, readable to size rounded up to 4) for the kernel, and `file`, the
 * same bytes on the host, which the call parses itself, so no table it did not
 * check reaches the kernel.  It is asynchronous on `stream` (NULL = the
 * context's), takes the restart-interval path only (a file below the
 * threshold is MYYUV_E_JPEG_UNSUPPORTED here) and reports data errors and a
 * stream larger than `cap` through myyuv_hip_sync_status; the stream goes to
 * d_out (4-byte aligned), its size to *d_out_size.
 * Workspace: the compress calls', the segment table (20 B per interval), the
 * Huffman tables and the file or the coefficient image (128 B per block). */
#define MYYUV_E_JPEG_UNSUPPORTED 21 /* "JPEG file is not a baseline 4:2:0 picture the container can hold" */
#define MYYUV_E_JPEG_SYNTAX 22      /* "JPEG file is damaged" */
#define MYYUV_E_JPEG_DATA 23        /* "JPEG entropy data is damaged" */
#define MYYUV_E_JPEG_TABLES 24      /* "the file's tables are not the codec's: name a quality" */
#define MYYUV_JPEG_SEGMENTS_MIN 64
typedef struct myyuv_jpeg_info {
  uint32_t width, height;               /* the file's W x H */
  uint32_t padded_width, padded_height; /* the stream's Wp x Hp */
  uint32_t scans;                       /* 1 (interleaved) or 3 */
  uint32_t restart_interval[3];         /* Ri of scan s, in MCUs (0: none) */
  uint32_t segments;                    /* restart intervals of all scans */
  uint32_t on_gpu;                      /* 1: the restart-interval path applies */
  uint32_t payload_bound;
  uint8_t keep_quality[3];              /* per plane, 0: none */
  uint8_t reserved;
} myyuv_jpeg_info;
int myyuv_jpeg_inspect(const uint8_t* file, uint32_t size, myyuv_jpeg_info* info);
int myyuv_gpu_jpeg_to_dct(myyuv_hip_handle h, const uint8_t* file, uint32_t size, const uint8_t* quality,
                          uint8_t* out, uint32_t cap, uint32_t* out_size, uint32_t* width, uint32_t* height,
                          uint8_t q_out[3], int64_t* bad_block);
int myyuv_gpu_jpeg_to_dct_device(myyuv_hip_handle h, const void* d_file, const uint8_t* file, uint32_t size,
                                 const uint8_t* quality, void* d_out, uint32_t cap, uint32_t* d_out_size,
                                 uint32_t* width, uint32_t* height, uint8_t q_out[3], void* stream);

/* Host-buffer batches (many frames per call; §7 step 9:
 * transfers overlapped with the kernels).  The batch runs in chunks of up to
 * 8 frames through two device slots: chunk k's host -> device copies, chunk
 * k-1's kernels (one launch per kernel for the chunk) and chunk k-2's
 * device -> host copies run at once, on three streams.  Every frame's bytes
 * are those of the single-frame calls; the calls return when every output
 * is in host memory.  Replaces a loop of YUV::compress / YUV::decompress
 * (myyuv_cli/main.cpp:151-207) over many frames.
 *
 * Compress: frames[f] -> payload f, written to the buffer alloc(user, f,
 * size) returns once the frame's size is known (NULL: MYYUV_E_CAPACITY and
 * the call stops); sizes[f] = its size.  alloc runs on the calling thread,
 * in frame order. */
typedef uint8_t* (*myyuv_payload_alloc_fn)(void* user, uint32_t frame, uint32_t size);
int myyuv_gpu_dct_compress_frames(myyuv_hip_handle h, const uint8_t* const* frames, uint32_t nframes,
                                  uint32_t width, uint32_t height, const uint8_t quality[3],
                                  myyuv_payload_alloc_fn alloc, void* user, uint32_t* sizes);
/* Contiguous form: frame f at iyuv + f*W*H*3/2 -> payload f at payloads +
 * f*cap.  MYYUV_E_CAPACITY when a payload exceeds `cap` (sizes[] hold the
 * sizes up to that frame). */
int myyuv_gpu_dct_compress_batch(myyuv_hip_handle h, const uint8_t* iyuv, uint32_t nframes,
                                 uint32_t width, uint32_t height, const uint8_t quality[3],
                                 uint8_t* payloads, uint32_t cap, uint32_t* sizes);
/* Decompress: stream f (payloads[f], sizes[f] bytes) -> frames[f]
 * (W*H*3/2 bytes).  Every stream's header is checked first (the
 * single-frame call's DCTYUV::load checks); a decode error stops the call
 * with *bad_block the batch-global index of the failing block (frame f's
 * block g: f * blocks-per-frame + g). */
int myyuv_gpu_dct_decompress_frames(myyuv_hip_handle h, const uint8_t* const* payloads, const uint32_t* sizes,
                                    uint32_t nframes, uint32_t width, uint32_t height, const uint8_t quality[3],
                                    uint8_t* const* frames, int64_t* bad_block);
/* Contiguous form: stream f at payloads + f*cap -> frame f at iyuv + f*W*H*3/2. */
int myyuv_gpu_dct_decompress_batch(myyuv_hip_handle h, const uint8_t* payloads, const uint32_t* sizes,
                                   uint32_t cap, uint32_t nframes, uint32_t width, uint32_t height,
                                   const uint8_t quality[3], uint8_t* iyuv, int64_t* bad_block);
/* myyuv_gpu_dct_decompress_frames with each frame converted on the device
 * (myyuv_gpu_dct_decompress_to_bmp's conversion): stream f -> bmps[f]
 * (|width|*|height|*bit_count/8 bytes).  Header checks, error order and
 * *bad_block as myyuv_gpu_dct_decompress_frames. */
int myyuv_gpu_dct_decompress_to_bmp_frames(myyuv_hip_handle h, const uint8_t* const* payloads,
                                           const uint32_t* sizes, uint32_t nframes, int32_t width,
                                           int32_t height, const uint8_t quality[3], uint16_t bit_count,
                                           uint32_t chroma, uint8_t* const* bmps, int64_t* bad_block);

/* Waits for `stream`, returns (and clears) the first device-side error since
 * the last call; *bad_block as above. */
int myyuv_hip_sync_status(myyuv_hip_handle h, void* stream, int64_t* bad_block);

/* Per-kernel timing (HIP events around each launch, on the launch stream).
 * enable=1 starts recording; myyuv_hip_kernel_stats fills, per kernel id
 * (MYYUV_K_*), the summed milliseconds and launch count since enabling.
 * Times are kernel execution times (start/stop stamped from the dispatch
 * packet, as rocprofv3's kernel trace). */
#define MYYUV_K_FDCT 0       /* K1 fdct_quant */
#define MYYUV_K_HUFF_ENC 1   /* K2 huff_encode (CAP=8 pass over every block) */
#define MYYUV_K_SCAN 2       /* single-pass chunk-size scan (both directions; decode: + header checks) */
#define MYYUV_K_COMPACT 3    /* K4 stream writer: look-back scan + tiles into the DCTYUV stream */
#define MYYUV_K_ENCODE_TILE 4 /* fused single-pass encoder K1 + K2 (MYYUV_ENCODER=fused) */
#define MYYUV_K_HUFF_DEC 5   /* K5 huff_decode */
#define MYYUV_K_IDCT 6       /* K6 dequant_idct */
#define MYYUV_K_HUFF_WIDE 7  /* K2 overflow pass, lane per block (long worklists) */
#define MYYUV_K_HUFF_R16 8   /* K2 overflow tier 1: register-resident, up to 16 symbols, lane per block */
#define MYYUV_K_HUFF_WAVE 9  /* K2 overflow pass, wave per block (short worklists) */
#define MYYUV_K_BMP 10       /* K7 bmp_to_iyuv (BMP -> IYUV conversion) */
#define MYYUV_K_FDCT_FIX 11  /* K1's exact path for the units K1 listed (fdct_fix) */
#define MYYUV_K_IYUV_BMP 12  /* K8 iyuv_to_bmp (IYUV -> BMP conversion) */
#define MYYUV_K_REGION 13    /* fused decoder of a rectangle of the frame (decode_region) */
#define MYYUV_K_SCALED 14    /* fused decoder at 1/2, 1/4 or 1/8 size (decode_scaled) */
#define MYYUV_K_REQUANT 15   /* decode + coefficient rescale of the requantiser (requant) */
#define MYYUV_K_COEF_XF 16   /* decode + in-block move + rescale of the transform (coef_xform) */
/* MYYUV_K_COUNT is the length of the arrays myyuv_hip_kernel_stats fills.  It
 * is part of that call's ABI (a caller built against this header passes
 * arrays of exactly that length), so it no longer grows: ids from
 * MYYUV_K_COUNT on are profiled like any other (their mask bits included) and
 * read with myyuv_hip_kernel_stats_n, which takes the arrays' length. */
#define MYYUV_K_COUNT 17
#define MYYUV_K_GATHER 17    /* byte gather of crop and join, wave per run (stream_gather) */
#define MYYUV_K_TOTAL 18     /* every id above is below this */
/* MYYUV_K_TOTAL is frozen as MYYUV_K_COUNT is (callers size their arrays for
 * myyuv_hip_kernel_stats_n with it).  Later ids follow it, up to MYYUV_K_END. */
#define MYYUV_K_COMPARE 18   /* fused decoder against a reference frame (decode_compare) */
#define MYYUV_K_FRAME_CMP 19 /* two raw frames against each other (frame_compare) */
#define MYYUV_K_METRIC_SUM 20 /* the compare kernels' per-group totals summed per plane (metric_reduce) */
#define MYYUV_K_END 21       /* every id above is below this */
/* MYYUV_K_END is frozen as the two bounds before it (callers size their arrays
 * with it too).  The probe's ids follow it, up to MYYUV_K_LIMIT. */
#define MYYUV_K_COEF_CMP 21  /* K6's transform of K1's coefficient image against the source frame (coef_compare) */
#define MYYUV_K_PROBE_OUT 22 /* a probe's sizes and plane records gathered into its myyuv_probe records (probe_out) */
#define MYYUV_K_LIMIT 23     /* every id above is below this */
/* MYYUV_K_LIMIT is frozen as the bounds before it (callers size their arrays
 * with it too).  The downscaler's id follows it; MYYUV_K_BOUND is the bound of
 * all ids, and the length to pass to myyuv_hip_kernel_stats_n for all of them. */
#define MYYUV_K_DOWNSCALE 23 /* decode + scaled inverse + forward transform of the downscaler (downscale) */
#define MYYUV_K_BOUND 24     /* every id above is below this */
/* MYYUV_K_BOUND is frozen as the bounds before it (callers size their arrays
 * with it too).  The id of compress-from-BMP follows it; MYYUV_K_TOP is the
 * bound of all ids, and the length to pass to myyuv_hip_kernel_stats_n for all
 * of them. */
#define MYYUV_K_BMP_FDCT 24  /* BMP -> IYUV conversion + K1's forward transform of compress-from-BMP (bmp_fdct) */
#define MYYUV_K_TOP 25       /* every id above is below this */
/* MYYUV_K_TOP is frozen as the bounds before it (callers size their arrays
 * with it too).  The ids of the JPEG export follow it; MYYUV_K_MAX is the
 * bound of all ids, and the length to pass to myyuv_hip_kernel_stats_n for all
 * of them. */
#define MYYUV_K_JPEG 25      /* decode + baseline entropy coder of the JPEG export, both launches (jpeg_export) */
#define MYYUV_K_JPEG_PLACE 26 /* the export's interval offsets, file header and markers (jpeg_place) */
#define MYYUV_K_MAX 27       /* every id above is below this */
/* MYYUV_K_MAX is frozen as the bounds before it (callers size their arrays
 * with it too).  The ids of the JPEG import follow it; MYYUV_K_CEIL is the
 * bound of all ids, and the length to pass to myyuv_hip_kernel_stats_n for all
 * of them. */
#define MYYUV_K_JPEG_IMPORT 27      /* baseline Huffman decoder of the JPEG import, a lane per restart interval (jpeg_import) */
#define MYYUV_K_JPEG_IMPORT_COEF 28 /* the import's hand-off from a host-decoded coefficient image (jpeg_import_coef) */
#define MYYUV_K_CEIL 29       /* every id is below this */
int myyuv_hip_profile(myyuv_hip_handle h, int enable);
/* As myyuv_hip_profile, but stamps only the kernels whose bit (1 << MYYUV_K_*)
 * is set in `mask` (0 disables): event stamping costs host and queue time per
 * launch, so a timed region profiles just the kernel it reports on. */
int myyuv_hip_profile_kernels(myyuv_hip_handle h, uint32_t mask);
int myyuv_hip_kernel_stats(myyuv_hip_handle h, double ms[MYYUV_K_COUNT],
                           int64_t launches[MYYUV_K_COUNT]);
/* The same for the first min(n, MYYUV_K_CEIL) ids; entries from
 * MYYUV_K_CEIL on, if any, are set to 0. */
int myyuv_hip_kernel_stats_n(myyuv_hip_handle h, uint32_t n, double* ms, int64_t* launches);

/* Block-level entry points for known-answer tests (device round trip of one
 * batch of blocks).  coef is zig-zag ordered int16[64] per block; the encoder
 * rejects (MYYUV_E_ARG) coefficients outside [-1024, 1023], the 11-bit range
 * the chunk format carries and K1 produces (DCT.cpp:276). */
int myyuv_gpu_fdct_blocks(myyuv_hip_handle h, const uint8_t* px, uint32_t nblocks,
                          const float qtable[64], int16_t* coef_zz);
int myyuv_gpu_huff_encode_blocks(myyuv_hip_handle h, const int16_t* coef_zz, uint32_t nblocks,
                                 uint8_t* chunks160, uint8_t* sizes);

#ifdef __cplusplus
}
#endif
#endif /* MYYUV_HIP_H */

"""ctypes binding of the C ABI (include/myyuv_hip.h) of the gfx950 DCT codec.

This is the Python view of the product path: every call goes to
libmyyuv_hip.so (HIP kernels).  There is no CPU fallback — if the library or
a GPU is missing, calls raise.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MYYUV_HIP_LIB selects a diagnostic build (e.g. build/stamps/libmyyuv_hip.so)
LIB_PATH = os.environ.get("MYYUV_HIP_LIB") or os.path.join(_HERE, "libmyyuv_hip.so")

OK = 0
E_ARG, E_QUALITY, E_WIDTH, E_HEIGHT, E_CAPACITY = 1, 2, 3, 4, 5
E_DCTYUV_SIZE, E_PLANE_SIZE, E_PLANE_NBLK, E_PLANE_CONTENT = 6, 7, 8, 9
E_BAD_CODE, E_UNKNOWN_SYMBOL, E_BAD_CHUNK, E_HIP, E_NO_DEVICE = 10, 11, 12, 13, 14
E_BMP_INVALID, E_BMP_SIGN, E_BMP_UNSUPPORTED = 15, 16, 17
CHROMA_NEAREST, CHROMA_LINEAR = 0, 1  # MYYUV_CHROMA_*

KERNELS = ["fdct_quant", "huff_encode", "scan_tiles", "stream_out", "encode_tile", "huff_decode",
           "dequant_idct", "huff_encode_wide", "huff_encode_r16", "huff_encode_wave", "bmp_to_iyuv",
           "fdct_fix", "iyuv_to_bmp", "decode_region", "decode_scaled", "requant", "coef_xform"]
# ids: MYYUV_K_* of include/myyuv_hip.h, in KERNELS order (tests/test_cabi.py checks both)
(K_FDCT, K_HUFF_ENC, K_SCAN, K_COMPACT, K_ENCODE_TILE, K_HUFF_DEC, K_IDCT, K_HUFF_WIDE,
 K_HUFF_R16, K_HUFF_WAVE, K_BMP, K_FDCT_FIX, K_IYUV_BMP, K_REGION, K_SCALED, K_REQUANT,
 K_COEF_XF) = range(len(KERNELS))
# KERNELS is the fixed-length list of myyuv_hip_kernel_stats (MYYUV_K_COUNT: part of that call's
# ABI, it does not grow); ids from there on are read with myyuv_hip_kernel_stats_n
KERNELS_ALL = KERNELS + ["stream_gather", "decode_compare", "frame_compare", "metric_reduce"]
K_GATHER = KERNELS_ALL.index("stream_gather")
K_TOTAL = K_GATHER + 1  # MYYUV_K_TOTAL: frozen like MYYUV_K_COUNT; the ids after it end at K_END
K_COMPARE = KERNELS_ALL.index("decode_compare")
K_FRAME_CMP = KERNELS_ALL.index("frame_compare")
K_METRIC_SUM = KERNELS_ALL.index("metric_reduce")
K_END = len(KERNELS_ALL)  # MYYUV_K_END: frozen like the two bounds before it; the ids after it end at K_LIMIT
# KERNELS_ALL's names and the probe's
KERNELS_EVERY = KERNELS_ALL + ["coef_compare", "probe_out"]
K_COEF_CMP = KERNELS_EVERY.index("coef_compare")
K_PROBE_OUT = KERNELS_EVERY.index("probe_out")
K_LIMIT = len(KERNELS_EVERY)  # MYYUV_K_LIMIT: frozen like the bounds before it; the ids after it end at K_BOUND
# the downscaler's id follows
KERNELS_FULL = KERNELS_EVERY + ["downscale"]
K_DOWNSCALE = KERNELS_FULL.index("downscale")
K_BOUND = len(KERNELS_FULL)  # MYYUV_K_BOUND: frozen like the bounds before it; the ids after it end at K_TOP
# compress-from-BMP's id follows; Codec.profile / Codec.kernel_stats take and return KERNELS_TOP's names
KERNELS_TOP = KERNELS_FULL + ["bmp_fdct"]
K_BMP_FDCT = KERNELS_TOP.index("bmp_fdct")
K_TOP = len(KERNELS_TOP)  # MYYUV_K_TOP: frozen like the bounds before it; the ids after it end at K_MAX
# the JPEG export's ids follow; Codec.profile / Codec.kernel_stats take and return KERNELS_MAX's names
KERNELS_MAX = KERNELS_TOP + ["jpeg_export", "jpeg_place"]
K_JPEG = KERNELS_MAX.index("jpeg_export")
K_JPEG_PLACE = KERNELS_MAX.index("jpeg_place")
K_MAX = len(KERNELS_MAX)  # MYYUV_K_MAX: frozen like the bounds before it; the ids after it end at K_CEIL
# the JPEG import's ids follow; Codec.profile / Codec.kernel_stats take and return KERNELS_CEIL's names
KERNELS_CEIL = KERNELS_MAX + ["jpeg_import", "jpeg_import_coef"]
K_JPEG_IMPORT = KERNELS_CEIL.index("jpeg_import")
K_JPEG_IMPORT_COEF = KERNELS_CEIL.index("jpeg_import_coef")
K_CEIL = len(KERNELS_CEIL)  # MYYUV_K_CEIL
E_TARGET = 18  # MYYUV_E_TARGET: "target not reachable" (error_message; strerror's table ends at 17)
E_JPEG_DIM = 20  # MYYUV_E_JPEG_DIM: "JPEG width and height must not exceed 65535" (error_message)
# the JPEG import's (error_message): not a file the container can hold, a damaged file, damaged
# entropy data (with the failing block), tables that are no quality's
E_JPEG_UNSUPPORTED, E_JPEG_SYNTAX, E_JPEG_DATA, E_JPEG_TABLES = 21, 22, 23, 24
JPEG_SEGMENTS_MIN = 64  # MYYUV_JPEG_SEGMENTS_MIN
PROBE_SIZE, PROBE_METRIC = 1, 2  # MYYUV_PROBE_*
# myyuv_block_metric, as the maps of the compare calls come back
BLOCK_METRIC = np.dtype([("sse", np.uint32), ("ssim", np.int32)])
SSIM_ONE = 1 << 24  # ssim of identical blocks
# MYYUV_XF_*: bit 0 mirror x, bit 1 mirror y, bit 2 swap (transpose first, then the mirrors)
(XF_NONE, XF_FLIP_H, XF_FLIP_V, XF_ROT180, XF_TRANSPOSE, XF_ROT90, XF_ROT270, XF_TRANSVERSE) = range(8)
XF_NAMES = {"none": 0, "flip_h": 1, "flip_v": 2, "rot180": 3, "transpose": 4, "rot90": 5, "rot270": 6,
            "transverse": 7}


def xf_swaps(op):
    """MYYUV_XF_SWAPS: the output frame is height x width."""
    return bool(op & 4)

# the exported symbols include/myyuv_hip.h declares (checked by the CPU tests)
EXPORTS = [
    "myyuv_hip_create", "myyuv_hip_destroy", "myyuv_hip_strerror", "myyuv_dct_payload_bound",
    "myyuv_gpu_dct_compress", "myyuv_gpu_dct_decompress", "myyuv_hip_reserve",
    "myyuv_gpu_dct_compress_device", "myyuv_gpu_dct_decompress_device", "myyuv_hip_sync_status",
    "myyuv_hip_profile", "myyuv_hip_profile_kernels", "myyuv_hip_kernel_stats", "myyuv_hip_kernel_stats_n",
    "myyuv_gpu_fdct_blocks",
    "myyuv_gpu_huff_encode_blocks", "myyuv_hip_reserve_batch", "myyuv_gpu_dct_compress_batch_device",
    "myyuv_gpu_dct_decompress_batch_device", "myyuv_gpu_bmp_to_iyuv", "myyuv_gpu_bmp_to_iyuv_device",
    "myyuv_gpu_dct_compress_batch", "myyuv_gpu_dct_compress_frames", "myyuv_gpu_dct_decompress_frames",
    "myyuv_gpu_dct_decompress_batch", "myyuv_gpu_iyuv_to_bmp", "myyuv_gpu_iyuv_to_bmp_device",
    "myyuv_gpu_dct_decompress_to_bmp", "myyuv_gpu_dct_decompress_to_bmp_frames",
    "myyuv_gpu_dct_decompress_region", "myyuv_gpu_dct_decompress_region_device",
    "myyuv_gpu_dct_decompress_region_to_bmp",
    "myyuv_gpu_dct_decompress_scaled", "myyuv_gpu_dct_decompress_scaled_device",
    "myyuv_gpu_dct_decompress_scaled_to_bmp",
    "myyuv_gpu_dct_requantize", "myyuv_gpu_dct_requantize_device",
    "myyuv_gpu_dct_transform", "myyuv_gpu_dct_transform_device",
    "myyuv_gpu_dct_downscale", "myyuv_gpu_dct_downscale_device",
    "myyuv_gpu_dct_crop", "myyuv_gpu_dct_crop_device", "myyuv_gpu_dct_join", "myyuv_gpu_dct_join_device",
    "myyuv_metric_psnr", "myyuv_metric_ssim", "myyuv_gpu_iyuv_compare", "myyuv_gpu_iyuv_compare_device",
    "myyuv_gpu_dct_compare", "myyuv_gpu_dct_compare_device",
    "myyuv_gpu_dct_probe", "myyuv_gpu_dct_probe_device", "myyuv_metric_sse_for_psnr", "myyuv_hip_error_message",
    "myyuv_gpu_dct_compress_to_size", "myyuv_gpu_dct_compress_to_sse",
    "myyuv_gpu_dct_compress_to_size_device", "myyuv_gpu_dct_compress_to_sse_device",
    "myyuv_gpu_bmp_dct_compress", "myyuv_gpu_bmp_dct_compress_device",
    "myyuv_jpeg_bound", "myyuv_gpu_dct_to_jpeg", "myyuv_gpu_dct_to_jpeg_device", "myyuv_gpu_iyuv_to_jpeg",
    "myyuv_jpeg_inspect", "myyuv_gpu_jpeg_to_dct", "myyuv_gpu_jpeg_to_dct_device",
]


class PlaneMetric(ctypes.Structure):
    """myyuv_plane_metric"""
    _fields_ = [("sse", ctypes.c_uint64), ("ssim_sum", ctypes.c_int64), ("nblocks", ctypes.c_uint32),
                ("max_abs", ctypes.c_uint32)]


class FrameMetric(ctypes.Structure):
    """myyuv_frame_metric"""
    _fields_ = [("plane", PlaneMetric * 3)]

    def as_ints(self):
        """((sse, ssim_sum, nblocks, max_abs) of Y, of U, of V), plain ints."""
        return tuple((int(p.sse), int(p.ssim_sum), int(p.nblocks), int(p.max_abs)) for p in self.plane)


class Probe(ctypes.Structure):
    """myyuv_probe (88 B)"""
    _fields_ = [("plane_bytes", ctypes.c_uint32 * 3), ("payload_bytes", ctypes.c_uint32), ("metric", FrameMetric)]

    def as_ints(self):
        """((plane bytes of Y, U, V), payload bytes, FrameMetric.as_ints()), plain ints."""
        return (tuple(int(v) for v in self.plane_bytes), int(self.payload_bytes), self.metric.as_ints())


class TargetResult(ctypes.Structure):
    """myyuv_target_result"""
    _fields_ = [("quality", ctypes.c_uint8 * 3), ("failed_planes", ctypes.c_uint8), ("probes", ctypes.c_uint32),
                ("at", Probe)]

    def as_dict(self):
        return {"quality": tuple(int(v) for v in self.quality), "failed_planes": int(self.failed_planes),
                "probes": int(self.probes), "at": self.at.as_ints()}


# myyuv_probe as an array's element (probe_device's d_out read back)
PROBE_DTYPE = np.dtype([("plane_bytes", np.uint32, 3), ("payload_bytes", np.uint32),
                        ("metric", [("sse", np.uint64), ("ssim_sum", np.int64), ("nblocks", np.uint32),
                                    ("max_abs", np.uint32)], 3)])

_lib = None
# myyuv_payload_alloc_fn
PAYLOAD_ALLOC = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32)


class JpegInfo(ctypes.Structure):
    """myyuv_jpeg_info."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("padded_width", ctypes.c_uint32),
                ("padded_height", ctypes.c_uint32), ("scans", ctypes.c_uint32),
                ("restart_interval", ctypes.c_uint32 * 3), ("segments", ctypes.c_uint32),
                ("on_gpu", ctypes.c_uint32), ("payload_bound", ctypes.c_uint32),
                ("keep_quality", ctypes.c_uint8 * 3), ("reserved", ctypes.c_uint8)]

    def as_dict(self):
        return {"width": self.width, "height": self.height, "padded_width": self.padded_width,
                "padded_height": self.padded_height, "scans": self.scans,
                "restart_interval": list(self.restart_interval)[:self.scans], "segments": self.segments,
                "on_gpu": bool(self.on_gpu), "payload_bound": self.payload_bound,
                "keep_quality": tuple(self.keep_quality)}


class CodecError(RuntimeError):
    """A MYYUV_E_* failure; .code is the number, str() the reference's message."""

    def __init__(self, code, bad_block=-1):
        self.code = code
        self.bad_block = bad_block
        self.result = None  # E_TARGET: TargetResult.as_dict() of the failing probe
        super().__init__(error_message(code) if _lib is not None else f"error {code}")


def _share_hip_runtime_with_torch():
    """torch ships its own libamdhip64 with the same soname (libamdhip64.so.7)
    as /opt/rocm's.  Two copies in one process means two HIP/HSA runtimes and
    the second one finds no GPU.  When torch is importable, load it first so
    this library binds to the runtime torch already mapped (the loader matches
    our NEEDED libamdhip64.so.7 against it); without torch the library uses
    /opt/rocm's runtime through its RUNPATH."""
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if os.environ.get("MYYUV_NO_TORCH_RUNTIME") != "1":
        _share_hip_runtime_with_torch()
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} missing: build it with `make -C yuv-manipulations-2_amd`"
                                " or __graft_entry__.build()")
    L = ctypes.CDLL(LIB_PATH)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    vp = ctypes.c_void_p
    u32 = ctypes.c_uint32
    L.myyuv_hip_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.myyuv_hip_destroy.argtypes = [vp]
    L.myyuv_hip_destroy.restype = None
    L.myyuv_hip_strerror.argtypes = [ctypes.c_int]
    L.myyuv_hip_strerror.restype = ctypes.c_char_p
    L.myyuv_hip_error_message.argtypes = [ctypes.c_int]
    L.myyuv_hip_error_message.restype = ctypes.c_char_p
    L.myyuv_dct_payload_bound.argtypes = [u32, u32]
    L.myyuv_dct_payload_bound.restype = u32
    L.myyuv_gpu_dct_compress.argtypes = [vp, u8p, u32, u32, u8p, u8p, u32, ctypes.POINTER(u32)]
    L.myyuv_gpu_dct_decompress.argtypes = [vp, u8p, u32, u32, u32, u8p, u8p,
                                           ctypes.POINTER(ctypes.c_int64)]
    L.myyuv_hip_reserve.argtypes = [vp, u32, u32]
    L.myyuv_gpu_dct_compress_device.argtypes = [vp, vp, u32, u32, u8p, vp, u32, vp, vp]
    L.myyuv_gpu_dct_decompress_device.argtypes = [vp, vp, vp, u32, u32, u32, u8p, vp, vp]
    L.myyuv_hip_reserve_batch.argtypes = [vp, u32, u32, u32]
    L.myyuv_gpu_dct_compress_batch_device.argtypes = [vp, vp, u32, u32, u32, u8p, vp, u32, vp, vp]
    L.myyuv_gpu_dct_decompress_batch_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, u8p, vp, vp]
    L.myyuv_hip_sync_status.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_int64)]
    L.myyuv_hip_profile.argtypes = [vp, ctypes.c_int]
    L.myyuv_hip_profile_kernels.argtypes = [vp, ctypes.c_uint32]
    L.myyuv_hip_kernel_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_double),
                                         ctypes.POINTER(ctypes.c_int64)]
    L.myyuv_hip_kernel_stats_n.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_int64)]
    L.myyuv_gpu_fdct_blocks.argtypes = [vp, u8p, u32, ctypes.POINTER(ctypes.c_float),
                                        ctypes.POINTER(ctypes.c_int16)]
    L.myyuv_gpu_huff_encode_blocks.argtypes = [vp, ctypes.POINTER(ctypes.c_int16), u32, u8p, u8p]
    i32 = ctypes.c_int32
    L.myyuv_gpu_bmp_to_iyuv.argtypes = [vp, u8p, i32, i32, ctypes.c_uint16, u8p]
    L.myyuv_gpu_bmp_to_iyuv_device.argtypes = [vp, vp, i32, i32, ctypes.c_uint16, vp, vp]
    L.myyuv_gpu_dct_compress_batch.argtypes = [vp, u8p, u32, u32, u32, u8p, u8p, u32, ctypes.POINTER(u32)]
    L.myyuv_gpu_dct_decompress_batch.argtypes = [vp, u8p, ctypes.POINTER(u32), u32, u32, u32, u32, u8p, u8p,
                                                 ctypes.POINTER(ctypes.c_int64)]
    L.myyuv_gpu_dct_decompress_frames.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u32), u32, u32, u32, u8p,
                                                  ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64)]
    L.myyuv_gpu_dct_compress_frames.argtypes = [vp, ctypes.POINTER(vp), u32, u32, u32, u8p, PAYLOAD_ALLOC, vp,
                                                ctypes.POINTER(u32)]
    u16 = ctypes.c_uint16
    i64p = ctypes.POINTER(ctypes.c_int64)
    L.myyuv_gpu_iyuv_to_bmp.argtypes = [vp, u8p, i32, i32, u16, u32, u8p]
    L.myyuv_gpu_iyuv_to_bmp_device.argtypes = [vp, vp, u32, i32, i32, u16, u32, vp, vp]
    L.myyuv_gpu_dct_decompress_to_bmp.argtypes = [vp, u8p, u32, i32, i32, u8p, u16, u32, u8p, i64p]
    L.myyuv_gpu_dct_decompress_to_bmp_frames.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u32), u32, i32, i32,
                                                         u8p, u16, u32, ctypes.POINTER(vp), i64p]
    L.myyuv_gpu_dct_decompress_region.argtypes = [vp, u8p, u32, u32, u32, u8p, u32, u32, u32, u32, u8p, i64p]
    L.myyuv_gpu_dct_decompress_region_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, u8p, u32, u32, u32, u32,
                                                         vp, vp]
    L.myyuv_gpu_dct_decompress_region_to_bmp.argtypes = [vp, u8p, u32, i32, i32, u8p, u32, u32, u32, u32, u16, u32,
                                                         u8p, i64p]
    L.myyuv_gpu_dct_decompress_scaled.argtypes = [vp, u8p, u32, u32, u32, u8p, u32, u8p, i64p]
    L.myyuv_gpu_dct_decompress_scaled_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, u8p, u32, vp, vp]
    L.myyuv_gpu_dct_decompress_scaled_to_bmp.argtypes = [vp, u8p, u32, i32, i32, u8p, u32, u16, u32, u8p, i64p]
    L.myyuv_gpu_dct_requantize.argtypes = [vp, u8p, u32, u32, u32, u8p, u8p, u8p, u32, ctypes.POINTER(u32), i64p]
    L.myyuv_gpu_dct_requantize_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, u8p, u8p, vp, u32, vp, vp]
    L.myyuv_gpu_dct_transform.argtypes = [vp, u8p, u32, u32, u32, u8p, u32, u8p, u8p, u32, ctypes.POINTER(u32),
                                          i64p]
    L.myyuv_gpu_dct_transform_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, u8p, u32, u8p, vp, u32, vp, vp]
    L.myyuv_gpu_dct_downscale.argtypes = [vp, u8p, u32, u32, u32, u8p, u32, u8p, u8p, u32, ctypes.POINTER(u32),
                                          i64p]
    L.myyuv_gpu_dct_downscale_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, u8p, u32, u8p, vp, u32, vp, vp]
    L.myyuv_gpu_dct_crop.argtypes = [vp, u8p, u32, u32, u32, u32, u32, u32, u32, u8p, u32, ctypes.POINTER(u32), i64p]
    L.myyuv_gpu_dct_crop_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, u32, u32, u32, u32, vp, u32, vp, vp]
    L.myyuv_gpu_dct_join.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u32), u32, u32, u32, u32, u8p, u32,
                                     ctypes.POINTER(u32), i64p]
    L.myyuv_gpu_dct_join_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, u32, vp, u32, vp, vp]
    fmp = ctypes.POINTER(FrameMetric)
    L.myyuv_metric_psnr.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    L.myyuv_metric_psnr.restype = ctypes.c_double
    L.myyuv_metric_ssim.argtypes = [ctypes.c_int64, ctypes.c_uint64]
    L.myyuv_metric_ssim.restype = ctypes.c_double
    L.myyuv_gpu_iyuv_compare.argtypes = [vp, u8p, u8p, u32, u32, fmp, vp]
    L.myyuv_gpu_iyuv_compare_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp, vp]
    L.myyuv_gpu_dct_compare.argtypes = [vp, u8p, u32, u32, u32, u8p, u8p, fmp, vp, i64p]
    L.myyuv_gpu_dct_compare_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, u8p, vp, u32, vp, vp, vp]
    prp, trp = ctypes.POINTER(Probe), ctypes.POINTER(TargetResult)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.myyuv_gpu_dct_probe.argtypes = [vp, u8p, u32, u32, u8p, u32, prp, vp]
    L.myyuv_gpu_dct_probe_device.argtypes = [vp, vp, u32, u32, u32, u8p, u32, vp, vp, vp]
    L.myyuv_metric_sse_for_psnr.argtypes = [ctypes.c_double, ctypes.c_uint64]
    L.myyuv_metric_sse_for_psnr.restype = ctypes.c_uint64
    L.myyuv_gpu_dct_compress_to_size.argtypes = [vp, u8p, u32, u32, u32, u8p, u32, ctypes.POINTER(u32), trp]
    L.myyuv_gpu_dct_compress_to_sse.argtypes = [vp, u8p, u32, u32, u64p, u8p, u32, ctypes.POINTER(u32), trp]
    L.myyuv_gpu_dct_compress_to_size_device.argtypes = [vp, vp, u32, u32, u32, vp, u32, vp, trp, vp]
    L.myyuv_gpu_dct_compress_to_sse_device.argtypes = [vp, vp, u32, u32, u64p, vp, u32, vp, trp, vp]
    L.myyuv_gpu_bmp_dct_compress.argtypes = [vp, u8p, i32, i32, u16, u8p, u8p, u32, ctypes.POINTER(u32)]
    L.myyuv_gpu_bmp_dct_compress_device.argtypes = [vp, vp, u32, i32, i32, u16, u8p, vp, u32, vp, vp]
    L.myyuv_jpeg_bound.argtypes = [u32, u32]
    L.myyuv_jpeg_bound.restype = ctypes.c_uint64
    L.myyuv_gpu_dct_to_jpeg.argtypes = [vp, u8p, u32, u32, u32, u8p, u8p, u32, ctypes.POINTER(u32), i64p]
    L.myyuv_gpu_dct_to_jpeg_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, u8p, vp, u32, vp, vp]
    L.myyuv_gpu_iyuv_to_jpeg.argtypes = [vp, u8p, u32, u32, u8p, u8p, u32, ctypes.POINTER(u32)]
    u32p = ctypes.POINTER(u32)
    L.myyuv_jpeg_inspect.argtypes = [u8p, u32, ctypes.POINTER(JpegInfo)]
    L.myyuv_gpu_jpeg_to_dct.argtypes = [vp, u8p, u32, u8p, u8p, u32, u32p, u32p, u32p, u8p, i64p]
    L.myyuv_gpu_jpeg_to_dct_device.argtypes = [vp, vp, u8p, u32, u8p, vp, u32, vp, u32p, u32p, u8p, vp]
    L.myyuv_debug_tinfo_guard.argtypes =[vp, u32, ctypes.c_int, ctypes.POINTER(u32)]  # diagnostic
    L.myyuv_debug_huff_encode_blocks.argtypes = [vp, ctypes.POINTER(ctypes.c_int16), u32, u32, u8p, u8p,
                                                 ctypes.POINTER(u32)]  # diagnostic
    L.myyuv_debug_k2_constants.argtypes = [ctypes.POINTER(u32)]  # diagnostic
    L.myyuv_debug_fdct_blocks.argtypes = [vp, u8p, u32, ctypes.POINTER(ctypes.c_float),
                                          ctypes.POINTER(ctypes.c_int16), u8p, ctypes.POINTER(u32)]  # diagnostic
    _lib = L
    return L


def strerror(code):
    return load().myyuv_hip_strerror(int(code)).decode()


def error_message(code):
    """myyuv_hip_error_message: the text of every code (strerror's for the codes up to 17)."""
    return load().myyuv_hip_error_message(int(code)).decode()


def payload_bound(w, h):
    return load().myyuv_dct_payload_bound(w, h)


def jpeg_inspect(data):
    """myyuv_jpeg_inspect (no device): a JPEG file's sizes, layout and, per
    plane, the quality an import that keeps the file's tables would take."""
    src = np.ascontiguousarray(np.frombuffer(memoryview(data).cast("B"), np.uint8))
    info = JpegInfo()
    rc = load().myyuv_jpeg_inspect(_u8(src), src.nbytes, ctypes.byref(info))
    if rc:
        raise CodecError(rc)
    return info.as_dict()


def jpeg_bound(w, h):
    """myyuv_jpeg_bound: a size no exported file of a w x h frame exceeds."""
    return int(load().myyuv_jpeg_bound(w, h))


def metric_psnr(sse, nsamples):
    """myyuv_metric_psnr: dB, inf at sse == 0."""
    return load().myyuv_metric_psnr(int(sse), int(nsamples))


def metric_ssim(ssim_sum, nblocks):
    """myyuv_metric_ssim: ssim_sum / (nblocks * 2^24)."""
    return load().myyuv_metric_ssim(int(ssim_sum), int(nblocks))


def metric_sse_for_psnr(db, nsamples):
    """myyuv_metric_sse_for_psnr: the largest sse whose PSNR over nsamples is at least db."""
    return int(load().myyuv_metric_sse_for_psnr(float(db), int(nsamples)))


def k2_constants():
    """Diagnostic (not in include/myyuv_hip.h): the constants K2's overflow
    regimes switch on, as the library was built (codec_common.hpp)."""
    v = (ctypes.c_uint32 * 7)()
    rc = load().myyuv_debug_k2_constants(v)
    if rc:
        raise CodecError(rc)
    names = ("r16_gate_single", "r16_gate", "wave_encode_limit", "batch_wave_limit", "k2_group", "window_blocks",
             "ovf_nub")
    return dict(zip(names, (int(x) for x in v)))


def batch_tiles(w, h):
    """K2's 256-block tiles per frame (FrameGeom::tcum[3]): per plane
    ceil(blocks / 256), Y then U and V."""
    y = (w // 8) * (h // 8)
    c = (w // 16) * (h // 16)
    return -(-y // 256) + 2 * -(-c // 256)


def _u8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _u8_array(a, name, writable=False):
    """The caller's buffer as-is (no copy): a C-contiguous uint8 ndarray, else
    ValueError (a strided or wider-typed array would hand the C ABI the wrong
    bytes, and a copy of `out` would drop the result)."""
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or not a.flags.c_contiguous:
        raise ValueError(f"{name}: a C-contiguous numpy uint8 array is required")
    if writable and not a.flags.writeable:
        raise ValueError(f"{name}: read-only array")
    return a


def _q(q):
    return np.ascontiguousarray(np.array(q, dtype=np.int64).astype(np.uint8))


class Codec:
    """One context (HIP stream + workspace) on one device."""

    def __init__(self, device=0):
        L = load()
        h = ctypes.c_void_p()
        rc = L.myyuv_hip_create(int(device), ctypes.byref(h))
        if rc:
            raise CodecError(rc)
        self._h = h
        self.device = device

    def close(self):
        if self._h:
            load().myyuv_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host-buffer API (what YUV::compress_map / decompress_map call) --
    def compress(self, iyuv, w, h, q):
        """IYUV bytes -> DCTYUV payload bytes."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(iyuv).cast("B"), np.uint8))
        if src.size < w * h * 3 // 2:
            raise ValueError("frame smaller than W*H*3/2")
        qa = _q(q)
        cap = payload_bound(w, h)
        out = np.empty(cap, np.uint8)
        size = ctypes.c_uint32(0)
        rc = load().myyuv_gpu_dct_compress(self._h, _u8(src), w, h, _u8(qa), _u8(out), cap,
                                           ctypes.byref(size))
        if rc:
            raise CodecError(rc)
        return out[: size.value].tobytes()

    def decompress(self, payload, w, h, q):
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        qa = _q(q)
        out = np.empty(w * h * 3 // 2, np.uint8)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_decompress(self._h, _u8(src), src.size, w, h, _u8(qa),
                                             _u8(out), ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)
        return out.tobytes()

    def compress_into(self, iyuv, w, h, q, out):
        """IYUV numpy buffer -> payload written into the caller's numpy buffer
        `out` (no per-call allocation); returns the payload size.  Both must be
        C-contiguous uint8 arrays: `iyuv` at least W*H*3/2 bytes, `out` sized
        by its byte count (a short `out` fails with E_CAPACITY)."""
        src = _u8_array(iyuv, "iyuv")
        dst = _u8_array(out, "out", writable=True)
        if src.nbytes < w * h * 3 // 2:
            raise ValueError("frame smaller than W*H*3/2")
        size = ctypes.c_uint32(0)
        rc = load().myyuv_gpu_dct_compress(self._h, _u8(src), w, h, _u8(_q(q)), _u8(dst), dst.nbytes,
                                           ctypes.byref(size))
        if rc:
            raise CodecError(rc)
        return size.value

    def decompress_into(self, payload, w, h, q, out):
        """payload numpy buffer -> IYUV frame written into the caller's numpy
        buffer `out` (at least W*H*3/2 bytes); both C-contiguous uint8."""
        src = _u8_array(payload, "payload")
        dst = _u8_array(out, "out", writable=True)
        if dst.nbytes < w * h * 3 // 2:
            raise ValueError("output smaller than W*H*3/2")
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_decompress(self._h, _u8(src), src.nbytes, w, h, _u8(_q(q)), _u8(dst),
                                             ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)

    def compress_batch(self, frames, w, h, q):
        """Host-buffer batch: a list of IYUV frames of one geometry -> their
        DCTYUV payloads (one launch per kernel for the batch)."""
        n = len(frames)
        fb = w * h * 3 // 2
        for i, f in enumerate(frames):
            if len(memoryview(f).cast("B")) != fb:
                raise ValueError(f"frame {i}: {len(memoryview(f).cast('B'))} bytes, a {w}x{h} IYUV frame has {fb}")
        src = np.ascontiguousarray(np.frombuffer(b"".join(bytes(f) for f in frames), np.uint8))
        cap = (payload_bound(w, h) + 3) & ~3
        out = np.empty(n * cap, np.uint8)
        sizes = (ctypes.c_uint32 * n)()
        rc = load().myyuv_gpu_dct_compress_batch(self._h, _u8(src), n, w, h, _u8(_q(q)), _u8(out), cap, sizes)
        if rc:
            raise CodecError(rc)
        return [out[i * cap: i * cap + sizes[i]].tobytes() for i in range(n)]

    def compress_frames(self, frames, w, h, q):
        """Host-buffer batch through the pointer-array entry point: each
        payload is written into a buffer sized once its length is known."""
        n = len(frames)
        fb = w * h * 3 // 2
        srcs = [np.frombuffer(bytes(f), np.uint8) for f in frames]
        for i, a in enumerate(srcs):
            if a.size != fb:
                raise ValueError(f"frame {i}: {a.size} bytes, a {w}x{h} IYUV frame has {fb}")
        ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in srcs])
        outs = [None] * n

        def alloc(_user, f, size):
            outs[f] = np.empty(max(size, 1), np.uint8)
            return outs[f].ctypes.data

        cb = PAYLOAD_ALLOC(alloc)
        sizes = (ctypes.c_uint32 * n)()
        rc = load().myyuv_gpu_dct_compress_frames(self._h, ptrs, n, w, h, _u8(_q(q)), cb, None, sizes)
        if rc:
            raise CodecError(rc)
        return [outs[i][: sizes[i]].tobytes() for i in range(n)]

    def decompress_batch(self, payloads, w, h, q):
        """Host-buffer batch decompress (pipelined): a list of DCTYUV
        payloads of one geometry and quality -> their IYUV frames."""
        n = len(payloads)
        fb = w * h * 3 // 2
        cap = max(len(p) for p in payloads)
        src = np.zeros(n * cap, np.uint8)
        sizes = (ctypes.c_uint32 * n)()
        for i, p in enumerate(payloads):
            src[i * cap: i * cap + len(p)] = np.frombuffer(bytes(p), np.uint8)
            sizes[i] = len(p)
        out = np.empty(n * fb, np.uint8)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_decompress_batch(self._h, _u8(src), sizes, cap, n, w, h, _u8(_q(q)), _u8(out),
                                                   ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)
        return [out[i * fb:(i + 1) * fb].tobytes() for i in range(n)]

    def decompress_frames(self, payloads, w, h, q):
        """The pointer-array form of decompress_batch."""
        n = len(payloads)
        fb = w * h * 3 // 2
        srcs = [np.frombuffer(bytes(p), np.uint8) for p in payloads]
        outs = [np.empty(fb, np.uint8) for _ in range(n)]
        ip = (ctypes.c_void_p * n)(*[a.ctypes.data for a in srcs])
        op = (ctypes.c_void_p * n)(*[a.ctypes.data for a in outs])
        sizes = (ctypes.c_uint32 * n)(*[a.size for a in srcs])
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_decompress_frames(self._h, ip, sizes, n, w, h, _u8(_q(q)), op, ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)
        return [o.tobytes() for o in outs]

    def bmp_to_iyuv(self, bmp_data, width, height, bit_count):
        """BMP::data (as stored; signed header width/height) -> IYUV bytes,
        as YUV(const BMP&, IYUV) (myyuv_yuv.cpp:88-128)."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(bmp_data).cast("B"), np.uint8))
        W, H = abs(int(width)), abs(int(height))
        if src.size < W * H * (bit_count // 8):
            raise ValueError("pixel array smaller than |w|*|h|*bit_count/8")
        out = np.empty(max(1, W * H * 3 // 2), np.uint8)
        rc = load().myyuv_gpu_bmp_to_iyuv(self._h, _u8(src), int(width), int(height), int(bit_count),
                                          _u8(out))
        if rc:
            raise CodecError(rc)
        return out[: W * H * 3 // 2].tobytes()

    def bmp_to_iyuv_device(self, d_bmp, width, height, bit_count, d_iyuv, stream=None):
        rc = load().myyuv_gpu_bmp_to_iyuv_device(self._h, d_bmp, int(width), int(height),
                                                 int(bit_count), d_iyuv, stream)
        if rc:
            raise CodecError(rc)

    # -- compress from BMP: the DCT stream of a BMP pixel array in one pass, no
    # IYUV frame in between (defined in include/myyuv_hip.h) --
    def compress_bmp(self, bmp_data, width, height, bit_count, q):
        """BMP::data (as stored; signed header width / height) -> DCTYUV
        payload bytes: compress(bmp_to_iyuv(...), |width|, |height|, q), bit for
        bit."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(bmp_data).cast("B"), np.uint8))
        cap = payload_bound(abs(int(width)), abs(int(height)))
        out = np.empty(max(1, cap), np.uint8)
        n = self.compress_bmp_into(src, width, height, bit_count, q, out)
        return out[:n].tobytes()

    def compress_bmp_into(self, bmp_data, width, height, bit_count, q, out):
        """compress_bmp from / into the caller's C-contiguous uint8 arrays;
        returns the payload size.  `out` is sized by its byte count
        (payload_bound(|width|, |height|) always fits; a short one fails with
        E_CAPACITY, CodecError.need the size needed)."""
        src = _u8_array(bmp_data, "bmp_data")
        dst = _u8_array(out, "out", writable=True)
        if src.nbytes < abs(int(width)) * abs(int(height)) * (int(bit_count) // 8):
            raise ValueError("pixel array smaller than |w|*|h|*bit_count/8")
        size = ctypes.c_uint32(0)
        rc = load().myyuv_gpu_bmp_dct_compress(self._h, _u8(src), int(width), int(height), int(bit_count),
                                               _u8(_q(q)), _u8(dst), dst.nbytes, ctypes.byref(size))
        if rc:
            err = CodecError(rc)
            err.need = size.value
            raise err
        return size.value

    def compress_bmp_device(self, d_bmp, nframes, width, height, bit_count, q, d_payload, cap, d_sizes, stream=None):
        """Device-resident batch: pixel array f at d_bmp + f*|w|*|h|*bit_count/8
        -> payload f at d_payload + f*cap, its size at d_sizes[f];
        asynchronous, device-side errors through sync_status."""
        rc = load().myyuv_gpu_bmp_dct_compress_device(self._h, d_bmp, int(nframes), int(width), int(height),
                                                      int(bit_count), _u8(_q(q)), d_payload, cap, d_sizes, stream)
        if rc:
            raise CodecError(rc)

    def iyuv_to_bmp(self, iyuv, width, height, bit_count=32, chroma=CHROMA_LINEAR):
        """IYUV frame -> the pixel array of a BMP with the signed header
        fields `width` / `height` (the inverse of bmp_to_iyuv; the conversion
        is defined in include/myyuv_hip.h)."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(iyuv).cast("B"), np.uint8))
        W, H = abs(int(width)), abs(int(height))
        if src.size < W * H * 3 // 2:
            raise ValueError("frame smaller than |w|*|h|*3/2")
        n = W * H * (int(bit_count) // 8)
        out = np.empty(max(1, n), np.uint8)
        rc = load().myyuv_gpu_iyuv_to_bmp(self._h, _u8(src), int(width), int(height), int(bit_count), int(chroma),
                                          _u8(out))
        if rc:
            raise CodecError(rc)
        return out[:n].tobytes()

    def iyuv_to_bmp_device(self, d_iyuv, nframes, width, height, bit_count, chroma, d_bmp, stream=None):
        rc = load().myyuv_gpu_iyuv_to_bmp_device(self._h, d_iyuv, int(nframes), int(width), int(height),
                                                 int(bit_count), int(chroma), d_bmp, stream)
        if rc:
            raise CodecError(rc)

    def decompress_to_bmp(self, payload, width, height, q, bit_count=32, chroma=CHROMA_LINEAR):
        """DCTYUV payload -> BMP pixel array: decompress, then iyuv_to_bmp,
        the frame staying on the device."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        n = abs(int(width)) * abs(int(height)) * (int(bit_count) // 8)
        out = np.empty(max(1, n), np.uint8)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_decompress_to_bmp(self._h, _u8(src), src.size, int(width), int(height), _u8(_q(q)),
                                                    int(bit_count), int(chroma), _u8(out), ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)
        return out[:n].tobytes()

    def decompress_to_bmp_frames(self, payloads, width, height, q, bit_count=32, chroma=CHROMA_LINEAR):
        """decompress_to_bmp for a list of payloads of one geometry and
        quality (pipelined, as decompress_frames)."""
        n = len(payloads)
        ob = abs(int(width)) * abs(int(height)) * (int(bit_count) // 8)
        srcs = [np.frombuffer(bytes(p), np.uint8) for p in payloads]
        outs = [np.empty(max(1, ob), np.uint8) for _ in range(n)]
        ip = (ctypes.c_void_p * n)(*[a.ctypes.data for a in srcs])
        op = (ctypes.c_void_p * n)(*[a.ctypes.data for a in outs])
        sizes = (ctypes.c_uint32 * n)(*[a.size for a in srcs])
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_decompress_to_bmp_frames(self._h, ip, sizes, n, int(width), int(height), _u8(_q(q)),
                                                           int(bit_count), int(chroma), op, ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)
        return [o[:ob].tobytes() for o in outs]

    # -- region decode: region = (rx, ry, rw, rh) in luma pixels, multiples of 16
    # (defined in include/myyuv_hip.h; only the region's chunks are read) --
    def decompress_region(self, payload, w, h, q, region):
        """DCTYUV payload -> the rw x rh IYUV frame cropped from the full
        decode at (rx, ry), as bytes."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        n = int(region[2]) * int(region[3]) * 3 // 2
        out = np.empty(max(1, n), np.uint8)
        self.decompress_region_into(src, w, h, q, region, out)
        return out[:n].tobytes()

    def decompress_region_into(self, payload, w, h, q, region, out):
        """decompress_region from / into the caller's C-contiguous uint8 arrays
        (`out` at least rw*rh*3/2 bytes; untouched when the call fails)."""
        src = _u8_array(payload, "payload")
        dst = _u8_array(out, "out", writable=True)
        rx, ry, rw, rh = (int(v) for v in region)
        if dst.nbytes < rw * rh * 3 // 2:
            raise ValueError("output smaller than rw*rh*3/2")
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_decompress_region(self._h, _u8(src), src.nbytes, w, h, _u8(_q(q)), rx, ry, rw, rh,
                                                    _u8(dst), ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)

    def decompress_region_device(self, d_payload, d_sizes, cap, nframes, w, h, q, region, d_iyuv, stream=None):
        """Device-resident batch: stream f at d_payload + f*cap -> region frame
        f at d_iyuv + f*rw*rh*3/2; asynchronous, errors through sync_status."""
        rx, ry, rw, rh = (int(v) for v in region)
        rc = load().myyuv_gpu_dct_decompress_region_device(self._h, d_payload, d_sizes, cap, nframes, w, h,
                                                           _u8(_q(q)), rx, ry, rw, rh, d_iyuv, stream)
        if rc:
            raise CodecError(rc)

    def decompress_region_to_bmp(self, payload, width, height, q, region, bit_count=32, chroma=CHROMA_LINEAR):
        """decompress_region, then iyuv_to_bmp of the region's frame on the
        device (width / height signed: the orientation of the BMP written)."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        rx, ry, rw, rh = (int(v) for v in region)
        n = rw * rh * (int(bit_count) // 8)
        out = np.empty(max(1, n), np.uint8)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_decompress_region_to_bmp(self._h, _u8(src), src.size, int(width), int(height),
                                                           _u8(_q(q)), rx, ry, rw, rh, int(bit_count), int(chroma),
                                                           _u8(out), ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)
        return out[:n].tobytes()

    # -- scaled decode: denom = 2, 4 or 8, a (w/denom) x (h/denom) frame from the
    # low-frequency corner of every block (defined in include/myyuv_hip.h) --
    def decompress_scaled(self, payload, w, h, q, denom):
        """DCTYUV payload -> the (w/denom) x (h/denom) IYUV frame, as bytes."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        d = int(denom)
        n = int(w) * int(h) * 3 // 2 // (d * d) if d in (2, 4, 8) else 0
        out = np.empty(max(1, n), np.uint8)
        self.decompress_scaled_into(src, w, h, q, d, out)
        return out[:n].tobytes()

    def decompress_scaled_into(self, payload, w, h, q, denom, out):
        """decompress_scaled from / into the caller's C-contiguous uint8 arrays
        (`out` at least w*h*3/2/denom^2 bytes; untouched when the call fails)."""
        src = _u8_array(payload, "payload")
        dst = _u8_array(out, "out", writable=True)
        d = int(denom)
        if d in (2, 4, 8) and dst.nbytes < int(w) * int(h) * 3 // 2 // (d * d):
            raise ValueError("output smaller than w*h*3/2/denom^2")
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_decompress_scaled(self._h, _u8(src), src.nbytes, w, h, _u8(_q(q)), d, _u8(dst),
                                                    ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)

    def decompress_scaled_device(self, d_payload, d_sizes, cap, nframes, w, h, q, denom, d_iyuv, stream=None):
        """Device-resident batch: stream f at d_payload + f*cap -> scaled frame
        f at d_iyuv + f*(w*h*3/2/denom^2); asynchronous, errors through
        sync_status."""
        rc = load().myyuv_gpu_dct_decompress_scaled_device(self._h, d_payload, d_sizes, cap, nframes, w, h,
                                                           _u8(_q(q)), int(denom), d_iyuv, stream)
        if rc:
            raise CodecError(rc)

    def decompress_scaled_to_bmp(self, payload, width, height, q, denom, bit_count=32, chroma=CHROMA_LINEAR):
        """decompress_scaled, then iyuv_to_bmp of the scaled frame on the
        device (width / height signed: the orientation of the BMP written)."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        d = int(denom)
        n = (abs(int(width)) // d) * (abs(int(height)) // d) * (int(bit_count) // 8) if d in (2, 4, 8) else 0
        out = np.empty(max(1, n), np.uint8)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_decompress_scaled_to_bmp(self._h, _u8(src), src.size, int(width), int(height),
                                                           _u8(_q(q)), d, int(bit_count), int(chroma), _u8(out),
                                                           ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)
        return out[:n].tobytes()

    # -- compare: PSNR's and block SSIM's integers between two frames, or between a
    # DCT stream and a frame without decoding it to memory (defined in include/myyuv_hip.h) --
    def compare_frames(self, ref, test, w, h, want_map=False):
        """Two raw IYUV frames -> ((sse, ssim_sum, nblocks, max_abs) of Y, U, V)
        as plain ints; with want_map also the per-block map (a BLOCK_METRIC
        array in the codec's block order, planes Y U V)."""
        a = np.ascontiguousarray(np.frombuffer(memoryview(ref).cast("B"), np.uint8))
        b = np.ascontiguousarray(np.frombuffer(memoryview(test).cast("B"), np.uint8))
        fb = int(w) * int(h) * 3 // 2
        if a.size < fb or b.size < fb:
            raise ValueError("frame smaller than W*H*3/2")
        out = FrameMetric()
        bmap = np.zeros(max(1, (w // 8) * (h // 8) + 2 * (w // 16) * (h // 16)), BLOCK_METRIC) if want_map else None
        rc = load().myyuv_gpu_iyuv_compare(self._h, _u8(a), _u8(b), w, h, ctypes.byref(out),
                                           bmap.ctypes.data if want_map else None)
        if rc:
            raise CodecError(rc)
        return (out.as_ints(), bmap) if want_map else out.as_ints()

    def compare_stream(self, payload, w, h, q, ref, want_map=False):
        """A DCTYUV payload against a raw IYUV frame, as compare_frames; the
        payload's decoded frame is never written."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        a = np.ascontiguousarray(np.frombuffer(memoryview(ref).cast("B"), np.uint8))
        if a.size < int(w) * int(h) * 3 // 2:
            raise ValueError("frame smaller than W*H*3/2")
        out = FrameMetric()
        bmap = np.zeros(max(1, (w // 8) * (h // 8) + 2 * (w // 16) * (h // 16)), BLOCK_METRIC) if want_map else None
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_compare(self._h, _u8(src), src.size, w, h, _u8(_q(q)), _u8(a), ctypes.byref(out),
                                          bmap.ctypes.data if want_map else None, ctypes.byref(bad))
        if rc:
            e = CodecError(rc, bad.value)
            e.metric = out.as_ints()  # (left zeroed by the call)
            raise e
        return (out.as_ints(), bmap) if want_map else out.as_ints()

    def compare_frames_device(self, d_ref, d_test, nframes, ref_frames, w, h, d_out, d_map=None, stream=None):
        """Device-resident batch of compare_frames: test frame f against
        reference frame f (ref_frames == nframes) or the one frame at d_ref
        (ref_frames == 1) -> d_out[f] (myyuv_frame_metric, 72 B) and the map at
        d_map when given; asynchronous."""
        rc = load().myyuv_gpu_iyuv_compare_device(self._h, d_ref, d_test, nframes, ref_frames, w, h, d_out, d_map,
                                                  stream)
        if rc:
            raise CodecError(rc)

    def compare_stream_device(self, d_payload, d_sizes, cap, nframes, w, h, q, d_ref, ref_frames, d_out, d_map=None,
                              stream=None):
        """Device-resident batch of compare_stream: stream f at d_payload +
        f*cap; asynchronous, errors through sync_status."""
        rc = load().myyuv_gpu_dct_compare_device(self._h, d_payload, d_sizes, cap, nframes, w, h, _u8(_q(q)), d_ref,
                                                 ref_frames, d_out, d_map, stream)
        if rc:
            raise CodecError(rc)

    # -- probe and encode to a target (defined in include/myyuv_hip.h) --
    def probe(self, iyuv, w, h, q, what=PROBE_SIZE | PROBE_METRIC, want_map=False):
        """What quality q would cost and give, no stream written:
        Probe.as_ints() = ((plane bytes), payload bytes, the frame metric);
        the part `what` leaves out is zero.  With want_map also the per-block
        map of the metric part (a BLOCK_METRIC array)."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(iyuv).cast("B"), np.uint8))
        if src.size < int(w) * int(h) * 3 // 2:
            raise ValueError("frame smaller than W*H*3/2")
        out = Probe()
        bmap = np.zeros(max(1, (w // 8) * (h // 8) + 2 * (w // 16) * (h // 16)), BLOCK_METRIC) if want_map else None
        rc = load().myyuv_gpu_dct_probe(self._h, _u8(src), w, h, _u8(_q(q)), int(what), ctypes.byref(out),
                                        bmap.ctypes.data if want_map else None)
        if rc:
            raise CodecError(rc)
        return (out.as_ints(), bmap) if want_map else out.as_ints()

    def probe_device(self, d_iyuv, nframes, w, h, q, what, d_out, d_map=None, stream=None):
        """Device-resident batch of probe: frame f -> d_out[f] (myyuv_probe,
        88 B, PROBE_DTYPE) and the map at d_map when given; asynchronous."""
        rc = load().myyuv_gpu_dct_probe_device(self._h, d_iyuv, nframes, w, h, _u8(_q(q)), int(what), d_out, d_map,
                                               stream)
        if rc:
            raise CodecError(rc)

    def _target(self, call, iyuv, w, h, target):
        src = np.ascontiguousarray(np.frombuffer(memoryview(iyuv).cast("B"), np.uint8))
        if src.size < int(w) * int(h) * 3 // 2:
            raise ValueError("frame smaller than W*H*3/2")
        cap = payload_bound(w, h)
        out = np.empty(cap, np.uint8)
        size = ctypes.c_uint32(0)
        res = TargetResult()
        rc = call(self._h, _u8(src), w, h, target, _u8(out), cap, ctypes.byref(size), ctypes.byref(res))
        if rc:
            e = CodecError(rc)
            e.result = res.as_dict()
            raise e
        return out[: size.value].tobytes(), res.as_dict()

    def compress_to_size(self, iyuv, w, h, max_payload_bytes):
        """The payload of the quality the size bisection (include/myyuv_hip.h)
        finds for a budget of max_payload_bytes, and the result as a dict
        (quality, failed_planes, probes, at).  E_TARGET: CodecError with
        .result the failing probe."""
        return self._target(load().myyuv_gpu_dct_compress_to_size, iyuv, w, h, int(max_payload_bytes))

    def compress_to_sse(self, iyuv, w, h, max_sse):
        """As compress_to_size, for a squared-error ceiling per plane."""
        t = (ctypes.c_uint64 * 3)(*(int(v) for v in max_sse))
        return self._target(load().myyuv_gpu_dct_compress_to_sse, iyuv, w, h, t)

    def compress_to_psnr(self, iyuv, w, h, db):
        """As compress_to_sse, every plane's PSNR at least db (a number, or one per plane)."""
        dbs = [float(v) for v in (db if isinstance(db, (tuple, list)) else (db, db, db))]
        if any(v != v for v in dbs):
            raise CodecError(E_ARG)
        n = (int(w) * int(h), int(w) * int(h) // 4, int(w) * int(h) // 4)
        return self.compress_to_sse(iyuv, w, h, [metric_sse_for_psnr(dbs[p], n[p]) for p in range(3)])

    def compress_to_size_device(self, d_iyuv, w, h, max_payload_bytes, d_payload, cap, d_size, stream=None):
        """Device-resident compress_to_size; blocks until the payload is
        written (the search reads each probe back).  Returns the result dict."""
        res = TargetResult()
        rc = load().myyuv_gpu_dct_compress_to_size_device(self._h, d_iyuv, w, h, int(max_payload_bytes), d_payload,
                                                          cap, d_size, ctypes.byref(res), stream)
        if rc:
            e = CodecError(rc)
            e.result = res.as_dict()
            raise e
        return res.as_dict()

    def compress_to_sse_device(self, d_iyuv, w, h, max_sse, d_payload, cap, d_size, stream=None):
        res = TargetResult()
        t = (ctypes.c_uint64 * 3)(*(int(v) for v in max_sse))
        rc = load().myyuv_gpu_dct_compress_to_sse_device(self._h, d_iyuv, w, h, t, d_payload, cap, d_size,
                                                         ctypes.byref(res), stream)
        if rc:
            e = CodecError(rc)
            e.result = res.as_dict()
            raise e
        return res.as_dict()

    # -- requantise: a DCT stream re-encoded at another quality on its coefficients,
    # no pixels in between (defined in include/myyuv_hip.h) --
    def requantize(self, payload, w, h, q_src, q_dst):
        """DCTYUV payload written at q_src -> the DCTYUV payload at q_dst, as bytes."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        out = np.empty(max(1, payload_bound(w, h)), np.uint8)
        n = self.requantize_into(src, w, h, q_src, q_dst, out)
        return out[:n].tobytes()

    def requantize_into(self, payload, w, h, q_src, q_dst, out):
        """requantize from / into the caller's C-contiguous uint8 arrays, which
        must not overlap; returns the result's size.  `out` is sized by its
        byte count (payload_bound(w, h) always fits; a short one fails with
        E_CAPACITY)."""
        src = _u8_array(payload, "payload")
        dst = _u8_array(out, "out", writable=True)
        size = ctypes.c_uint32(0)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_requantize(self._h, _u8(src), src.nbytes, w, h, _u8(_q(q_src)), _u8(_q(q_dst)),
                                             _u8(dst), dst.nbytes, ctypes.byref(size), ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)
        return size.value

    def requantize_device(self, d_payload, d_sizes, cap_in, nframes, w, h, q_src, q_dst, d_out, cap_out,
                          d_out_sizes, stream=None):
        """Device-resident batch: stream f at d_payload + f*cap_in (size
        d_sizes[f]) -> stream f at d_out + f*cap_out, its size at
        d_out_sizes[f] (device u32); asynchronous, errors through sync_status."""
        rc = load().myyuv_gpu_dct_requantize_device(self._h, d_payload, d_sizes, cap_in, nframes, w, h,
                                                    _u8(_q(q_src)), _u8(_q(q_dst)), d_out, cap_out, d_out_sizes,
                                                    stream)
        if rc:
            raise CodecError(rc)

    # -- export to JPEG: a DCT stream written as a baseline JPEG file on its
    # coefficients (defined in include/myyuv_hip.h) --
    def to_jpeg(self, payload, w, h, q):
        """DCTYUV payload written at q -> the JPEG file's bytes.  The first try
        has room for a file of the stream's size (a picture's file is about
        half of it); a larger file is asked for again at the size the call
        reports, never at jpeg_bound."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        out = np.empty(src.nbytes + 1024, np.uint8)
        try:
            n = self.to_jpeg_into(src, w, h, q, out)
        except CodecError as e:
            if e.code != E_CAPACITY:
                raise
            out = np.empty(e.size, np.uint8)
            n = self.to_jpeg_into(src, w, h, q, out)
        return out[:n].tobytes()

    def to_jpeg_into(self, payload, w, h, q, out):
        """to_jpeg from / into the caller's C-contiguous uint8 arrays, which
        must not overlap; returns the file's size.  `out` is sized by its byte
        count; a short one fails with E_CAPACITY, the error's .size the size
        needed."""
        src = _u8_array(payload, "payload")
        dst = _u8_array(out, "out", writable=True)
        size = ctypes.c_uint32(0)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_to_jpeg(self._h, _u8(src), src.nbytes, w, h, _u8(_q(q)), _u8(dst), dst.nbytes,
                                          ctypes.byref(size), ctypes.byref(bad))
        if rc:
            e = CodecError(rc, bad.value)
            e.size = size.value
            raise e
        return size.value

    def iyuv_to_jpeg(self, iyuv, w, h, q):
        """Raw IYUV frame -> the JPEG file of its stream at q (compress, then
        to_jpeg; the stream stays on the device)."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(iyuv).cast("B"), np.uint8))
        if src.size < w * h * 3 // 2:
            raise ValueError("frame smaller than W*H*3/2")
        size = ctypes.c_uint32(0)
        out = np.empty(max(4096, w * h // 4), np.uint8)
        for _ in range(2):
            rc = load().myyuv_gpu_iyuv_to_jpeg(self._h, _u8(src), w, h, _u8(_q(q)), _u8(out), out.nbytes,
                                               ctypes.byref(size))
            if rc != E_CAPACITY:
                break
            out = np.empty(size.value, np.uint8)
        if rc:
            raise CodecError(rc)
        return out[:size.value].tobytes()

    def to_jpeg_device(self, d_payload, d_sizes, cap_in, nframes, w, h, q, d_out, cap_out, d_out_sizes,
                       stream=None):
        """Device-resident batch: stream f at d_payload + f*cap_in (size
        d_sizes[f]) -> the file at d_out + f*cap_out, its size at
        d_out_sizes[f] (device u32); asynchronous, errors through sync_status."""
        rc = load().myyuv_gpu_dct_to_jpeg_device(self._h, d_payload, d_sizes, cap_in, nframes, w, h, _u8(_q(q)),
                                                 d_out, cap_out, d_out_sizes, stream)
        if rc:
            raise CodecError(rc)

    # -- import from JPEG: a baseline 4:2:0 JPEG file read into a DCT stream on its
    # coefficients (defined in include/myyuv_hip.h) --
    def from_jpeg(self, data, q=None):
        """JPEG file -> (payload, Wp, Hp, qualities).  q None keeps the file's
        tables (E_JPEG_TABLES when they are no quality's), else the stream is
        rescaled to q."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(data).cast("B"), np.uint8))
        bound = jpeg_inspect(src)["payload_bound"]
        out = np.empty(max(bound, 64), np.uint8)
        n, w, h, qs = self.from_jpeg_into(src, out, q)
        return out[:n].tobytes(), w, h, qs

    def from_jpeg_into(self, data, out, q=None):
        """from_jpeg from / into the caller's C-contiguous uint8 arrays; returns
        (size, Wp, Hp, qualities).  A short `out` fails with E_CAPACITY, the
        error's .size the size needed."""
        src = _u8_array(data, "data")
        dst = _u8_array(out, "out", writable=True)
        size, w, h = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        qs = np.zeros(3, np.uint8)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_jpeg_to_dct(self._h, _u8(src), src.nbytes, None if q is None else _u8(_q(q)),
                                          _u8(dst), dst.nbytes, ctypes.byref(size), ctypes.byref(w),
                                          ctypes.byref(h), _u8(qs), ctypes.byref(bad))
        if rc:
            e = CodecError(rc, bad.value)
            e.size = size.value
            raise e
        return size.value, w.value, h.value, tuple(int(v) for v in qs)

    def from_jpeg_device(self, d_file, data, d_out, cap, d_out_size, q=None, stream=None):
        """Device-resident: the file at d_file (and the same bytes, `data`, on
        the host) -> the stream at d_out, its size at d_out_size (device u32);
        asynchronous, data errors through sync_status.  Returns (Wp, Hp,
        qualities).  Files below JPEG_SEGMENTS_MIN restart intervals:
        E_JPEG_UNSUPPORTED."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(data).cast("B"), np.uint8))
        w, h = ctypes.c_uint32(0), ctypes.c_uint32(0)
        qs = np.zeros(3, np.uint8)
        rc = load().myyuv_gpu_jpeg_to_dct_device(self._h, d_file, _u8(src), src.nbytes,
                                                 None if q is None else _u8(_q(q)), d_out, cap, d_out_size,
                                                 ctypes.byref(w), ctypes.byref(h), _u8(qs), stream)
        if rc:
            raise CodecError(rc)
        return w.value, h.value, tuple(int(v) for v in qs)

    # -- transform: a DCT stream mirrored, rotated or transposed on its coefficients,
    # optionally at another quality (defined in include/myyuv_hip.h) --
    def transform(self, payload, w, h, q_src, op, q_dst=None):
        """DCTYUV payload of a w x h frame written at q_src -> the payload of
        the frame moved by `op` (XF_*; h x w when xf_swaps(op)) at q_dst
        (default: q_src), as bytes."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        out = np.empty(max(1, payload_bound(w, h)), np.uint8)
        n = self.transform_into(src, w, h, q_src, op, q_src if q_dst is None else q_dst, out)
        return out[:n].tobytes()

    def transform_into(self, payload, w, h, q_src, op, q_dst, out):
        """transform from / into the caller's C-contiguous uint8 arrays, which
        must not overlap; returns the result's size (requantize_into's rules)."""
        src = _u8_array(payload, "payload")
        dst = _u8_array(out, "out", writable=True)
        size = ctypes.c_uint32(0)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_transform(self._h, _u8(src), src.nbytes, w, h, _u8(_q(q_src)), op, _u8(_q(q_dst)),
                                            _u8(dst), dst.nbytes, ctypes.byref(size), ctypes.byref(bad))
        if rc:
            raise CodecError(rc, bad.value)
        return size.value

    def transform_device(self, d_payload, d_sizes, cap_in, nframes, w, h, q_src, op, q_dst, d_out, cap_out,
                         d_out_sizes, stream=None):
        """Device-resident batch, as requantize_device, every frame moved by `op`."""
        rc = load().myyuv_gpu_dct_transform_device(self._h, d_payload, d_sizes, cap_in, nframes, w, h,
                                                   _u8(_q(q_src)), op, _u8(_q(q_dst)), d_out, cap_out, d_out_sizes,
                                                   stream)
        if rc:
            raise CodecError(rc)

    # -- downscale: the DCT stream of the 1/2, 1/4 or 1/8-size frame from a DCT stream,
    # the small frame never in memory (defined in include/myyuv_hip.h) --
    def downscale(self, payload, w, h, q_src, denom, q_dst=None):
        """DCTYUV payload of a w x h frame written at q_src -> the payload of
        the (w/denom) x (h/denom) frame at q_dst (default: q_src), as bytes:
        compress(decompress_scaled(payload, denom), q_dst), bit for bit."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        d = int(denom)
        cap = payload_bound(int(w) // d, int(h) // d) if d in (2, 4, 8) else 0
        out = np.empty(max(1, cap), np.uint8)
        n = self.downscale_into(src, w, h, q_src, d, q_src if q_dst is None else q_dst, out)
        return out[:n].tobytes()

    def downscale_into(self, payload, w, h, q_src, denom, q_dst, out):
        """downscale from / into the caller's C-contiguous uint8 arrays, which
        must not overlap; returns the result's size.  `out` is sized by its
        byte count (payload_bound(w/denom, h/denom) always fits; a short one
        fails with E_CAPACITY, CodecError.need the size needed)."""
        src = _u8_array(payload, "payload")
        dst = _u8_array(out, "out", writable=True)
        size = ctypes.c_uint32(0)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_downscale(self._h, _u8(src), src.nbytes, w, h, _u8(_q(q_src)), int(denom),
                                            _u8(_q(q_dst)), _u8(dst), dst.nbytes, ctypes.byref(size),
                                            ctypes.byref(bad))
        if rc:
            err = CodecError(rc, bad.value)
            err.need = size.value
            raise err
        return size.value

    def downscale_device(self, d_payload, d_sizes, cap_in, nframes, w, h, q_src, denom, q_dst, d_out, cap_out,
                         d_out_sizes, stream=None):
        """Device-resident batch, as requantize_device: stream f at d_payload +
        f*cap_in -> the 1/denom-size stream f at d_out + f*cap_out, its size at
        d_out_sizes[f]; asynchronous, errors through sync_status."""
        rc = load().myyuv_gpu_dct_downscale_device(self._h, d_payload, d_sizes, cap_in, nframes, w, h,
                                                   _u8(_q(q_src)), int(denom), _u8(_q(q_dst)), d_out, cap_out,
                                                   d_out_sizes, stream)
        if rc:
            raise CodecError(rc)

    # -- crop and join: a rectangle cut out of a DCT stream, a grid of streams laid
    # side by side as one, on the chunk bytes (defined in include/myyuv_hip.h) --
    def crop(self, payload, w, h, region):
        """DCTYUV payload of a w x h frame -> the payload of its rectangle
        region = (rx, ry, rw, rh) (multiples of 16), as bytes."""
        src = np.ascontiguousarray(np.frombuffer(memoryview(payload).cast("B"), np.uint8))
        out = np.empty(36 + src.nbytes, np.uint8)  # (a part of the source never exceeds it)
        n = self.crop_into(src, w, h, region, out)
        return out[:n].tobytes()

    def crop_into(self, payload, w, h, region, out):
        """crop from / into the caller's C-contiguous uint8 arrays, which must
        not overlap; returns the result's size.  A short `out` fails with
        E_CAPACITY (CodecError.need holds the size needed)."""
        src = _u8_array(payload, "payload")
        dst = _u8_array(out, "out", writable=True)
        rx, ry, rw, rh = region
        size = ctypes.c_uint32(0)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_crop(self._h, _u8(src), src.nbytes, w, h, rx, ry, rw, rh, _u8(dst), dst.nbytes,
                                       ctypes.byref(size), ctypes.byref(bad))
        if rc:
            err = CodecError(rc, bad.value)
            err.need = size.value
            raise err
        return size.value

    def crop_device(self, d_payload, d_sizes, cap_in, nframes, w, h, region, d_out, cap_out, d_out_sizes,
                    stream=None):
        """Device-resident batch, one rectangle for all frames (requantize_device's
        layout and rules); asynchronous, errors through sync_status."""
        rx, ry, rw, rh = region
        rc = load().myyuv_gpu_dct_crop_device(self._h, d_payload, d_sizes, cap_in, nframes, w, h, rx, ry, rw, rh,
                                              d_out, cap_out, d_out_sizes, stream)
        if rc:
            raise CodecError(rc)

    def join(self, payloads, cols, rows, tw, th):
        """cols * rows DCTYUV payloads of tw x th frames, row-major -> the payload
        of the (cols*tw) x (rows*th) frame, as bytes."""
        out = np.empty(max(1, 36 + sum(len(p) for p in payloads)), np.uint8)
        n = self.join_into(payloads, cols, rows, tw, th, out)
        return out[:n].tobytes()

    def join_into(self, payloads, cols, rows, tw, th, out):
        """join into the caller's C-contiguous uint8 array; returns the result's
        size (crop_into's rules).  len(payloads) must be cols * rows."""
        if len(payloads) != cols * rows:
            raise ValueError("join: cols * rows payloads are required")
        srcs = [np.ascontiguousarray(np.frombuffer(memoryview(p).cast("B"), np.uint8)) for p in payloads]
        dst = _u8_array(out, "out", writable=True)
        ptrs = (ctypes.c_void_p * max(1, len(srcs)))(*[s.ctypes.data for s in srcs])
        sizes = (ctypes.c_uint32 * max(1, len(srcs)))(*[s.nbytes for s in srcs])
        size = ctypes.c_uint32(0)
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_gpu_dct_join(self._h, ptrs, sizes, cols, rows, tw, th, _u8(dst), dst.nbytes,
                                       ctypes.byref(size), ctypes.byref(bad))
        if rc:
            err = CodecError(rc, bad.value)
            err.need = size.value
            raise err
        return size.value

    def join_device(self, d_payload, d_sizes, cap_in, cols, rows, tw, th, d_out, cap_out, d_out_size, stream=None):
        """Device-resident join: tile t at d_payload + t*cap_in (size d_sizes[t])
        -> the stream at d_out, its size at *d_out_size (device u32)."""
        rc = load().myyuv_gpu_dct_join_device(self._h, d_payload, d_sizes, cap_in, cols, rows, tw, th, d_out, cap_out,
                                              d_out_size, stream)
        if rc:
            raise CodecError(rc)

    # -- device-resident API (pointers are device addresses, e.g. torch data_ptr) --
    def reserve(self, w, h):
        rc = load().myyuv_hip_reserve(self._h, w, h)
        if rc:
            raise CodecError(rc)

    def compress_device(self, d_iyuv, w, h, q, d_payload, cap, d_size, stream=None):
        rc = load().myyuv_gpu_dct_compress_device(self._h, d_iyuv, w, h, _u8(_q(q)), d_payload,
                                                  cap, d_size, stream)
        if rc:
            raise CodecError(rc)

    def decompress_device(self, d_payload, d_size, cap, w, h, q, d_iyuv, stream=None):
        rc = load().myyuv_gpu_dct_decompress_device(self._h, d_payload, d_size, cap, w, h,
                                                    _u8(_q(q)), d_iyuv, stream)
        if rc:
            raise CodecError(rc)

    # batches: frame f at d_iyuv + f*W*H*3/2, payload f at d_payload + f*cap,
    # its size at d_sizes[f] (u32)
    def reserve_batch(self, w, h, nframes):
        rc = load().myyuv_hip_reserve_batch(self._h, w, h, nframes)
        if rc:
            raise CodecError(rc)

    def compress_batch_device(self, d_iyuv, nframes, w, h, q, d_payload, cap, d_sizes, stream=None):
        rc = load().myyuv_gpu_dct_compress_batch_device(self._h, d_iyuv, nframes, w, h, _u8(_q(q)),
                                                        d_payload, cap, d_sizes, stream)
        if rc:
            raise CodecError(rc)

    def decompress_batch_device(self, d_payload, d_sizes, cap, nframes, w, h, q, d_iyuv, stream=None):
        rc = load().myyuv_gpu_dct_decompress_batch_device(self._h, d_payload, d_sizes, cap, nframes, w,
                                                          h, _u8(_q(q)), d_iyuv, stream)
        if rc:
            raise CodecError(rc)

    def sync_status(self, stream=None):
        bad = ctypes.c_int64(-1)
        rc = load().myyuv_hip_sync_status(self._h, stream, ctypes.byref(bad))
        return rc, bad.value

    def profile(self, enable, kernels=None):
        """Per-kernel event stamping: all kernels, or only the named ones."""
        if kernels is None:
            rc = load().myyuv_hip_profile(self._h, 1 if enable else 0)
        else:
            mask = sum(1 << KERNELS_CEIL.index(k) for k in kernels) if enable else 0
            rc = load().myyuv_hip_profile_kernels(self._h, mask)
        if rc:
            raise CodecError(rc)

    def kernel_stats(self):
        """{name: (summed ms, launches)} for every name of KERNELS_CEIL."""
        ms = (ctypes.c_double * K_CEIL)()
        n = (ctypes.c_int64 * K_CEIL)()
        rc = load().myyuv_hip_kernel_stats_n(self._h, K_CEIL, ms, n)
        if rc:
            raise CodecError(rc)
        return {KERNELS_CEIL[i]: (ms[i], n[i]) for i in range(K_CEIL)}

    def tinfo_guard(self, ntiles, arm):
        """Diagnostic (not in include/myyuv_hip.h): arm=True writes a canary
        into the tile-info words past batch tile ntiles; arm=False returns how
        many of them a kernel overwrote since."""
        n = ctypes.c_uint32(0)
        rc = load().myyuv_debug_tinfo_guard(self._h, int(ntiles), 1 if arm else 0, ctypes.byref(n))
        if rc:
            raise CodecError(rc)
        return n.value

    # -- block-level known-answer entry points --
    def fdct_blocks(self, px, qtable):
        px = np.ascontiguousarray(px, np.uint8).reshape(-1, 64)
        qt = np.ascontiguousarray(qtable, np.float32).reshape(64)
        out = np.empty((px.shape[0], 64), np.int16)
        rc = load().myyuv_gpu_fdct_blocks(self._h, _u8(px), px.shape[0],
                                          qt.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)))
        if rc:
            raise CodecError(rc)
        return out

    def fdct_blocks_listed(self, px, qtable):
        """Diagnostic (not in include/myyuv_hip.h): fdct_blocks, and which
        blocks K1 listed for its exact path k_fdct_fix: (coef int16[n, 64]
        zig-zag, listed bool[n], (the number of list entries, the longest of
        the 32 lists)).  RuntimeError when the lists hold what K1 may not
        write (an entry out of range or in the wrong list, a block twice, a
        count above the list's capacity)."""
        px = np.ascontiguousarray(px, np.uint8).reshape(-1, 64)
        qt = np.ascontiguousarray(qtable, np.float32).reshape(64)
        out = np.empty((px.shape[0], 64), np.int16)
        listed = np.zeros(px.shape[0], np.uint8)
        counts = (ctypes.c_uint32 * 2)()
        rc = load().myyuv_debug_fdct_blocks(self._h, _u8(px), px.shape[0],
                                            qt.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), _u8(listed), counts)
        if rc == 101:  # kDiagFixList (myyuv_hip_diag.cpp)
            raise RuntimeError("K1's fix lists are inconsistent")
        if rc:
            raise CodecError(rc)
        return out, listed.astype(bool), (int(counts[0]), int(counts[1]))

    def huff_encode_blocks(self, coef_zz):
        c = np.ascontiguousarray(coef_zz, np.int16).reshape(-1, 64)
        n = c.shape[0]
        chunks = np.zeros((n, 160), np.uint8)
        sizes = np.zeros(n, np.uint8)
        rc = load().myyuv_gpu_huff_encode_blocks(
            self._h, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), n, _u8(chunks), _u8(sizes))
        if rc:
            raise CodecError(rc)
        return [chunks[i, : sizes[i]].tobytes() for i in range(n)]

    def huff_encode_blocks_counted(self, coef_zz, nframes=1):
        """Diagnostic (not in include/myyuv_hip.h): huff_encode_blocks over a
        batch of `nframes` frames (coef_zz: nframes x blocks-per-frame blocks),
        as arrays: (chunks uint8[n, 160] zero-padded, sizes uint8[n], (the
        length of K2's overflow list, of what the CAP-16 tier listed again, the
        overflow passes' and the dense runs' chunk bytes as the tiles' info
        words book them))."""
        c = np.ascontiguousarray(coef_zz, np.int16).reshape(-1, 64)
        n = c.shape[0]
        if nframes < 1 or n % nframes:
            raise ValueError("the block count is not a multiple of nframes")
        chunks = np.zeros((n, 160), np.uint8)
        sizes = np.zeros(n, np.uint8)
        counts = (ctypes.c_uint32 * 4)()
        rc = load().myyuv_debug_huff_encode_blocks(
            self._h, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), n // nframes, nframes, _u8(chunks),
            _u8(sizes), counts)
        if rc:
            raise CodecError(rc)
        return chunks, sizes, tuple(int(x) for x in counts)

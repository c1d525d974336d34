"""IYUV -> BMP (K8), the parts that need no GPU: the restatement
(tests/colorref.py) of the definition in include/myyuv_hip.h against answers
worked by hand, its precision statements, its round trip through K7's oracle,
and the entry points' argument errors (checked before the context is used, so
a null handle reaches them)."""
import ctypes
import functools

import numpy as np
import pytest

import colorref as C


def one(y, u, v):
    """B, G, R of a pixel whose chroma sums are those of the samples (u, v)."""
    return tuple(int(c) for c in C.convert(np.array([y]), np.array([16 * u]), np.array([16 * v]))[0])


# ------------------------------------------------------------ known answers
def test_grey_is_tinted():
    """(128, 128, 128): yf = 128/255 = .50196, uf = vf = 2048/4080 - .5 =
    .0019608; r = .50196 + 1.403 * .0019608 = .504712 -> 128.70 + .5 -> 129;
    g = .50196 - .0014 - .000675 = .499886 -> 127.47 + .5 -> 127;
    b = .50196 + 1.773 * .0019608 = .505437 -> 128.89 + .5 -> 129."""
    assert one(128, 128, 128) == (129, 127, 129)


def test_white_and_black_chroma_extremes():
    """(255, 128, 128): yf = 1; r and b exceed 1 and clamp to 255; g = 1 -
    .0014 - .000675 = .997926 -> 254.47 + .5 -> 254.
    (0, 0, 0): uf = vf = -.5; r = -.7015 and b = -.8865 clamp to 0; g = .357 +
    .172 = .529 -> 134.895 + .5 -> 135."""
    assert one(255, 128, 128) == (255, 254, 255)
    assert one(0, 0, 0) == (0, 135, 0)


def test_4x2_frame_by_hand():
    """A 4x2 frame has a 2x1 chroma plane.  Under LINEAR every vertical
    neighbour clamps onto the one chroma row, columns 0 and 3 clamp
    horizontally too (16 x their sample, as NEAREST), and columns 1 and 2 mix
    12:4 with the other sample.  With one sample value per plane the two modes
    agree everywhere (9 + 3 + 3 + 1 = 16)."""
    y = [10, 60, 110, 160, 210, 250, 30, 90]
    u0, u1, v0, v1 = 100, 180, 90, 200
    fr = bytes(y + [u0, u1, v0, v1])
    su = C.chroma_sums(C.planes(fr, 4, 2)[1], 4, 2, C.LINEAR)[0]
    sv = C.chroma_sums(C.planes(fr, 4, 2)[2], 4, 2, C.LINEAR)[0]
    assert su.tolist() == [[16 * u0, 12 * u0 + 4 * u1, 12 * u1 + 4 * u0, 16 * u1]] * 2
    assert sv.tolist() == [[16 * v0, 12 * v0 + 4 * v1, 12 * v1 + 4 * v0, 16 * v1]] * 2
    lin, near = C.restate(fr, 4, 2, C.LINEAR)[0], C.restate(fr, 4, 2, C.NEAREST)[0]
    assert np.array_equal(lin[:, [0, 3]], near[:, [0, 3]])
    assert not np.array_equal(lin[:, [1, 2]], near[:, [1, 2]])
    # worked by hand, row 0 column 1: Y 60, su = 12*100 + 4*180 = 1920, sv = 12*90 + 4*200 = 1880:
    # yf = .235294, uf = -.029412, vf = -.039216; r = .180274 -> 46.47 -> 46; g = .235294 + .028000 +
    # .010118 = .273412 -> 70.22 -> 70; b = .183147 -> 47.20 -> 47
    assert lin[0, 1].tolist() == [47, 70, 46]
    flat = bytes(y + [140, 140, 77, 77])
    assert np.array_equal(C.restate(flat, 4, 2, C.LINEAR), C.restate(flat, 4, 2, C.NEAREST))


def test_pixel_order_and_alpha():
    fr = C.random_frame(8, 4, 5)
    top = C.pixels(C.restate(fr, 8, 4, C.LINEAR)[0], 32)
    assert (top[..., 3] == 0xFF).all()
    assert C.to_bmp(fr, 8, -4, 32, C.LINEAR) == top.tobytes()
    assert C.to_bmp(fr, 8, 4, 32, C.LINEAR) == top[::-1].tobytes()
    assert C.to_bmp(fr, -8, 4, 32, C.LINEAR) == top.reshape(-1, 4)[::-1].tobytes()
    assert C.to_bmp(fr, 8, -4, 24, C.LINEAR) == top[..., :3].tobytes()


# ------------------------------------------------------- precision statements
@functools.lru_cache(maxsize=None)
def nearest_table():
    return C.nearest_table()


def test_nearest_has_no_fragile_inputs():
    """All 2^24 (Y, U, V) triples give the same bytes in fp32 and in float64;
    77 % of them clamp in some component."""
    t = nearest_table()
    assert np.array_equal(t, C.nearest_table("f64"))
    clamps = ((t == 0) | (t == 255)).any(-1).mean()
    assert 0.76 < clamps < 0.78


def test_exhaustive_frame_holds_every_triple():
    y, u, v = C.planes(C.exhaustive_frame(), 4096, 4096)
    up = lambda p: np.repeat(np.repeat(p[0], 2, 0), 2, 1).astype(np.uint32)
    assert np.unique(y[0].astype(np.uint32) << 16 | up(u) << 8 | up(v)).size == 1 << 24


# --------------------------------------------------- round trip through K7
def test_luma_round_trip_all_triples(oracle):
    """Restatement, then K7's oracle: Y' = (uint8)(0.299 R + 0.587 G + 0.114 B)
    is not a fixed point of Y.  Where a component clamps, colour is lost and Y
    moves far (-80 .. +79 over all triples).  Where none clamps (0 < c < 255),
    the shader's matrix and K7's are inverses to about 1e-3 and the truncating
    cast decides: measured over all 2^24 triples, Y' - Y is -1 for 1,931,259
    of the 3,868,674 unclamped triples and 0 for the rest, never anything else
    (from the restatement and the oracle alone; 24 and 32 bpp alike)."""
    t = nearest_table()
    every = np.broadcast_to(np.arange(256)[:, None, None], t.shape[:3]).reshape(-1)
    for bits in (24, 32):  # all 2^24 triples as a 4096x4096 image: the worst deviation, as measured
        back = oracle.bmp_to_iyuv(C.pixels(t.reshape(-1, 3), bits).tobytes(), 4096, -4096, bits)
        d = np.frombuffer(back, np.uint8)[: 1 << 24].astype(int) - every
        assert (d.min(), d.max()) == (-80, 79)
    inside = ((t > 0) & (t < 255)).all(-1)
    ys = np.broadcast_to(np.arange(256)[:, None, None], inside.shape)[inside]
    px = t[inside]  # (n, 3), n % 8 == 2: pad to a 4-wide, even-height image of unclamped pixels
    n = len(px)
    assert n == 3868674
    pad = (-n) % 8
    px = np.concatenate([px, px[:pad]])
    for bits in (24, 32):
        back = oracle.bmp_to_iyuv(C.pixels(px, bits).tobytes(), 4, -(len(px) // 4), bits)
        d = np.frombuffer(back, np.uint8)[:n].astype(int) - ys
        assert (d.min(), d.max()) == (-1, 0)
        assert int((d == -1).sum()) == 1931259


@pytest.mark.parametrize("sw,sh", C.ORIENTS)
@pytest.mark.parametrize("mode", [C.NEAREST, C.LINEAR])
def test_luma_round_trip_orientations(oracle, sw, sh, mode):
    """A frame with mild chroma (no component clamps) survives restatement ->
    K7 within the same -1 .. 0, pixel for pixel, in all three orientations: K7
    fed the output with the same signs sees the pixels top-down."""
    w, h = 64, 48
    rng = np.random.default_rng(11)
    y = rng.integers(48, 208, w * h, dtype=np.uint8)
    uv = rng.integers(112, 145, w * h // 2, dtype=np.uint8)
    fr = y.tobytes() + uv.tobytes()
    px = C.restate(fr, w, h, mode)
    assert ((px > 0) & (px < 255)).all()
    for bits in (24, 32):
        back = oracle.bmp_to_iyuv(C.to_bmp(fr, sw * w, sh * h, bits, mode), sw * w, sh * h, bits)
        d = np.frombuffer(back, np.uint8)[: w * h].astype(int) - y
        assert (d.min(), d.max()) == (-1, 0)


# ------------------------------------------------------------ argument errors
ARG_CASES = [
    (6, -2, 32, 1, 15),    # |w| % 4: BMP::isValidHeader would refuse the result
    (4, -2, 0, 1, 15),     # bit count 0
    (-4, -2, 32, 1, 16),   # sign cases
    (0, 2, 32, 1, 16),
    (4, 0, 32, 1, 16),
    (4, -3, 32, 1, 17),    # odd height
    (4, -2, 16, 1, 17),    # not 24 / 32 bpp
    (4, -2, 32, 2, 1),     # chroma mode
    (32768, -32768, 32, 0, 1),   # exactly 4 GiB of BGRA
    (4, -2, 32, 1, 1),     # all fine: the null handle is what is left
    (4, -2, 24, 0, 1),
]


@pytest.mark.parametrize("w,h,bits,chroma,code", ARG_CASES)
def test_argument_errors(w, h, bits, chroma, code):
    import myyuv_hip

    L = myyuv_hip.load()
    buf = (ctypes.c_uint8 * 64)()
    out = (ctypes.c_uint8 * 64)()
    assert L.myyuv_gpu_iyuv_to_bmp(None, buf, w, h, bits, chroma, out) == code
    assert L.myyuv_gpu_iyuv_to_bmp_device(None, ctypes.addressof(buf), 1, w, h, bits, chroma,
                                          ctypes.addressof(out), None) == code


def test_null_buffers_and_frame_count():
    import myyuv_hip

    L = myyuv_hip.load()
    buf = (ctypes.c_uint8 * 64)()
    assert L.myyuv_gpu_iyuv_to_bmp(None, None, 4, -2, 32, 1, buf) == myyuv_hip.E_ARG
    assert L.myyuv_gpu_iyuv_to_bmp(None, buf, 4, -2, 32, 1, None) == myyuv_hip.E_ARG
    assert L.myyuv_gpu_iyuv_to_bmp_device(None, ctypes.addressof(buf), 0, 4, -2, 32, 1, ctypes.addressof(buf),
                                          None) == myyuv_hip.E_ARG
    q = (ctypes.c_uint8 * 3)(50, 50, 50)
    bad = ctypes.c_int64(7)
    assert L.myyuv_gpu_dct_decompress_to_bmp(None, buf, 64, 16, -16, q, 32, 1, buf, ctypes.byref(bad)) == myyuv_hip.E_ARG
    assert bad.value == -1


def test_constants_and_kernel_name():
    import myyuv_hip

    assert (myyuv_hip.CHROMA_NEAREST, myyuv_hip.CHROMA_LINEAR) == (C.NEAREST, C.LINEAR) == (0, 1)
    assert myyuv_hip.KERNELS[myyuv_hip.K_IYUV_BMP] == "iyuv_to_bmp"


def test_strerror_is_unchanged():
    import myyuv_hip

    want = ["Success", "Invalid argument", "Level of quality must be between 1 and 100",
            "Error. width % 8 must be 0", "Error. height % 8 must be 0",
            "Output buffer too small for the compressed stream", "DCTYUV load bad size",
            "DCTYUVPlane load bad size", "DCTYUVPlane load chunks_sizes_size bad size",
            "DCTYUVPlane load content_size bad size", "Huffman bad code", "Huffman unknown symbol",
            "Huffman bad chunk", "HIP runtime error", "No HIP device available", "BMP is invalid",
            "Unaccounted width and height sign", "BMP to IYUV needs 24 or 32 bits per pixel and even height",
            "Unknown error"]
    assert [myyuv_hip.strerror(i) for i in range(19)] == want

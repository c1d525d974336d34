"""numpy restatement of IYUV -> BMP (K8, csrc/k_color.hip), the yardstick of
tests/test_yuv_to_bmp.py and tests/test_gpu_yuv_to_bmp.py.

No reference program emits these bytes (the reference converts in a GLSL
fragment shader, myyuv_opengl/viewer/frag_yuv.glsl), so the definition in
include/myyuv_hip.h is restated here operation by operation: fp32, left to
right, every product and sum rounded on its own (numpy never fuses), then the
UNORM8 write floor(clamp(c, 0, 1) * 255 + 0.5).

  restate(...)   the definition (variant "f32"); variants "f64" (the same
                 expression in float64) and "fma" (green's two products
                 contracted into fused multiply-adds) exist only to count the
                 pixels that are sensitive to precision and to contraction
  to_bmp(...)    restate + the BMP pixel order for signed width / height
"""
import numpy as np

NEAREST, LINEAR = 0, 1
ORIENTS = [(1, -1), (-1, 1), (1, 1)]  # BMP::colorData's three sign cases


def planes(iyuv, w, h, nframes=1):
    a = np.frombuffer(bytes(iyuv), np.uint8).reshape(nframes, w * h * 3 // 2)
    y = a[:, : w * h].reshape(nframes, h, w)
    u = a[:, w * h: w * h * 5 // 4].reshape(nframes, h // 2, w // 2)
    v = a[:, w * h * 5 // 4:].reshape(nframes, h // 2, w // 2)
    return y, u, v


def chroma_sums(p, w, h, mode):
    """Per luma pixel the chroma sample sum over 4080 of plane p
    (nframes, h/2, w/2): 16 x the nearest sample, or the 9/3/3/1 sum of
    GL_LINEAR + CLAMP_TO_EDGE at 1:1, clamped inside the frame's own plane."""
    p = p.astype(np.int32)
    x, y = np.arange(w), np.arange(h)
    cx, cy = x >> 1, y >> 1
    if mode == NEAREST:
        return 16 * p[:, cy][:, :, cx]
    nx = np.clip(np.where(x & 1, cx + 1, cx - 1), 0, w // 2 - 1)
    ny = np.clip(np.where(y & 1, cy + 1, cy - 1), 0, h // 2 - 1)
    rc, rn = p[:, cy], p[:, ny]
    return 9 * rc[:, :, cx] + 3 * rc[:, :, nx] + 3 * rn[:, :, cx] + rn[:, :, nx]


def _fused_sub(c, k, x):
    """fl32(c - k * x), k a float32 constant, c and x float32 arrays: one fused
    multiply-add.  The product of two float32 values is exact in float64; the
    sum is rounded to float64 and then to float32 (a double rounding that can
    differ from a true FMA only when the float64 sum lands exactly on a float32
    tie: good enough to count sensitive pixels, which is all the variant is
    for)."""
    return (c.astype(np.float64) - np.float64(np.float32(k)) * x.astype(np.float64)).astype(np.float32)


def convert(y, su, sv, variant="f32"):
    """(Y, su, sv) integer arrays (broadcast against each other) -> uint8
    array of their common shape + (3,): B, G, R."""
    F = np.float64 if variant == "f64" else np.float32
    yf = y.astype(F) / F(255.0)
    uf = su.astype(F) / F(4080.0) - F(0.5)
    vf = sv.astype(F) / F(4080.0) - F(0.5)
    r = yf + F(1.403) * vf
    if variant == "fma":
        g = _fused_sub(_fused_sub(yf, 0.714, vf), 0.344, uf)
    else:
        g = (yf - F(0.714) * vf) - F(0.344) * uf
    b = yf + F(1.773) * uf
    out = np.empty(np.broadcast_shapes(y.shape, su.shape, sv.shape) + (3,), np.uint8)
    for i, c in enumerate((b, g, r)):
        out[..., i] = np.floor(np.minimum(np.maximum(c, F(0.0)), F(1.0)) * F(255.0) + F(0.5)).astype(np.uint8)
    return out


def restate(iyuv, w, h, mode, nframes=1, variant="f32"):
    """IYUV frames -> (nframes, h, w, 3) uint8, rows top-down, B, G, R."""
    y, u, v = planes(iyuv, w, h, nframes)
    return convert(y, chroma_sums(u, w, h, mode), chroma_sums(v, w, h, mode), variant)


def orient(px, width, height):
    """(h, w, bpp) top-down pixels -> the BMP pixel array whose header has the
    signed `width` / `height`: the inverse of BMP::colorData."""
    if width > 0 and height < 0:
        return px
    if width > 0 and height > 0:
        return px[::-1]
    if width < 0 and height > 0:
        return px.reshape(-1, px.shape[-1])[::-1]
    raise ValueError("Unaccounted width and height sign")


def pixels(bgr, bits):
    """(..., 3) B, G, R -> (..., bits/8): 32 bpp appends alpha 0xFF."""
    if bits == 24:
        return bgr
    out = np.full(bgr.shape[:-1] + (4,), 0xFF, np.uint8)
    out[..., :3] = bgr
    return out


def to_bmp(iyuv, width, height, bits, mode, variant="f32"):
    """One frame -> the bytes myyuv_gpu_iyuv_to_bmp writes."""
    w, h = abs(width), abs(height)
    px = pixels(restate(iyuv, w, h, mode, 1, variant)[0], bits)
    return np.ascontiguousarray(orient(px, width, height)).tobytes()


def nearest_table(variant="f32"):
    """[Y, U, V] -> B, G, R under NEAREST, all 2^24 triples."""
    k = np.arange(256)
    return convert(k[:, None, None], 16 * k[None, :, None], 16 * k[None, None, :], variant)


def exhaustive_frame():
    """A 4096x4096 IYUV frame holding every (Y, U, V) triple once under
    NEAREST: the 2048x2048 chroma planes hold every (U, V) pair 64 times, and
    the pair's 64 2x2 luma quads hold Y = 0..255."""
    i = np.arange(1 << 22, dtype=np.uint32).reshape(2048, 2048)
    u = (i >> 14).astype(np.uint8)
    v = ((i >> 6) & 255).astype(np.uint8)
    y = np.empty((4096, 4096), np.uint8)
    for dy in range(2):
        for dx in range(2):
            y[dy::2, dx::2] = ((i & 63) * 4 + 2 * dy + dx).astype(np.uint8)
    return y.tobytes() + u.tobytes() + v.tobytes()


def random_frame(w, h, seed, nframes=1):
    return np.random.default_rng(seed).integers(0, 256, nframes * w * h * 3 // 2, dtype=np.uint8).tobytes()

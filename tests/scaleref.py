"""What a scaled decode must return, restated with numpy from the definition
in include/myyuv_hip.h ("Scaled decode"): the payload parsed with the layout of
DESIGN.md §3, every chunk decoded by the oracle's Huffman decoder, then the
N x N inverse DCT of each block's low-frequency corner in float32 with separate
multiplies and adds.  Never calls the code under test."""
import functools
import struct

import numpy as np

DENOMS = (2, 4, 8)
F = np.float32
# B_N as the header's literals (float.fromhex: exact)
C_ = F(float.fromhex("0x1.6a09e6p-2"))
S_ = F(float.fromhex("0x1.d906bcp-2"))
T_ = F(float.fromhex("0x1.87de2ap-3"))
BASIS = {1: np.array([[C_]], F),
         2: np.array([[C_, C_], [C_, -C_]], F),
         4: np.array([[C_, C_, C_, C_], [S_, T_, -T_, -S_], [C_, -C_, -C_, C_], [T_, -S_, S_, -T_]], F)}


def basis_from_formula(N):
    """B_N[k][i] = fp32(sqrt(N/8) a_k cos((2i+1) k pi / 2N)), in double, rounded once."""
    k = np.arange(N, dtype=np.float64)[:, None]
    i = np.arange(N, dtype=np.float64)[None, :]
    a = np.where(k == 0, np.sqrt(1.0 / N), np.sqrt(2.0 / N))
    return (np.sqrt(N / 8.0) * a * np.cos((2 * i + 1) * k * np.pi / (2 * N))).astype(F)


def round_half_away(x):
    """roundf: sign * floor(|x| + 0.5), in float64 (exact for float32 inputs of
    this size).  np.round rounds half to even and is wrong here."""
    x = np.asarray(x, np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def scaled_blocks(coef_natural, Q_natural, N):
    """[n, 64] int16 natural-order blocks -> [n, N, N] uint8 pixels."""
    z = np.asarray(coef_natural, np.int16).reshape(-1, 8, 8)[:, :N, :N]
    Q = np.asarray(Q_natural, F).reshape(8, 8)[:N, :N]
    B = BASIS[N]
    Z = z.astype(F) * Q
    n = len(Z)
    U = np.zeros((n, N, N), F)
    for i in range(N):
        for k in range(N):
            for j in range(N):
                U[:, i, j] = U[:, i, j] + B[k, i] * Z[:, k, j]
    R = np.zeros((n, N, N), F)
    for i in range(N):
        for k in range(N):
            for j in range(N):
                R[:, i, j] = R[:, i, j] + U[:, i, k] * B[k, j]
    assert U.dtype == F and R.dtype == F
    return np.clip(round_half_away(R).astype(np.int64) + 128, 0, 255).astype(np.uint8)


def parse_planes(payload):
    """[(sizes, content)] of the three planes (u32 plane_size[3],
    per plane u32 nblk, u32 content_size, nblk size bytes, the chunks)."""
    payload = bytes(payload)
    ps = struct.unpack_from("<III", payload, 0)
    off, out = 12, []
    for p in range(3):
        nblk, csize = struct.unpack_from("<II", payload, off)
        sizes = payload[off + 8:off + 8 + nblk]
        content = payload[off + 8 + nblk:off + 8 + nblk + csize]
        out.append((sizes, content))
        off += ps[p]
    return out


@functools.lru_cache(maxsize=8)
def coefficients(payload):
    """Per plane the [nblk, 64] int16 natural-order coefficients (shared
    between the scales: not to be modified)."""
    from oracle import oracle as O

    memo, out = {}, []
    for sizes, content in parse_planes(payload):
        blocks = np.empty((len(sizes), 64), np.int16)
        pos = 0
        for k, s in enumerate(sizes):
            ch = content[pos:pos + s]
            b = memo.get(ch)
            if b is None:
                b = memo[ch] = np.asarray(O.huff_decode_block(ch), np.int16).reshape(64).copy()
            blocks[k] = b
            pos += s
        out.append(blocks)
    return out


def decode_scaled(payload, w, h, q, denom):
    """The (w/denom) x (h/denom) IYUV frame, as bytes."""
    from oracle import oracle as O

    assert denom in DENOMS and w % 16 == 0 and h % 16 == 0
    N = 8 // denom
    out = []
    for p, blocks in enumerate(coefficients(bytes(payload))):
        pw, ph = (w, h) if p == 0 else (w // 2, h // 2)
        bw, bh = pw // 8, ph // 8
        assert len(blocks) == bw * bh
        px = scaled_blocks(blocks, O.qtable(q[p], p != 0), N)
        out.append(px.reshape(bh, bw, N, N).transpose(0, 2, 1, 3).reshape(bh * N, bw * N).tobytes())
    res = b"".join(out)
    assert len(res) == w * h * 3 // 2 // (denom * denom)
    return res


@functools.lru_cache(maxsize=None)
def cached(payload, w, h, q, denom):
    """decode_scaled, computed once per (stream, scale) and shared by the tests."""
    return decode_scaled(payload, w, h, tuple(q), denom)

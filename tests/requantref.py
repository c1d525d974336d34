"""What a requantise must return, restated with numpy from the definition in
include/myyuv_hip.h ("Requantise"): the payload parsed with the layout of
DESIGN.md §3, every chunk decoded by the oracle's Huffman decoder, each
coefficient rescaled in float32 (multiply, then divide), rounded half away
from zero and clamped to the chunk format's 11 bits, and the blocks written
out again by the oracle's Huffman encoder (coefgen.build_payload).  Never calls
the code under test."""
import functools

import numpy as np

import coefgen
import scaleref as S

F = np.float32
COEF_MIN, COEF_MAX = -1024, 1023
_CHUNKS = None


def round_half_away(x):
    """roundf of float32 values: widened to float64 first, where |x| + 0.5 is
    exact (floor(x + 0.5) in float32 is wrong just below a .5)."""
    x = np.asarray(x)
    assert x.dtype == F
    x = x.astype(np.float64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def quotients(z, Qs, Qd):
    """t = ((float)z * Qs) / Qd, both operations in float32."""
    z = np.asarray(z, np.int16).astype(F)
    Qs, Qd = np.asarray(Qs, F), np.asarray(Qd, F)
    prod = z * Qs
    assert prod.dtype == F
    t = prod / Qd
    assert t.dtype == F
    return t


def requant(z, Qs, Qd):
    """int16 coefficients (any shape broadcastable with the tables) -> z'."""
    return np.clip(round_half_away(quotients(z, Qs, Qd)), COEF_MIN, COEF_MAX).astype(np.int16)


def is_tie(t):
    """float32 quotients whose fractional part is exactly .5."""
    t = np.asarray(t, F).astype(np.float64)
    return np.abs(t - np.trunc(t)) == 0.5


def tables(q, oracle):
    return [np.asarray(oracle.qtable(q[p], p != 0), F) for p in range(3)]


def requant_planes(payload, q_src, q_dst):
    """Per plane: ([nblk, 64] requantised natural-order blocks, the float32
    quotients they were rounded from).  The source coefficients are
    scaleref.coefficients' (shared, not modified)."""
    from oracle import oracle as O

    Qs, Qd = tables(q_src, O), tables(q_dst, O)
    out = []
    for p, nat in enumerate(S.coefficients(bytes(payload))):
        t = quotients(nat, Qs[p][None, :], Qd[p][None, :])
        out.append((np.clip(round_half_away(t), COEF_MIN, COEF_MAX).astype(np.int16), t))
    return out


def requantize(payload, q_src, q_dst):
    """The requantised DCTYUV payload, as bytes."""
    from oracle import oracle as O

    global _CHUNKS
    if _CHUNKS is None:
        _CHUNKS = coefgen.Chunks(O.huff_encode_block)  # the oracle's chunk per distinct block, once
    planes = [nat[:, coefgen.ZZ] for nat, _ in requant_planes(payload, q_src, q_dst)]  # build_payload: zig-zag
    return coefgen.build_payload(planes, _CHUNKS)


@functools.lru_cache(maxsize=None)
def cached(payload, q_src, q_dst):
    """requantize, computed once per (stream, quality pair) and shared by the tests."""
    return requantize(payload, tuple(q_src), tuple(q_dst))

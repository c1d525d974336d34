"""What a transform must return, restated with numpy from the definition in
include/myyuv_hip.h ("Transform"): every chunk decoded by the oracle's Huffman
decoder (scaleref.coefficients), each block transposed for a swap, rescaled by
requantref.requant between the source table at the source position and the
destination table at the destination position, negated where the mirrors say
so and clamped, placed at its destination block, and the blocks written out
again by the oracle's Huffman encoder (coefgen.build_payload).  Also the pixel
mover the pixel tests compare against.  Never calls the code under test."""
import functools

import numpy as np

import coefgen
import requantref as Q
import scaleref as S

NAMES = {"none": 0, "flip_h": 1, "flip_v": 2, "rot180": 3, "transpose": 4, "rot90": 5, "rot270": 6, "transverse": 7}
OPS = tuple(range(8))
MX, MY, SWAP = 1, 2, 4
_CHUNKS = None


def out_size(w, h, op):
    return (h, w) if op & SWAP else (w, h)


def plane_shapes(w, h):
    """(bw, bh) in blocks of the three planes."""
    return [(w // 8, h // 8), (w // 16, h // 16), (w // 16, h // 16)]


def block_map(op, bw, bh):
    """dest[k]: the destination index of source block k = by * bw + bx, straight
    from the definition's formulas."""
    by, bx = np.divmod(np.arange(bw * bh, dtype=np.int64), bw)
    if op & SWAP:
        bx1, by1, bw1, bh1 = by, bx, bh, bw
    else:
        bx1, by1, bw1, bh1 = bx, by, bw, bh
    bxd = bw1 - 1 - bx1 if op & MX else bx1
    byd = bh1 - 1 - by1 if op & MY else by1
    return byd * bw1 + bxd


def signs(op):
    """[8, 8] of +-1 at the destination position (u', v')."""
    u, v = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    neg = (bool(op & MX) & (v % 2 == 1)) ^ (bool(op & MY) & (u % 2 == 1))
    return np.where(neg, -1, 1).astype(np.int64)


def xform_blocks(z, op, Qs, Qd):
    """[n, 64] int16 natural-order blocks -> the blocks z' (same order of blocks)."""
    z = np.asarray(z, np.int16).reshape(-1, 8, 8)
    Qs, Qd = np.asarray(Qs, Q.F).reshape(8, 8), np.asarray(Qd, Q.F).reshape(8, 8)
    if op & SWAP:  # z'[u'][v'] comes from z[v'][u'], with Qs[v'][u'] and Qd[u'][v']
        z, Qs = z.transpose(0, 2, 1), Qs.T
    z1 = Q.requant(z, Qs[None], Qd[None]).astype(np.int64)
    return np.clip(signs(op)[None] * z1, Q.COEF_MIN, Q.COEF_MAX).astype(np.int16).reshape(-1, 64)


def xform_planes(planes, w, h, op, q_src, q_dst):
    """Per plane the [nblk, 64] natural-order blocks in the destination's block order."""
    from oracle import oracle as O

    Qs, Qd = Q.tables(q_src, O), Q.tables(q_dst, O)
    out = []
    for p, (nat, (bw, bh)) in enumerate(zip(planes, plane_shapes(w, h))):
        assert len(nat) == bw * bh
        dest = block_map(op, bw, bh)
        assert sorted(dest.tolist()) == list(range(bw * bh))
        moved = np.empty((bw * bh, 64), np.int16)
        moved[dest] = xform_blocks(nat, op, Qs[p], Qd[p])
        out.append(moved)
    return out


def transform(payload, w, h, q_src, op, q_dst):
    """The transformed DCTYUV payload, as bytes."""
    from oracle import oracle as O

    global _CHUNKS
    if _CHUNKS is None:
        _CHUNKS = coefgen.Chunks(O.huff_encode_block)
    planes = xform_planes(S.coefficients(bytes(payload)), w, h, op, q_src, q_dst)
    return coefgen.build_payload([nat[:, coefgen.ZZ] for nat in planes], _CHUNKS)


@functools.lru_cache(maxsize=None)
def cached(payload, w, h, q_src, op, q_dst):
    """transform, computed once per input and shared by the tests."""
    return transform(payload, w, h, tuple(q_src), op, tuple(q_dst))


# ---- pixels ----------------------------------------------------------------
def move_plane(a, op):
    """A 2-D array moved by op: transpose first, then the mirrors."""
    if op & SWAP:
        a = a.T
    if op & MX:
        a = a[:, ::-1]
    if op & MY:
        a = a[::-1, :]
    return a


def move_iyuv(iyuv, w, h, op):
    """The IYUV frame (bytes) moved by op; its size is out_size(w, h, op)."""
    a = np.frombuffer(bytes(iyuv), np.uint8)
    assert a.size == w * h * 3 // 2
    planes = (a[:w * h].reshape(h, w), a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2),
              a[w * h * 5 // 4:].reshape(h // 2, w // 2))
    return b"".join(np.ascontiguousarray(move_plane(p, op)).tobytes() for p in planes)


def check_mover():
    """The pixel mover equals numpy's own functions for the named operations."""
    a = np.arange(6 * 10).reshape(6, 10)
    want = {"none": a, "flip_h": np.flip(a, 1), "flip_v": np.flip(a, 0), "rot180": np.rot90(a, 2),
            "transpose": a.T, "rot90": np.rot90(a, -1), "rot270": np.rot90(a, 1),
            "transverse": np.rot90(a, 2).T}
    for name, op in NAMES.items():
        assert np.array_equal(move_plane(a, op), want[name]), name
    H, W = a.shape
    r = move_plane(a, NAMES["rot90"])
    assert all(r[y, x] == a[H - 1 - x, y] for y in range(W) for x in range(H))  # out[y][x] = in[H-1-x][y]
    return True

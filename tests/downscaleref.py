"""What a downscale must return (include/myyuv_hip.h, "Downscale"):

    compress(decompress_scaled(x, q_src, denom), q_dst)

with decompress_scaled the numpy restatement scaleref and compress the
oracle's.  Never calls the code under test.  Also csrc/downscale.h's work map
restated with numpy, for the host test."""
import functools

import numpy as np

import scaleref as S

DENOMS = S.DENOMS
SEG = 64  # downscale.h kSeg


def q3(q):
    return (q, q, q) if isinstance(q, int) else tuple(q)


@functools.lru_cache(maxsize=None)
def cached(payload, w, h, q_src, denom, q_dst):
    """The expected stream, computed once per case and shared by the tests."""
    from oracle import oracle as O

    return O.compress(S.cached(bytes(payload), w, h, tuple(q_src), denom), w // denom, h // denom, tuple(q_dst))


def valid(w, h, denom):
    return denom in DENOMS and w > 0 and h > 0 and w % (16 * denom) == 0 and h % (16 * denom) == 0


def work_map(w, h, denom):
    """One row per source block, sorted as the host program walks them (wave,
    run, lane): [wave, plane, run, lane, source block, output block, slot,
    first pixel's byte in the wave's image], uint32."""
    assert valid(w, h, denom)
    N = 8 // denom
    rows, wave0 = [], 0
    for p in range(3):
        sh = 3 if p == 0 else 4
        sbw, sbh = w >> sh, h >> sh
        dbw, dbh = sbw // denom, sbh // denom
        spr = -(-sbw // SEG)
        sy, sx = np.divmod(np.arange(sbw * sbh, dtype=np.int64), sbw)
        oy, r = np.divmod(sy, denom)
        k, lane = np.divmod(sx, SEG)
        wave = wave0 + oy * spr + k
        slot, c = np.divmod(lane, denom)
        out_block = oy * dbw + sx // denom
        pix = 64 * slot + 8 * (r * N) + N * c
        rows.append(np.stack([wave, np.full_like(wave, p), r, lane, sy * sbw + sx, out_block, slot, pix], axis=1))
        wave0 += spr * dbh
    m = np.concatenate(rows)
    order = np.lexsort((m[:, 3], m[:, 2], m[:, 0]))
    return m[order].astype(np.uint32)


def plane_blocks(w, h, denom):
    """Per plane (source blocks per row, source block rows, output blocks per row, output block rows)."""
    out = []
    for p in range(3):
        sh = 3 if p == 0 else 4
        out.append((w >> sh, h >> sh, (w >> sh) // denom, (h >> sh) // denom))
    return out

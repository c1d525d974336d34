"""What a region decode must return, stated with numpy: the crop of a full
decode (include/myyuv_hip.h, region decode).  The full decode itself comes from
the oracle, never from the code under test."""
import functools
import os

import numpy as np

import synth
from conftest import GOLDEN


def crop(iyuv, w, h, region):
    """The rw x rh IYUV frame (bytes) cut from the w x h frame `iyuv` at
    region = (rx, ry, rw, rh), luma pixels, top-down: Y, then U and V at half
    the coordinates."""
    rx, ry, rw, rh = region
    assert rx % 2 == 0 and ry % 2 == 0 and rw % 2 == 0 and rh % 2 == 0
    assert 0 <= rx and 0 <= ry and rx + rw <= w and ry + rh <= h
    a = np.frombuffer(bytes(iyuv), np.uint8)
    assert a.size == w * h * 3 // 2
    y = a[: w * h].reshape(h, w)
    u = a[w * h: w * h * 5 // 4].reshape(h // 2, w // 2)
    v = a[w * h * 5 // 4:].reshape(h // 2, w // 2)
    cx, cy, cw, ch = rx // 2, ry // 2, rw // 2, rh // 2
    return b"".join(p.tobytes() for p in (y[ry:ry + rh, rx:rx + rw], u[cy:cy + ch, cx:cx + cw],
                                          v[cy:cy + ch, cx:cx + cw]))


def blocks(w, h):
    """Blocks per plane (Y, U, V) of a w x h frame."""
    return (w // 8) * (h // 8), (w // 16) * (h // 16), (w // 16) * (h // 16)


def block_rect(w, h, plane, k):
    """The 16-aligned luma rectangle around block k (row-major) of `plane`."""
    bw = w // 8 if plane == 0 else w // 16
    px = 8 if plane == 0 else 16  # luma pixels per block of the plane
    x, y = (k % bw) * px, (k // bw) * px
    return x & ~15, y & ~15, 16, 16


def contains_block(w, h, region, g):
    """Whether frame-global block g (plane-major, row-major) lies in the region."""
    rx, ry, rw, rh = region
    ny, nc, _ = blocks(w, h)
    plane = 0 if g < ny else (1 if g < ny + nc else 2)
    k = g - (0, ny, ny + nc)[plane]
    bw = w // 8 if plane == 0 else w // 16
    px = 8 if plane == 0 else 16
    x, y = (k % bw) * px, (k // bw) * px
    return rx <= x < rx + rw and ry <= y < ry + rh


@functools.lru_cache(maxsize=None)
def chef():
    import myyuv_file

    return myyuv_file.YUVFile.load(os.path.join(GOLDEN, "chef-with-trumpet.myyuv"))


@functools.lru_cache(maxsize=None)
def tiled_stream(w, h, q, ox=400, oy=300):
    """(payload, full decode) of the w x h window of the golden chef frame at
    (ox, oy), wrapped (synth.tiled_frame), compressed by the oracle at q."""
    from oracle import oracle as O

    f = chef()
    raw = synth.tiled_frame(f.data, f.width, f.height, w, h, ox, oy).tobytes()
    pay = O.compress(raw, w, h, q)
    return pay, O.decompress(pay, w, h, q)


@functools.lru_cache(maxsize=None)
def noise_stream(w, h, q=(100, 100, 100)):
    from oracle import oracle as O

    raw = synth.noise_frame(w, h).tobytes()
    pay = O.compress(raw, w, h, q)
    return pay, O.decompress(pay, w, h, q)

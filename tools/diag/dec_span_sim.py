#!/usr/bin/env python3
"""CPU simulation of the span decoder's work (k_decode_span):
from the oracle's coefficients of the bench frame (chef-big, 4032x3008), the
decode passes and the symbol-loop wave-positions per frame when a wave owns a
span of S consecutive blocks of one plane, finishes the one-symbol chunks in
closed form and decodes the others in passes of 64 in block order.  S = 64
with every block "real" is today's k_decode_idct (a pass per 64-block group).

A pass's symbol loop runs to its longest message: wave-positions = the sum
of that length over the passes (77.8k per frame for today's decoder at q50).

  python3 tools/diag/dec_span_sim.py [quality, default 50]"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yuv-manipulations-2_amd")]


def plane_chunks(payload):
    """Per plane: the list of chunks (u32 plane_size[3]; per plane u32
    nblocks, u32 content_size, u8 size[nblocks], the chunks)."""
    out, pos = [], 12
    for p in range(3):
        ps = struct.unpack_from("<I", payload, 4 * p)[0]
        nb, _ = struct.unpack_from("<II", payload, pos)
        sizes = np.frombuffer(payload, np.uint8, nb, pos + 8)
        offs = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]) + pos + 8 + nb
        out.append([bytes(payload[offs[i]:offs[i + 1]]) for i in range(nb)])
        pos += ps
    return out


def is_closed_form(c):
    return len(c) == 7 and c[:4] == b"\x01\x00\x03\x00" and c[5] < 8 and c[6] == 0


def main():
    import myyuv_file
    from oracle import oracle as O

    q = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    g = myyuv_file.YUVFile.load(os.path.join(ROOT, "tests", "golden", "chef-with-trumpet-big-DCT-50.myyuv"))
    w, h = g.width, g.height
    payload = g.data
    if q != 50:
        raw = O.decompress(g.data, w, h, tuple(g.params))
        payload = O.compress(raw, w, h, (q, q, q))
    planes = []
    memo = {}
    for chunks in plane_chunks(payload):
        msz = np.zeros(len(chunks), np.int64)
        single = np.zeros(len(chunks), bool)
        for i, c in enumerate(chunks):
            m = memo.get(c)
            if m is None:
                nat = np.asarray(O.huff_decode_block(c)).reshape(64)
                nz = np.nonzero(nat[ZZ])[0]
                m = memo[c] = (int(nz[-1]) + 1 if len(nz) else 0, is_closed_form(c))
            msz[i], single[i] = m
        planes.append((msz, single))
    nblk = sum(len(m) for m, _ in planes)
    nsingle = sum(int(s.sum()) for _, s in planes)
    print(f"{w}x{h} q{q}: {nblk} blocks, {100.0 * nsingle / nblk:.1f} % one-symbol closed forms")

    def positions(lengths):  # one pass: to the longest message
        return int(lengths.max())

    base = None
    print(f"{'S':>12} {'passes':>8} {'per 64 blocks':>14} {'wave-positions':>15}")
    for S in (0, 128, 256, 512):
        npass = npos = 0
        for msz, single in planes:
            if S == 0:  # today: a pass per 64-block group, every block in it
                for a in range(0, len(msz), 64):
                    npass += 1
                    npos += positions(msz[a:a + 64])
                continue
            for a in range(0, len(msz), S):
                real = msz[a:a + S][~single[a:a + S]]
                for b in range(0, len(real), 64):
                    npass += 1
                    npos += positions(real[b:b + 64])
        base = base or (npass, npos)
        print(f"{'64 (today)' if S == 0 else S:>12} {npass:8d} {npass / base[0]:14.2f} {npos:10d} ({npos / base[1]:.2f})")


ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
               41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15,
               23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

if __name__ == "__main__":
    main()

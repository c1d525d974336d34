"""What the JPEG export must write, restated in Python from the definition in
include/myyuv_hip.h ("Export to JPEG"), and an independent baseline parser that
reads such a file back to coefficients.  Never calls the code under test.

export(payload, w, h, q)  the file's bytes, from scaleref.coefficients (the
                          oracle's Huffman decode of every chunk) and
                          oracle.qtable;
export_planes(planes, w, h, qtables)  the same from coefficient planes;
parse(data)               markers, DQT, DHT, DRI and SOS read, the entropy data
                          un-stuffed, the RST sequence checked, every block
                          Huffman-decoded with the file's own tables and the DC
                          prediction undone: (w, h, planes, qtables), natural
                          order.
"""
import functools
import struct

import numpy as np

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
               41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15,
               23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
RESTART = 64

# ITU-T T.81 Annex K.3-K.6 (BITS, HUFFVAL)
DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHR = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
AC_CHR = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
# in the file's order, with the DHT segment's Tc/Th byte
DHT = ((0x00, DC_LUM), (0x10, AC_LUM), (0x01, DC_CHR), (0x11, AC_CHR))


def codes(bits, vals):
    """{symbol: (code, length)} of Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    assert k == len(vals)
    return out


def seg(marker, body):
    return struct.pack(">HH", marker, len(body) + 2) + bytes(body)


def header(w, h, qtables):
    """SOI to DRI.  qtables: three natural-order tables of 64 integers 1..255."""
    out = [b"\xff\xd8", seg(0xFFE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))]
    for p in range(3):
        t = np.asarray(qtables[p]).reshape(64)
        assert t.min() >= 1 and t.max() <= 255 and (t == np.round(t)).all()
        out.append(seg(0xFFDB, bytes([p]) + bytes(int(v) for v in t[ZZ])))
    out.append(seg(0xFFC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 2])))
    for tc_th, (bits, vals) in DHT:
        out.append(seg(0xFFC4, bytes([tc_th]) + bytes(bits) + bytes(vals)))
    out.append(seg(0xFFDD, struct.pack(">H", RESTART)))
    return b"".join(out)


def category(v):
    return int(abs(int(v))).bit_length()


def interval_bytes(zz_blocks, dc_codes, ac_codes):
    """One restart interval: blocks [n, 64] in zig-zag order -> stuffed bytes."""
    acc, n, pred = 0, 0, 0
    for b in zz_blocks:
        b = [int(v) for v in b]
        d = b[0] - pred
        pred = b[0]
        c = category(d)
        assert c <= 11
        code, length = dc_codes[c]
        acc = (acc << length) | code
        acc = (acc << c) | ((d if d >= 0 else d - 1) & ((1 << c) - 1))
        n += length + c
        run = 0
        for v in b[1:]:
            if v == 0:
                run += 1
                continue
            v = max(v, -1023)  # baseline has no AC category 11
            while run >= 16:
                code, length = ac_codes[0xF0]
                acc = (acc << length) | code
                n += length
                run -= 16
            c = category(v)
            assert 1 <= c <= 10
            code, length = ac_codes[(run << 4) | c]
            acc = (acc << length) | code
            acc = (acc << c) | ((v if v >= 0 else v - 1) & ((1 << c) - 1))
            n += length + c
            run = 0
        if run:
            code, length = ac_codes[0x00]
            acc = (acc << length) | code
            n += length
    pad = -n % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((n + pad) // 8, "big").replace(b"\xff", b"\xff\x00")


def export_planes(planes, w, h, qtables):
    """planes: per plane [nblk, 64] int16 in NATURAL order, raster block order."""
    assert w % 16 == 0 and h % 16 == 0 and 0 < w <= 65535 and 0 < h <= 65535
    out = [header(w, h, qtables)]
    for p, nat in enumerate(planes):
        nat = np.asarray(nat, np.int16).reshape(-1, 64)
        assert len(nat) == ((w // 8) * (h // 8) if p == 0 else (w // 16) * (h // 16))
        zz = nat[:, ZZ]
        dc_codes, ac_codes = (codes(*DC_LUM), codes(*AC_LUM)) if p == 0 else (codes(*DC_CHR), codes(*AC_CHR))
        out.append(seg(0xFFDA, bytes([1, p + 1, 0x00 if p == 0 else 0x11, 0, 63, 0])))
        for m, k0 in enumerate(range(0, len(zz), RESTART)):
            if m:
                out.append(bytes([0xFF, 0xD0 + (m - 1) % 8]))
            out.append(interval_bytes(zz[k0:k0 + RESTART], dc_codes, ac_codes))
    out.append(b"\xff\xd9")
    return b"".join(out)


def qtables_of(q):
    from oracle import oracle as O

    return [np.asarray(O.qtable(q[p], p != 0)).reshape(64) for p in range(3)]


@functools.lru_cache(maxsize=None)
def export(payload, w, h, q):
    """The file of a stream (computed once per stream and shared)."""
    import scaleref as S

    return export_planes(S.coefficients(bytes(payload)), w, h, qtables_of(tuple(q)))


# ---- the parser -------------------------------------------------------------
class _Bits:
    def __init__(self, data):
        self.v = int.from_bytes(data, "big")
        self.n = 8 * len(data)
        self.pos = 0

    def peek16(self):
        left = self.n - self.pos
        if left >= 16:
            return (self.v >> (left - 16)) & 0xFFFF
        return ((self.v & ((1 << left) - 1)) << (16 - left)) | ((1 << (16 - left)) - 1)

    def take(self, k):
        assert self.pos + k <= self.n, "entropy data ends inside a block"
        left = self.n - self.pos
        self.pos += k
        return (self.v >> (left - k)) & ((1 << k) - 1)


def _lookup(bits, vals):
    """16-bit prefix -> (symbol, length), or None."""
    tab = [None] * 65536
    for sym, (code, length) in codes(bits, vals).items():
        lo = code << (16 - length)
        for i in range(lo, lo + (1 << (16 - length))):
            tab[i] = (sym, length)
    return tab


def _symbol(br, tab):
    e = tab[br.peek16()]
    assert e is not None, "no such code"
    br.take(e[1])
    return e[0]


def _extend(v, c):
    return v if c == 0 or v >= (1 << (c - 1)) else v - (1 << c) + 1


def _decode_interval(data, nblocks, dc_tab, ac_tab):
    br = _Bits(data)
    out = np.zeros((nblocks, 64), np.int16)
    pred = 0
    for i in range(nblocks):
        c = _symbol(br, dc_tab)
        assert c <= 11
        pred += _extend(br.take(c), c)
        out[i, 0] = pred
        k = 1
        while k < 64:
            rs = _symbol(br, ac_tab)
            r, c = rs >> 4, rs & 15
            if c == 0:
                if r == 15:
                    k += 16
                    assert k < 64, "ZRL past the block"
                    continue
                assert r == 0
                break
            k += r
            assert k < 64, "run past the block"
            out[i, k] = _extend(br.take(c), c)
            k += 1
    left = br.n - br.pos
    assert left < 8 and br.take(left) == (1 << left) - 1, "padding is 1-bits, less than a byte"
    return out


def parse(data):
    """(w, h, [natural-order int16 [nblk, 64] per plane], [natural-order int[64] per plane])."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    pos = 2
    qt, huff, frame, ri = {}, {}, None, 0
    planes = {}
    while True:
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        if m == 0xD9:
            assert pos + 2 == len(data), "bytes after EOI"
            break
        n = struct.unpack_from(">H", data, pos + 2)[0]
        body = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if m == 0xE0:
            assert body[:5] == b"JFIF\0"
        elif m == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZZ] = list(body[1:65])
                qt[body[0] & 15] = t
                body = body[65:]
        elif m == 0xC0:
            prec, h, w, nc = struct.unpack_from(">BHHB", body, 0)
            assert prec == 8 and nc == 3
            frame = (w, h, [tuple(body[6 + 3 * i:9 + 3 * i]) for i in range(3)])
            assert [c[1] for c in frame[2]] == [0x22, 0x11, 0x11]
        elif m == 0xC4:
            while body:
                bits = list(body[1:17])
                nv = sum(bits)
                huff[body[0]] = _lookup(bits, list(body[17:17 + nv]))
                body = body[17 + nv:]
        elif m == 0xDD:
            ri = struct.unpack(">H", body)[0]
        elif m == 0xDA:
            assert frame is not None and ri > 0
            assert body[0] == 1 and tuple(body[3:6]) == (0, 63, 0)
            cid, tabs = body[1], body[2]
            idx = [c[0] for c in frame[2]].index(cid)
            w, h, comps = frame
            nblk = (w // 8) * (h // 8) if idx == 0 else (w // 16) * (h // 16)
            # the entropy data: up to the next marker that is neither FF00 nor RSTm
            chunks, cur, expect = [], bytearray(), 0
            while True:
                j = data.index(b"\xff", pos)
                cur += data[pos:j]
                nxt = data[j + 1]
                if nxt == 0x00:
                    cur.append(0xFF)
                    pos = j + 2
                elif 0xD0 <= nxt <= 0xD7:
                    assert nxt == 0xD0 + expect % 8, "RST out of sequence"
                    expect += 1
                    chunks.append(bytes(cur))
                    cur = bytearray()
                    pos = j + 2
                else:
                    chunks.append(bytes(cur))
                    pos = j
                    break
            assert len(chunks) == -(-nblk // ri), (len(chunks), nblk)
            dc_tab, ac_tab = huff[tabs >> 4], huff[0x10 | (tabs & 15)]
            parts = [_decode_interval(ch, min(ri, nblk - i * ri), dc_tab, ac_tab) for i, ch in enumerate(chunks)]
            zz = np.concatenate(parts)
            nat = np.zeros_like(zz)
            nat[:, ZZ] = zz
            planes[idx] = nat
        else:
            raise AssertionError(f"unexpected marker {m:#x}")
    w, h, comps = frame
    assert sorted(planes) == [0, 1, 2]
    return w, h, [planes[i] for i in range(3)], [qt[comps[i][2]] for i in range(3)]


def dht_segments(data):
    """{Tc/Th byte: (BITS, HUFFVAL)} of a JPEG file's DHT segments."""
    data, pos, out = bytes(data), 2, {}
    while data[pos + 1] != 0xDA:
        n = struct.unpack_from(">H", data, pos + 2)[0]
        if data[pos + 1] == 0xC4:
            body = data[pos + 4:pos + 2 + n]
            while body:
                bits = list(body[1:17])
                nv = sum(bits)
                out[body[0]] = (bits, list(body[17:17 + nv]))
                body = body[17 + nv:]
        pos += 2 + n
    return out

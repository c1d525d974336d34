"""What the JPEG import must read, restated in Python from the definition in
include/myyuv_hip.h ("Import from JPEG").  Never calls the code under test.

parse(data)   an independent baseline parser for 4:2:0 files with one
              interleaved scan or three non-interleaved ones: markers, DQT, DHT
              and DRI read (several tables per segment, fill bytes, APPn / COM
              skipped), the entropy data cut at the RSTm markers and un-stuffed,
              every block Huffman-decoded with the scan's own tables and the DC
              prediction undone, every block put at its place in the file's
              MCU-padded grid: a Parsed.
write(...)    the reverse: a file of either scan layout from coefficient
              planes, with a chosen restart interval per scan and chosen
              Huffman tables, so crafted files need no Pillow.
stream(...)   the DCT stream an import must return for given planes (the
              oracle's Huffman encoder over coefgen.build_payload).
"""
import functools
import struct

import numpy as np

import coefgen
import jpegref as J

ZZ = J.ZZ
DEFAULT_DHT = {tc_th: (tuple(b), tuple(v)) for tc_th, (b, v) in J.DHT}
_CHUNKS = None


class Parsed:
    def __init__(self):
        self.W = self.H = self.Wp = self.Hp = 0
        self.planes = None   # per plane int16 [nblk, 64], natural order, the padded grid's raster order
        self.qt = None       # per plane int[64], natural order
        self.interleaved = False
        self.ri = []         # per scan
        self.segments = 0    # restart intervals of all scans


def grid(W, H):
    """Blocks per row and rows of the padded grid, per plane."""
    mx, my = -(-W // 16), -(-H // 16)
    return [(2 * mx, 2 * my), (mx, my), (mx, my)]


def own(W, H):
    """A component's own blocks in a non-interleaved scan."""
    return [(-(-W // 8), -(-H // 8)), (-(-W // 16), -(-H // 16)), (-(-W // 16), -(-H // 16))]


@functools.lru_cache(maxsize=None)
def _lookup(bits, vals):
    return J._lookup(list(bits), list(vals))


def _decode_block(br, dc_tab, ac_tab, pred):
    """One block in zig-zag order, and the new predictor."""
    out = np.zeros(64, np.int16)
    c = J._symbol(br, dc_tab)
    assert c <= 11
    pred += J._extend(br.take(c), c)
    assert -1024 <= pred <= 1023
    out[0] = pred
    k = 1
    while k < 64:
        rs = J._symbol(br, ac_tab)
        r, c = rs >> 4, rs & 15
        if c == 0:
            if r == 15:
                k += 16
                assert k < 64, "ZRL past the block"
                continue
            assert r == 0
            break
        assert c <= 10
        k += r
        assert k < 64, "run past the block"
        out[k] = J._extend(br.take(c), c)
        k += 1
    return out, pred


def parse(data):
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    pos = 2
    qt, huff, frame, ri = {}, {}, None, 0
    P = Parsed()
    zz = None
    covered = set()
    while True:
        assert data[pos] == 0xFF, pos
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0xD9:
            break
        n = struct.unpack_from(">H", data, pos)[0]
        body = data[pos + 2:pos + n]
        pos += n
        if m == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZZ] = list(body[1:65])
                qt[body[0] & 15] = t
                body = body[65:]
        elif m == 0xC0:
            prec, h, w, nc = struct.unpack_from(">BHHB", body, 0)
            assert prec == 8 and nc == 3
            frame = [tuple(body[6 + 3 * i:9 + 3 * i]) for i in range(3)]
            assert [c[1] for c in frame] == [0x22, 0x11, 0x11]
            P.W, P.H = w, h
            P.Wp, P.Hp = -(-w // 16) * 16, -(-h // 16) * 16
            zz = [np.zeros((gw * gh, 64), np.int16) for gw, gh in grid(w, h)]
            P.qt = [None] * 3
        elif m == 0xC4:
            while body:
                bits = tuple(body[1:17])
                nv = sum(bits)
                huff[body[0]] = _lookup(bits, tuple(body[17:17 + nv]))
                body = body[17 + nv:]
        elif m == 0xDD:
            ri = struct.unpack(">H", body)[0]
        elif m == 0xDA:
            assert frame is not None
            ns = body[0]
            assert ns in (1, 3) and tuple(body[1 + 2 * ns:4 + 2 * ns]) == (0, 63, 0)
            comps = []
            for j in range(ns):
                idx = [c[0] for c in frame].index(body[1 + 2 * j])
                assert idx not in covered
                covered.add(idx)
                tabs = body[2 + 2 * j]
                comps.append((idx, huff[tabs >> 4], huff[0x10 | (tabs & 15)]))
                P.qt[idx] = qt[frame[idx][2]].copy()
            P.interleaved = ns == 3
            P.ri.append(ri)
            # the entropy data: up to the next marker that is neither FF00 nor RSTm
            chunks, cur, expect = [], bytearray(), 0
            while True:
                j = data.index(b"\xff", pos)
                cur += data[pos:j]
                k = j
                while data[k] == 0xFF:
                    k += 1
                nxt = data[k]
                if nxt == 0x00:
                    assert k == j + 1
                    cur.append(0xFF)
                    pos = k + 1
                elif 0xD0 <= nxt <= 0xD7:
                    assert ri and nxt == 0xD0 + expect % 8, "RST out of sequence"
                    expect += 1
                    chunks.append(bytes(cur))
                    cur = bytearray()
                    pos = k + 1
                else:
                    chunks.append(bytes(cur))
                    pos = j
                    break
            g = grid(P.W, P.H)
            if ns == 3:
                mx, my = g[1]
                where = []
                for m_ in range(mx * my):
                    y, x = divmod(m_, mx)
                    where.append([(0, (2 * y + (j >> 1)) * g[0][0] + 2 * x + (j & 1)) for j in range(4)]
                                 + [(1, m_), (2, m_)])
            else:
                idx = comps[0][0]
                cw, ch = own(P.W, P.H)[idx]
                where = [[(idx, by * g[idx][0] + bx)] for by in range(ch) for bx in range(cw)]
            total = len(where)
            step = ri if ri else total
            assert len(chunks) == -(-total // step), (len(chunks), total, ri)
            P.segments += len(chunks)
            tabs = {c[0]: (c[1], c[2]) for c in comps}
            for i, chunk in enumerate(chunks):
                br = J._Bits(chunk)
                pred = {0: 0, 1: 0, 2: 0}
                for mcu in where[i * step:(i + 1) * step]:
                    for p, b in mcu:
                        zz[p][b], pred[p] = _decode_block(br, tabs[p][0], tabs[p][1], pred[p])
        else:
            assert 0xE0 <= m <= 0xEF or m == 0xFE, f"unexpected marker {m:#x}"
    assert covered == {0, 1, 2}
    P.planes = []
    for p in range(3):
        nat = np.zeros_like(zz[p])
        nat[:, ZZ] = zz[p]
        P.planes.append(nat)
    return P


# ---- the writer -------------------------------------------------------------
def _dht_segments(tables, merged):
    parts = [bytes([tc_th]) + bytes(tables[tc_th][0]) + bytes(tables[tc_th][1]) for tc_th in (0x00, 0x10, 0x01, 0x11)]
    return [J.seg(0xFFC4, b"".join(parts))] if merged else [J.seg(0xFFC4, p) for p in parts]


def write(planes, W, H, qtables, interleaved=True, ri=0, tables=None, scan_order=(0, 1, 2), merged=False,
          fill=0, ids=(1, 2, 3), extra=(), raw=None):
    """planes: per plane [nblk, 64] in NATURAL order on the padded grid (raster
    order).  ri: one restart interval (in MCUs) or one per scan.  tables:
    {0x00, 0x10, 0x01, 0x11: (BITS, HUFFVAL)} (luma uses 0/0, chroma 1/1).
    merged: all DQT tables in one segment and all DHT tables in one.  fill:
    0xFF bytes in front of every RSTm.  extra: segments put after SOI.  raw:
    {(plane, block): [(bits, count), ...]} written instead of that block's code
    (the predictor stays as it is), for files no encoder writes.  Coefficients
    may be wider than int16 (a DC out of range)."""
    tables = dict(DEFAULT_DHT if tables is None else tables)
    ris = [ri] * 3 if isinstance(ri, int) else list(ri)
    g = grid(W, H)
    zz = [np.asarray(p, np.int64).reshape(-1, 64)[:, ZZ] for p in planes]
    raw = raw or {}
    for p in range(3):
        assert len(zz[p]) == g[p][0] * g[p][1], (p, len(zz[p]))
    out = [b"\xff\xd8"] + list(extra)
    dqt = [bytes([p]) + bytes(int(v) for v in np.asarray(qtables[p]).reshape(64)[ZZ]) for p in range(3)]
    out += [J.seg(0xFFDB, b"".join(dqt))] if merged else [J.seg(0xFFDB, d) for d in dqt]
    out.append(J.seg(0xFFC0, struct.pack(">BHHB", 8, H, W, 3)
                     + bytes([ids[0], 0x22, 0, ids[1], 0x11, 1, ids[2], 0x11, 2])))
    out += _dht_segments(tables, merged)
    code = {k: J.codes(list(b), list(v)) for k, (b, v) in tables.items()}
    last_ri = None

    def scan(comps, mcus, r):
        nonlocal last_ri
        if r != last_ri and (r or last_ri):
            out.append(J.seg(0xFFDD, struct.pack(">H", r)))
        last_ri = r
        out.append(J.seg(0xFFDA, bytes([len(comps)]) + b"".join(bytes([ids[p], 0x00 if p == 0 else 0x11])
                                                                   for p in comps) + bytes([0, 63, 0])))
        step = r if r else len(mcus)
        for m, k0 in enumerate(range(0, len(mcus), step)):
            if m:
                out.append(b"\xff" * fill + bytes([0xFF, 0xD0 + (m - 1) % 8]))
            out.append(_interval(mcus[k0:k0 + step], zz, code, raw))

    if interleaved:
        mx, my = g[1]
        mcus = []
        for m_ in range(mx * my):
            y, x = divmod(m_, mx)
            mcus.append([(0, (2 * y + (j >> 1)) * g[0][0] + 2 * x + (j & 1)) for j in range(4)] + [(1, m_), (2, m_)])
        scan((0, 1, 2), mcus, ris[0])
    else:
        for s, p in enumerate(scan_order):
            cw, ch = own(W, H)[p]
            scan((p,), [[(p, by * g[p][0] + bx)] for by in range(ch) for bx in range(cw)], ris[s])
    out.append(b"\xff\xd9")
    return b"".join(out)


def _interval(mcus, zz, code, raw):
    """One restart interval: MCUs of (plane, block) pairs -> stuffed bytes."""
    acc, n = 0, 0
    pred = [0, 0, 0]
    for mcu in mcus:
        for p, b in mcu:
            if (p, b) in raw:
                for bits, count in raw[(p, b)]:
                    acc = (acc << count) | bits
                    n += count
                continue
            dc_codes, ac_codes = (code[0x00], code[0x10]) if p == 0 else (code[0x01], code[0x11])
            blk = [int(v) for v in zz[p][b]]
            d = blk[0] - pred[p]
            pred[p] = blk[0]
            c = J.category(d)
            cd, length = dc_codes[c]
            acc = (((acc << length) | cd) << c) | ((d if d >= 0 else d - 1) & ((1 << c) - 1))
            n += length + c
            run = 0
            for v in blk[1:]:
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    cd, length = ac_codes[0xF0]
                    acc = (acc << length) | cd
                    n += length
                    run -= 16
                c = J.category(v)
                cd, length = ac_codes[(run << 4) | c]
                acc = (((acc << length) | cd) << c) | ((v if v >= 0 else v - 1) & ((1 << c) - 1))
                n += length + c
                run = 0
            if run:
                cd, length = ac_codes[0x00]
                acc = (acc << length) | cd
                n += length
    pad = -n % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((n + pad) // 8, "big").replace(b"\xff", b"\xff\x00")


# ---- what the import returns ------------------------------------------------
def stream(planes):
    """The DCT stream of natural-order planes (the oracle's Huffman encoder)."""
    from oracle import oracle as O

    global _CHUNKS
    if _CHUNKS is None:
        _CHUNKS = coefgen.Chunks(O.huff_encode_block)
    return coefgen.build_payload([np.asarray(p, np.int16).reshape(-1, 64)[:, ZZ] for p in planes], _CHUNKS)


def keep_quality(table, chroma):
    """The smallest q in 1..100 whose table is `table` (natural order), or 0."""
    from oracle import oracle as O

    t = np.asarray(table).reshape(64)
    for q in range(1, 101):
        if (np.asarray(O.qtable(q, chroma)).reshape(64) == t).all():
            return q
    return 0


def rescaled(planes, qt_file, q_dst):
    """planes requantised from the file's tables to q_dst's (requantref's arithmetic)."""
    import requantref as RQ
    from oracle import oracle as O

    out = []
    for p in range(3):
        Qd = np.asarray(O.qtable(q_dst[p], p != 0), np.float32).reshape(64)
        out.append(RQ.requant(planes[p], np.asarray(qt_file[p], np.float32)[None, :], Qd[None, :]))
    return out

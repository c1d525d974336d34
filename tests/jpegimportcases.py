"""Crafted JPEG files for the import's tests (CPU and GPU share them), built
with jpegimportref's writer from coefficient planes, so each file's content is
known without any decoder.  Never calls the code under test.

good_cases()    name -> Case: files the import must read; .planes is what it
                must find (natural order, the padded grid).
error_cases()   (name, bytes, code) for every UNSUPPORTED / SYNTAX rule.
data_cases()    name -> DataCase: files with one damaged block each (or two),
                the block the call must report and the planes it then holds.
"""
import functools
import struct

import numpy as np

import jpegimportref as JI
import jpegref as J

E_UNSUPPORTED, E_SYNTAX, E_DATA, E_TABLES = 21, 22, 23, 24
ZZ = JI.ZZ


class Case:
    def __init__(self, data, W, H, planes, qt, segments, interleaved):
        self.data, self.W, self.H, self.planes, self.qt = data, W, H, planes, qt
        self.segments, self.interleaved = segments, interleaved
        self.Wp, self.Hp = -(-W // 16) * 16, -(-H // 16) * 16


def qtables(q):
    return J.qtables_of(q)


def picture_planes(W, H, seed):
    """Sparse blocks like a picture's: a DC walk, a few low-frequency ACs."""
    rng = np.random.default_rng(seed)
    out = []
    for gw, gh in JI.grid(W, H):
        n = gw * gh
        zz = np.zeros((n, 64), np.int64)
        zz[:, 0] = np.clip(np.cumsum(rng.integers(-40, 41, n)), -1024, 1023)
        for k in range(1, 12):
            on = rng.random(n) < 0.5 / k
            zz[on, k] = rng.integers(-30, 31, int(on.sum()))
        nat = np.zeros_like(zz)
        nat[:, ZZ] = zz
        out.append(nat.astype(np.int16))
    return out


def crafted_planes(W, H, seed=3):
    """Blocks around every branch of the block decoder: ZRL chains (runs of 16,
    32, 47), coefficient 63 nonzero (no EOB), DC swings of category 11, run 15
    with size 10 (a 16-bit code), runs of +-1 / 255 that make 0xFF bytes,
    all-zero blocks."""
    rng = np.random.default_rng(seed)
    pool = []
    for run in (15, 16, 31, 32, 47, 61):
        b = np.zeros(64, np.int64)
        b[0], b[1 + run] = 5, -3
        pool.append(b)
    b = np.zeros(64, np.int64)
    b[63] = -2
    pool.append(b)
    b = np.zeros(64, np.int64)
    b[0], b[1], b[17], b[33], b[63] = 100, 1023, -1023, 600, 1
    pool.append(b)
    for dc in (-1024, 1023, -1024, 1023, 0):
        b = np.zeros(64, np.int64)
        b[0] = dc
        pool.append(b)
    b = np.zeros(64, np.int64)
    b[0] = -1
    b[1:40] = -1
    pool.append(b)
    b = np.zeros(64, np.int64)
    b[0] = 255
    b[1:30] = 255
    pool.append(b)
    pool.append(np.zeros(64, np.int64))
    pool = np.stack(pool)
    out = []
    for gw, gh in JI.grid(W, H):
        n = gw * gh
        zz = pool[np.concatenate([np.arange(len(pool)), rng.integers(0, len(pool), n)])[:n]]
        nat = np.zeros_like(zz)
        nat[:, ZZ] = zz
        out.append(nat.astype(np.int16))
    return out


def _covered(planes, W, H):
    """planes with the blocks a non-interleaved scan does not hold zeroed."""
    out = []
    for p, (gw, gh) in enumerate(JI.grid(W, H)):
        cw, ch = JI.own(W, H)[p]
        a = np.asarray(planes[p]).reshape(gh, gw, 64).copy()
        a[ch:, :, :] = 0
        a[:, cw:, :] = 0
        out.append(a.reshape(-1, 64))
    return out


def _case(W, H, planes, q=(50, 50, 50), qt=None, interleaved=True, ri=0, **kw):
    qt = qtables(q) if qt is None else qt
    if not interleaved:
        planes = _covered(planes, W, H)
    data = JI.write(planes, W, H, qt, interleaved=interleaved, ri=ri, **kw)
    ris = [ri] * 3 if isinstance(ri, int) else list(ri)
    if interleaved:
        total = [JI.grid(W, H)[1][0] * JI.grid(W, H)[1][1]]
    else:
        total = [JI.own(W, H)[p][0] * JI.own(W, H)[p][1] for p in kw.get("scan_order", (0, 1, 2))]
    segs = sum(-(-t // r) if r else 1 for t, r in zip(total, ris))
    return Case(data, W, H, planes, qt, segs, interleaved)


@functools.lru_cache(maxsize=None)
def good_cases():
    odd_qt = [np.clip(np.arange(64) * 3 + 2 + 5 * p, 1, 255) for p in range(3)]  # no quality's tables
    app = (J.seg(0xFFE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])), J.seg(0xFFFE, b"a comment"),
           J.seg(0xFFEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 1])))
    return {
        "one_mcu": _case(16, 16, crafted_planes(16, 16)),
        "48x32_ri2": _case(48, 32, crafted_planes(48, 32), q=(90, 50, 10), ri=2, extra=app),
        "144x128_ri1": _case(144, 128, crafted_planes(144, 128), ri=1, fill=3, merged=True),
        "144x128_picture": _case(144, 128, picture_planes(144, 128, 1), q=(90, 90, 90), ri=1),
        "272x16_planar_ri5": _case(272, 16, crafted_planes(272, 16), interleaved=False, ri=5),
        "272x16_planar_ri1": _case(272, 16, crafted_planes(272, 16), interleaved=False, ri=1, fill=1),
        "272x16_planar_ri123": _case(272, 16, picture_planes(272, 16, 2), interleaved=False, ri=(1, 2, 3),
                                     scan_order=(2, 0, 1), ids=(7, 0, 200)),
        "200x40_planar_ri1": _case(200, 40, crafted_planes(200, 40), interleaved=False, ri=1),
        "37x21_planar": _case(37, 21, picture_planes(37, 21, 4), interleaved=False, ri=0),
        "144x128_own_tables": _case(144, 128, picture_planes(144, 128, 5), qt=odd_qt, ri=1),
    }


# ---- files that must be refused ------------------------------------------------
def _patch(data, old, new, nth=0):
    i = -1
    for _ in range(nth + 1):
        i = data.index(old, i + 1)
    return data[:i] + new + data[i + len(old):]


def marker_offsets(data):
    """Offsets of every marker segment's start, the scans' entropy data skipped."""
    out, pos = [], 2
    while data[pos + 1] != 0xD9:
        out.append(pos)
        n = struct.unpack_from(">H", data, pos + 2)[0]
        m = data[pos + 1]
        pos += 2 + n
        if m == 0xDA:
            while not (data[pos] == 0xFF and data[pos + 1] != 0 and not 0xD0 <= data[pos + 1] <= 0xD7):
                pos += 1
    out.append(pos)
    return out


@functools.lru_cache(maxsize=None)
def error_cases():
    W, H = 48, 32
    planes, qt = picture_planes(W, H, 7), qtables((50, 50, 50))
    base = JI.write(planes, W, H, qt, ri=2)
    planar = JI.write(_covered(planes, W, H), W, H, qt, interleaved=False, ri=4)
    sof = base.index(b"\xff\xc0")
    sof_seg = base[sof:sof + 19]
    out = []
    for m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC9, 0xCF):
        out.append((f"sof{m & 15}", _patch(base, b"\xff\xc0", bytes([0xFF, m])), E_UNSUPPORTED))
    out.append(("precision_12", base[:sof + 4] + b"\x0c" + base[sof + 5:], E_UNSUPPORTED))
    for nc in (1, 4):
        out.append((f"components_{nc}", base[:sof + 9] + bytes([nc]) + base[sof + 10:], E_UNSUPPORTED))
    for name, hv in (("444", 0x11), ("422", 0x21), ("440", 0x12)):
        out.append((f"sampling_{name}", base[:sof + 11] + bytes([hv]) + base[sof + 12:], E_UNSUPPORTED))
    dqt = base.index(b"\xff\xdb")
    out.append(("tables_16bit", base[:dqt + 4] + b"\x10" + base[dqt + 5:], E_UNSUPPORTED))
    out.append(("dnl", JI.write(planes, W, H, qt, extra=(J.seg(0xFFDC, b"\0\x20"),)), E_UNSUPPORTED))
    out.append(("two_frames", JI.write(planes, W, H, qt, extra=(sof_seg,)), E_UNSUPPORTED))
    out.append(("adobe_transform_0", JI.write(planes, W, H, qt, extra=(
        J.seg(0xFFEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 0])),)), E_UNSUPPORTED))
    out.append(("height_0", base[:sof + 5] + b"\0\0" + base[sof + 7:], E_UNSUPPORTED))
    # structural damage
    out.append(("no_soi", b"\xff\xd9" + base[2:], E_SYNTAX))
    out.append(("no_sof", base[:sof] + base[sof + 19:], E_SYNTAX))
    out.append(("no_eoi", base[:-2], E_SYNTAX))
    sos = base.index(b"\xff\xda")
    out.append(("undefined_table", base[:sos + 6] + b"\x22" + base[sos + 7:], E_SYNTAX))
    out.append(("undefined_component", base[:sos + 5] + b"\x09" + base[sos + 6:], E_SYNTAX))
    out.append(("spectral_selection", base[:sos + 11] + b"\x01" + base[sos + 12:], E_SYNTAX))
    dri = base.index(b"\xff\xdd")
    out.append(("restart_count", base[:dri + 4] + b"\0\x03" + base[dri + 6:], E_SYNTAX))
    out.append(("restart_without_dri", base[:dri] + base[dri + 6:], E_SYNTAX))
    out.append(("rst_out_of_sequence", _patch(base, b"\xff\xd1", b"\xff\xd2"), E_SYNTAX))
    out.append(("covered_twice", JI.write(_covered(planes, W, H), W, H, qt, interleaved=False,
                                          scan_order=(0, 1, 1)), E_SYNTAX))
    out.append(("not_covered", JI.write(_covered(planes, W, H), W, H, qt, interleaved=False,
                                        scan_order=(0, 1)), E_SYNTAX))
    dht = base.index(b"\xff\xc4")
    out.append(("oversubscribed_bits", base[:dht + 5] + b"\x03" + base[dht + 6:], E_SYNTAX))
    out.append(("zero_table_entry", base[:dqt + 5] + b"\0" + base[dqt + 6:], E_SYNTAX))
    out.append(("segment_length_1", base[:dqt + 2] + b"\0\x01" + base[dqt + 4:], E_SYNTAX))
    # truncation at every marker boundary, inside every segment, and inside the entropy data
    for name, f in (("interleaved", base), ("planar", planar)):
        for o in marker_offsets(f):
            for cut in (o, o + 1, o + 2, o + 3, o + 5):
                if cut < len(f):
                    out.append((f"truncated_{name}_{cut}", f[:cut], E_SYNTAX))
        out.append((f"truncated_{name}_data", f[:len(f) - 9], E_SYNTAX))
    return out


# ---- damaged entropy data ---------------------------------------------------------
class DataCase:
    def __init__(self, data, W, H, bad, planes, qt):
        self.data, self.W, self.H, self.bad, self.planes, self.qt = data, W, H, bad, planes, qt
        self.Wp, self.Hp = -(-W // 16) * 16, -(-H // 16) * 16


def _mcu_blocks(W, H, m):
    g = JI.grid(W, H)
    y, x = divmod(m, g[1][0])
    return [(0, (2 * y + (j >> 1)) * g[0][0] + 2 * x + (j & 1)) for j in range(4)] + [(1, m), (2, m)]


def _global(W, H, p, b):
    g = JI.grid(W, H)
    return sum(g[i][0] * g[i][1] for i in range(p)) + b


@functools.lru_cache(maxsize=None)
def data_cases():
    """144x128, one interleaved scan, a restart per MCU: interval i is MCU i and
    lane i % 64 of wave i // 64.  Every kind of damage in the first, a middle
    and the last lane of the first wave and in the second wave; luma block j of the
    MCU is damaged, it and the MCU's later blocks are lost."""
    W, H = 144, 128
    qt = qtables((50, 50, 50))
    base = picture_planes(W, H, 11)
    luma, chroma = JI.DEFAULT_DHT, JI.DEFAULT_DHT
    # tables with symbols no baseline block may hold, at codes the pictures' blocks do not use
    def swapped(tc_th, old, new):
        t = dict(JI.DEFAULT_DHT)
        bits, vals = t[tc_th]
        t[tc_th] = (bits, tuple(new if v == old else v for v in vals))
        return t

    def sym(tables, tc_th, s):
        code, length = J.codes(list(tables[tc_th][0]), list(tables[tc_th][1]))[s]
        return (code, length)

    dc0 = sym(JI.DEFAULT_DHT, 0x00, 0)  # DC difference 0
    zrl = sym(JI.DEFAULT_DHT, 0x10, 0xF0)
    kinds = {
        # name: (tables, the damaged block's bits; None: through the planes)
        "dc_range": (None, None),
        "dc_category_12": (swapped(0x00, 11, 12), lambda t: [sym(t, 0x00, 12), (0, 12)]),
        "ac_size_11": (swapped(0x10, 0xFA, 0x0B), lambda t: [dc0, sym(t, 0x10, 0x0B), (0, 11)]),
        "ac_size_0_run_3": (swapped(0x10, 0xFA, 0x30), lambda t: [dc0, sym(t, 0x10, 0x30)]),
        "run_past_63": (None, lambda t: [dc0, zrl, zrl, zrl, sym(t, 0x10, 0xF1), (1, 1)]),
        "zrl_past_63": (None, lambda t: [dc0, zrl, zrl, zrl, zrl, sym(t, 0x10, 0x00)]),
        "no_code": (None, lambda t: [dc0, (0xFFFF, 16)]),
    }
    out = {}
    for kind, (tables, bits) in kinds.items():
        for mcus, j in (((0,), 2), ((31,), 0), ((63,), 3), ((71,), 1), ((40, 5), 3)):
            planes = [p.copy() for p in base]
            raw = {}
            t = JI.DEFAULT_DHT if tables is None else tables
            want = [p.copy() for p in base]
            for m in mcus:
                blocks = _mcu_blocks(W, H, m)
                p, b = blocks[j]
                if bits is None:
                    # out of range, on the side of the predictor (the difference keeps to category 11)
                    pred = int(base[0][blocks[j - 1][1], 0]) if 0 < j < 4 else 0
                    planes[p] = planes[p].astype(np.int64)
                    planes[p][b, 0] = 1500 if pred >= 0 else -1500
                else:
                    raw[(p, b)] = bits(t)
                for pp, bb in blocks[j:]:
                    want[pp][bb] = 0
            p, b = _mcu_blocks(W, H, min(mcus))[j]
            bad = min(_global(W, H, *_mcu_blocks(W, H, m)[j]) for m in mcus)
            data = JI.write(planes, W, H, qt, ri=1, tables=tables, raw=raw)
            out[f"{kind}_mcu{'_'.join(map(str, mcus))}"] = DataCase(data, W, H, bad, want, qt)
    # a block that needs bits beyond its interval's last byte: the MCU's last block without its EOB
    for m in (0, 63, 71):
        p, b = _mcu_blocks(W, H, m)[5]
        want = [q.copy() for q in base]
        want[p][b] = 0
        dcc = sym(JI.DEFAULT_DHT, 0x01, 0)
        data = JI.write(base, W, H, qt, ri=1, raw={(p, b): [dcc]})
        out[f"underrun_mcu{m}"] = DataCase(data, W, H, _global(W, H, p, b), want, qt)
    return out

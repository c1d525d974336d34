"""Crafted DCTYUV streams for the decoder-conformance tests, each with its
expected outcome written down by construction (never taken from a decoder).

A case is a `StreamCase`:
  name, w, h, q, payload
  kind     'accept'  a layout no encoder writes; the reference and the oracle
                     decode it, to `frame()` (coefgen.compose of its blocks)
           'defined' rejected, and the reference throws the message that
                     include/myyuv_hip.h maps to the code
           'strict'  rejected; undefined in the reference (it reads past a
                     chunk or trusts a 32-bit sum), this build's own codes
  expect   (code, bad_block) as include/myyuv_hip.h defines them for
           myyuv_gpu_dct_decompress; (0, None) for an accepted stream
  repaired the same stream with its fault(s) undone (rejected cases)
  branch   the source branch it targets, one of BRANCHES
  blocks   per plane the zig-zag blocks the (repaired) stream decodes to
  faults   [Fault]: what a decode that reads only some blocks (the region
           decode) meets; header faults have none (they fail every call)

Streams are built from a `Layout` (three planes of chunks plus the header
fields that may lie), serialised here; a Layout without lies equals
coefgen.build_payload of its blocks (asserted for every base layout).

Why no case needs, or can cause, a read outside an allocation of `cap` bytes
(csrc/k_chain.hpp, csrc/k_stream.hip, csrc/k_huff_decode.hip):
  * header families: parse_stream is given min(size word, cap) and returns
    at size <= 12; the plane-header loads are clamped to size - 8; every sum
    is 64-bit; on any failure the scan returns before it reads a size byte,
    and the decoders see desc->bad, take limit = 0 and read only byte 0..15
    of the slot (cap >= 64 in every test).
  * size-table families (hn, hc, slack, trailing): a header that passed has
    12 + ps0 + ps1 + ps2 <= size, 8 + hn + hc <= ps and hn >= blocks, so the
    size bytes [sizes_pos, sizes_pos + blocks) and the content [content_pos,
    content_pos + content_size) lie inside the stream; the scan and the
    decoders read size bytes at those positions only.
  * chunk families (sizes, nbits, tables, messages, overruns): the staging
    window ends at E = content_pos + min(scanned end, content_size) <= size;
    load4 / stage() read whole quads below `limit` = min(size word, cap) and
    zero-fill single bytes at or past it; everything else a chunk decides
    (table walk, value positions, bit positions) indexes the LDS stage, where
    parse_table keeps the walk inside 3 + tb <= s, decode_regular reads a
    value only for a matched code of a regular table (inside its group) and
    decode_general_to walks the groups inside tb.  A lane whose chunks would
    pass content_size is switched off before any of this (code 9).
  * output: every store address comes from the frame geometry and the
    block index, never from the stream.
"""
import struct

import numpy as np

import coefgen
from malformed import _irregular_chunk, _pack11

Q = (50, 50, 50)

# one entry per parser branch / accepted layout the cases target
BRANCHES = (
    "parse_stream: size <= 12",
    "parse_stream: 12+ps0+ps1+ps2 > size",
    "parse_stream: ps <= 8",
    "parse_stream: hn == 0",
    "parse_stream: hc == 0",
    "parse_stream: 8+hn+hc > ps",
    "parse_stream: hn < blocks",
    "parse_stream: 64-bit sums",
    "parse_table: s < 3",
    "parse_table: nbits > 512",
    "parse_table: 3+tb+ceil(nbits/8) > s",
    "parse_table: group overruns tb",
    "parse_table: more than 64 entries of one length",
    "decode: bits run out at code length 2..8",
    "decode: no match, >= 8 bits left (11) / fewer (10)",
    "decode: Kraft-oversubscribed table, uint8 first wraps",
    "decode_general_to: empty length / cd < first (neg)",
    "decode_group: rel+s > content_size",
    "order: lowest block of two bad chunks",
    "order: content overrun against chunk errors",
    "order: header fault against chunk fault",
    "accept: trailing bytes after plane 2",
    "accept: slack at a plane's end",
    "accept: hn > blocks",
    "accept: content_size > sum of sizes",
    "accept: chunks longer than their message, junk after the bits",
    "accept: 64 chunks of 255 B in one group",
    "accept: chunk 00 00 00",
    "accept: 64 symbols exactly / with bits left over",
    "accept: unused and duplicate table entries",
    "accept: values -1024 and 1023",
    "accept: 3+tb = 20 / 21",
    "accept: table of more than 64 entries",
    "accept: 64 entries of one length",
)


class Fault:
    """One fault as a partial decode meets it: `detect` the frame-global
    blocks whose reading reveals it, `key` the device's precedence (lowest
    wins: 2 * block + 1 for a chunk, 2 * first block of the plane for a
    content overrun), (code, bad_block) what is then reported."""

    def __init__(self, key, code, bad_block, detect):
        self.key, self.code, self.bad_block, self.detect = key, code, bad_block, frozenset(detect)


class Plane:
    def __init__(self, blocks, chunks):
        self.blocks = np.asarray(blocks, np.int16).reshape(-1, 64).copy()
        self.chunks = list(chunks)
        self.extra_sizes = b""  # size bytes after the blocks' (hn > blocks)
        self.filler = b""       # bytes after the chunks, inside content_size
        self.slack = b""        # bytes after the content, inside ps
        self.hn = self.hc = self.ps = None  # header fields that lie

    def copy(self):
        c = Plane(self.blocks, self.chunks)
        c.extra_sizes, c.filler, c.slack = self.extra_sizes, self.filler, self.slack
        c.hn, c.hc, c.ps = self.hn, self.hc, self.ps
        return c

    def body(self):
        assert all(len(c) <= 255 for c in self.chunks)
        sizes = bytes(len(c) for c in self.chunks) + self.extra_sizes
        content = b"".join(self.chunks) + self.filler
        hn = len(sizes) if self.hn is None else self.hn
        hc = len(content) if self.hc is None else self.hc
        return struct.pack("<II", hn, hc) + sizes + content + self.slack


class Layout:
    def __init__(self, w, h, planes):
        self.w, self.h, self.planes = w, h, planes
        self.trailing = b""

    def copy(self):
        c = Layout(self.w, self.h, [p.copy() for p in self.planes])
        c.trailing = self.trailing
        return c

    def payload(self):
        bodies = [p.body() for p in self.planes]
        ps = [len(b) if p.ps is None else p.ps for p, b in zip(self.planes, bodies)]
        return struct.pack("<III", *ps) + b"".join(bodies) + self.trailing

    def cum(self):
        n = [len(p.chunks) for p in self.planes]
        return (0, n[0], n[0] + n[1], n[0] + n[1] + n[2])

    def blocks(self):
        return [p.blocks for p in self.planes]

    def set(self, p, k, chunk, block=None):
        """Chunk k of plane p; `block`: the zig-zag block it decodes to."""
        self.planes[p].chunks[k] = bytes(chunk)
        if block is not None:
            self.planes[p].blocks[k] = block


class StreamCase:
    def __init__(self, name, lay, kind, expect, branch, repaired=None, faults=(), payload=None):
        self.name, self.w, self.h, self.q = name, lay.w, lay.h, Q
        self.payload = lay.payload() if payload is None else payload
        self.kind, self.expect, self.branch = kind, expect, branch
        self.repaired = repaired
        self.faults = list(faults)
        self.blocks = lay.blocks()
        self.nblk = lay.cum()[3]

    def frame(self, oracle):
        """What the (repaired) stream decodes to, from the blocks alone."""
        return coefgen.compose(self.blocks, self.w, self.h, self.q, oracle)

    def plain(self, oracle_or_chunks):
        return coefgen.build_payload(self.blocks, oracle_or_chunks)

    def region_expect(self, w, h, region, contains_block):
        """(code, bad_block) of a decode of `region`, or (0, None)."""
        if self.expect[0] and not self.faults:
            return self.expect  # a header fault fails every call
        seen = [f for f in self.faults if any(contains_block(w, h, region, g) for g in f.detect)]
        if not seen:
            return (0, None)
        f = min(seen, key=lambda f: f.key)
        return (f.code, f.bad_block)


# ---- base layouts -----------------------------------------------------------
def _base_blocks(w, h, seed):
    """Small seeded blocks (messages of 0..6 symbols, values in -30..30):
    chunks of 7..20 B, so a 64-block group stages in one round."""
    rng = np.random.default_rng(seed)
    out = []
    for n in coefgen.plane_counts(w, h):
        b = np.zeros((n, 64), np.int16)
        for k in range(n):
            msz = int(rng.integers(0, 7))
            if msz:
                v = rng.integers(-30, 31, msz)
                v[-1] = v[-1] if v[-1] else 7
                b[k, :msz] = v
        out.append(b)
    return out


def base_layout(w, h, chunks, seed=11):
    blocks = _base_blocks(w, h, seed + w)
    lay = Layout(w, h, [Plane(b, [chunks.one(z) for z in b]) for b in blocks])
    assert lay.payload() == coefgen.build_payload(blocks, chunks)
    return lay


def _zz(seq):
    b = np.zeros(64, np.int16)
    b[:len(seq)] = seq
    return b


def _chunk(groups, seq, nbits_extra=0):
    """malformed._irregular_chunk at its exact size; nbits_extra more bits
    declared (and present) after the message."""
    ch = bytearray(_irregular_chunk(groups, seq, 4096))
    nbits, tb = ch[0] | (ch[1] << 8), ch[2]
    nb2 = nbits + nbits_extra
    ch[0], ch[1] = nb2 & 0xFF, nb2 >> 8
    return bytes(ch[:3 + tb + (nb2 + 7) // 8])


def _chunk_picks(groups, picks):
    """(chunk, values): the message is given as (length, rank among the
    table's entries of that length, in append order), so a duplicate value's
    second code can be sent; codes by the decoder's rule, first_L + rank."""
    by_len = {}
    for L, vals in groups:
        by_len.setdefault(L, []).extend(vals)
    first, f = {}, 0
    for L in range(1, 9):
        first[L] = f
        f = (f + len(by_len.get(L, []))) << 1
    bits, vals = [], []
    for L, r in picks:
        code = first[L] + r
        assert code < (1 << L)
        bits += [(code >> b) & 1 for b in range(L - 1, -1, -1)]
        vals.append(by_len[L][r])
    table = b"".join(_group(L, v) for L, v in groups)
    return _raw_chunk(len(bits), table, _bits(bits)), vals


def _raw_chunk(nbits, table, data):
    return bytes([nbits & 0xFF, nbits >> 8, len(table)]) + bytes(table) + bytes(data)


def _group(L, vals):
    return bytes([((L - 1) << 5) | (len(vals) - 1)]) + _pack11(vals)


def _bits(bitlist):
    acc = 0
    for i, b in enumerate(bitlist):
        acc |= (b & 1) << i
    return acc.to_bytes((len(bitlist) + 7) // 8, "little")


# a table with one code of every length 1..8: "0", "10", ..., "11111110"
_LADDER = b"".join(_group(L, [L]) for L in range(1, 9))


def bad_chunks():
    """name -> (chunk, code, kind, branch): single chunks that must be
    rejected, each built so that exactly the named check fails."""
    out = {}
    valid = _chunk([(1, [3]), (2, [-2, 9])], [3, -2, 9, 3])
    for n in (0, 1, 2):
        out[f"size{n}"] = (valid[:n], 12, "strict", "parse_table: s < 3")
    # nbits 513 with every byte it asks for present: only nbits > 512 fails
    out["nbits513"] = (_raw_chunk(513, _group(1, [5]), bytes(65)), 12, "strict", "parse_table: nbits > 512")
    out["nbits65535"] = (_raw_chunk(0xFFFF, _group(1, [5]), bytes(200)), 12, "strict", "parse_table: nbits > 512")
    assert 3 + valid[2] + ((valid[0] | valid[1] << 8) + 7) // 8 == len(valid)
    out["short_by_one"] = (valid[:-1], 12, "strict", "parse_table: 3+tb+ceil(nbits/8) > s")
    # a group of 2 values needs 1 + 3 table bytes; tb says 3 (the byte is there)
    out["group_overrun"] = (_raw_chunk(8, _group(1, [5, 6])[:3], _group(1, [5, 6])[3:] + b"\x00"), 12, "strict",
                            "parse_table: group overruns tb")
    assert out["group_overrun"][0][2] == 3
    v65 = list(range(1, 66))
    out["len7_x65"] = (_raw_chunk(7, _group(7, v65[:32]) + _group(7, v65[32:64]) + _group(7, v65[64:]), b"\x00"),
                       12, "strict", "parse_table: more than 64 entries of one length")
    for L in range(2, 9):  # one symbol "0", then L - 1 ones: the length-L code needs one more bit
        out[f"bits_out_len{L}"] = (_raw_chunk(L, _LADDER, _bits([0] + [1] * (L - 1))), 10, "defined",
                                   "decode: bits run out at code length 2..8")
    for r in (1, 7):  # only a length-8 code, r bits
        out[f"bits_out_only8_r{r}"] = (_raw_chunk(r, _group(8, [4]), b"\x00"), 10, "defined",
                                       "decode: bits run out at code length 2..8")
    nm = _group(2, [5])  # code "00" only; the bits are all ones
    out["nomatch_8left"] = (_raw_chunk(8, nm, b"\xff"), 11, "defined",
                            "decode: no match, >= 8 bits left (11) / fewer (10)")
    out["nomatch_7left"] = (_raw_chunk(7, nm, b"\xff"), 10, "defined",
                            "decode: no match, >= 8 bits left (11) / fewer (10)")
    out["nomatch_after_symbol"] = (_raw_chunk(10, nm, b"\xfc\x03"), 11, "defined",
                                   "decode: no match, >= 8 bits left (11) / fewer (10)")
    out["nomatch_after_symbol_7left"] = (_raw_chunk(9, nm, b"\xfc\x01"), 10, "defined",
                                         "decode: no match, >= 8 bits left (11) / fewer (10)")
    return out


def odd_chunks():
    """name -> (chunk, zig-zag block, branch): single chunks no encoder
    writes that must decode, to the block written next to them."""
    out = {}
    out["zero3"] = (b"\x00\x00\x00", _zz([]), "accept: chunk 00 00 00")
    # length 3 = [-7, 11 | 11, 300] (two groups): 11 twice, both codes sent; 300 never
    ch, vals = _chunk_picks([(3, [-7, 11]), (1, [0]), (3, [11, 300])], [(1, 0), (3, 0), (3, 1), (3, 2), (1, 0), (3, 2)])
    assert vals == [0, -7, 11, 11, 0, 11]
    out["unused_duplicate"] = (ch, _zz(vals), "accept: unused and duplicate table entries")
    out["extremes"] = (_chunk([(1, [-1024]), (2, [1023])], [-1024, 1023] * 20), _zz([-1024, 1023] * 20),
                       "accept: values -1024 and 1023")
    t17 = [(2, [1]), (3, [2]), (4, [3]), (5, [4, 5, 6, 7, 8])]
    t18 = [(2, [1]), (3, [2]), (4, [3, 4, 5]), (5, [6, 7, 8])]
    for name, t, n in (("tb17", t17, 17), ("tb18", t18, 18)):
        seq = [v for _, vs in t for v in vs] * 2
        ch = _chunk(t, seq)
        assert ch[2] == n
        out[name] = (ch, _zz(seq), "accept: 3+tb = 20 / 21")
    s64 = ([2, -3, 2, 2, 5, -3, 2, 9] * 8)[:64]
    t64 = [(3, [9, 5]), (1, [2]), (2, [-3])]  # (groups and values not in the encoder's order)
    out["sym64"] = (_chunk(t64, s64), _zz(s64), "accept: 64 symbols exactly / with bits left over")
    out["sym64_bits_left"] = (_chunk(t64, s64, nbits_extra=13), _zz(s64),
                              "accept: 64 symbols exactly / with bits left over")
    # oversubscribed at length 7 (126 + 4 > 128): the uint8 `first` of length 8
    # wraps to 4; its three length-8 entries and two of length 7 are unreachable
    gk = [(1, [1]), (2, [2]), (3, [3]), (4, [4]), (5, [5]), (6, [6]), (7, [7, 8, 9, 10]), (8, [11, 12, 13])]
    sk = [1, 2, 3, 4, 5, 6, 7, 8, 1, 8]
    out["kraft_wrap"] = (_chunk(gk, sk), _zz(sk), "decode: Kraft-oversubscribed table, uint8 first wraps")
    # lengths 2 and 4 empty: the codes taken sit right at `first` of lengths 3
    # and 5.  (cd < first cannot arise: a code that fails length L has cd >=
    # first + count there, so 2 cd + b >= the next first; the uint8 wrap needs
    # cd >= 128, which only length 8 has.  The branch is unreachable in the
    # oracle and in decode_general_to alike; this is the nearest stream.)
    gn = [(1, [1]), (3, [2, 3]), (5, [4, 5, 6])]
    sn = [2, 4, 1, 3, 6, 5, 2]
    out["empty_lengths"] = (_chunk(gn, sn), _zz(sn), "decode_general_to: empty length / cd < first (neg)")
    # more than 64 entries in all, never more than 64 of one length
    v80 = [v for v in range(-40, 41) if v]
    g80 = [(7, v80[:32]), (7, v80[32:40]), (8, v80[40:72]), (8, v80[72:])]
    ch80 = _chunk(g80, v80[:64])
    assert ch80[2] == 114 and (ch80[0] | ch80[1] << 8) == 472
    out["table80_split"] = (ch80, _zz(v80[:64]), "accept: table of more than 64 entries")
    v66 = [v for v in range(-33, 34) if v]
    g66 = [(6, v66[:22]), (7, v66[22:44]), (8, v66[44:])]  # one group per length: a "regular" table
    s66 = v66[:22] + v66[22:44] + v66[44:64]
    out["table66_regular"] = (_chunk(g66, s66), _zz(s66), "accept: table of more than 64 entries")
    v64 = list(range(100, 164))
    out["len7_x64"] = (_chunk([(7, v64[:32]), (7, v64[32:])], v64), _zz(v64), "accept: 64 entries of one length")
    return out


def _junk(n, seed):
    return bytes(np.random.default_rng(seed).integers(1, 256, n, dtype=np.uint8))


def _pad(chunk, size, seed):
    """`chunk` made `size` bytes long with non-zero junk after its bits."""
    assert len(chunk) >= 3 and len(chunk) <= size <= 255
    return chunk + _junk(size - len(chunk), seed)


# (plane, block in plane): lane 0, lane 63, mid-group, first and last group of
# every plane of the 208x96 frame (312 + 78 + 78 blocks: no block row divides
# a 64-block group)
POSITIONS_208 = ((0, 0), (0, 63), (0, 100), (0, 311), (1, 0), (1, 63), (1, 77), (2, 64), (2, 30))


def _overrun_detect(lay, p, hc):
    """Blocks of plane p whose chunk ends past hc."""
    acc, out = 0, []
    for k, c in enumerate(lay.planes[p].chunks):
        acc += len(c)
        if acc > hc:
            out.append(lay.cum()[p] + k)
    return out


def _chunk_fault(lay, p, k, code):
    g = lay.cum()[p] + k
    return Fault(2 * g + 1, code, g, [g])


def _overrun_fault(lay, p, hc):
    first = lay.cum()[p]
    return Fault(2 * first, 9, first if first else -1, _overrun_detect(lay, p, hc))


def build(oracle):
    """Every case, in a fixed order."""
    chunks = coefgen.Chunks(oracle.huff_encode_block)
    cases = []
    bad, odd = bad_chunks(), odd_chunks()
    small = base_layout(16, 16, chunks)
    mid = base_layout(208, 96, chunks)

    def reject(name, lay, kind, expect, branch, good, faults=(), payload=None):
        cases.append(StreamCase(name, lay, kind, expect, branch, repaired=good.payload(), faults=faults,
                                payload=payload))
        cases[-1].blocks = good.blocks()

    def accept(name, lay, branch):
        cases.append(StreamCase(name, lay, "accept", (0, None), branch))

    # ---- header faults (bad_block -1 on every single-frame call) ------------
    for tag, base in (("16", small), ("208", mid)):
        pay = base.payload()
        reject(f"hdr_size12_{tag}", base, "defined", (6, -1), "parse_stream: size <= 12", base, payload=pay[:12])
        reject(f"hdr_cut1_{tag}", base, "defined", (6, -1), "parse_stream: 12+ps0+ps1+ps2 > size", base,
               payload=pay[:-1])
    for p in range(3):
        for i, (tag, field, val, code, kind, branch) in enumerate((
                ("ps_is_8", "ps", 8, 7, "defined", "parse_stream: ps <= 8"),
                ("hn_is_0", "hn", 0, 8, "defined", "parse_stream: hn == 0"),
                ("hc_is_0", "hc", 0, 9, "defined", "parse_stream: hc == 0"),
                ("ps_minus_1", "ps", "minus1", 7, "defined", "parse_stream: 8+hn+hc > ps"),
                ("hn_short_by_1", "hn", "short", 8, "strict", "parse_stream: hn < blocks"),
                ("ps_ffffffff", "ps", 0xFFFFFFFF, 6, "strict", "parse_stream: 64-bit sums"),
                ("hn_ffffffff", "hn", 0xFFFFFFFF, 7, "strict", "parse_stream: 64-bit sums"),
                ("hc_ffffffff", "hc", 0xFFFFFFFF, 7, "strict", "parse_stream: 64-bit sums"))):
            base, gtag = (small, "16") if (p + i) % 2 else (mid, "208")
            if val == "short" and p:  # (16x16's chroma planes have one block: short by one is hn == 0)
                base, gtag = mid, "208"
            lay = base.copy()
            pl = lay.planes[p]
            if val == "minus1":
                val = len(pl.body()) - 1
            elif val == "short":
                val = len(pl.chunks) - 1
            setattr(pl, field, val)
            reject(f"hdr_{tag}_p{p}_{gtag}", lay, kind, (code, -1), branch, base)

    # ---- chunk faults, each kind at a position of the 208x96 frame ----------
    names = sorted(bad)
    for i, name in enumerate(names):
        ch, code, kind, branch = bad[name]
        p, k = POSITIONS_208[i % len(POSITIONS_208)]
        lay = mid.copy()
        lay.set(p, k, ch)
        reject(f"chunk_{name}_p{p}k{k}", lay, kind, (code, mid.cum()[p] + k), branch, mid,
               faults=[_chunk_fault(mid, p, k, code)])
    # the two plainest faults at every position, and in every plane of 16x16
    for name in ("bits_out_len3", "size2"):
        ch, code, kind, branch = bad[name]
        spots = [(mid, "208", p, k) for p, k in POSITIONS_208] + [(small, "16", 0, 3), (small, "16", 1, 0),
                                                                  (small, "16", 2, 0), (small, "16", 0, 0)]
        for base, tag, p, k in spots:
            cname = f"chunk_{name}_p{p}k{k}" + ("_16" if tag == "16" else "")
            if any(c.name == cname for c in cases):
                continue
            lay = base.copy()
            lay.set(p, k, ch)
            reject(cname, lay, kind, (code, base.cum()[p] + k), branch, base,
                   faults=[_chunk_fault(base, p, k, code)])

    # ---- a group that stages in two rounds (64 chunks of 100 B > 5,104 B) ---
    two = mid.copy()
    for k in range(64, 128):
        two.set(0, k, _pad(two.planes[0].chunks[k], 100, 1000 + k))
    accept("two_rounds_208", two, "accept: chunks longer than their message, junk after the bits")
    for k, name in ((66, "bits_out_len8"), (126, "nbits513"), (127, "nomatch_8left")):
        ch, code, kind, branch = bad[name]
        lay = two.copy()
        lay.set(0, k, ch)
        reject(f"two_rounds_{name}_k{k}", lay, kind, (code, k), branch, two, faults=[_chunk_fault(two, 0, k, code)])

    # ---- content overruns: the plane's sizes sum to content_size + 1 at the
    # crossing chunk (first, middle, last of the plane) ----------------------
    for base, tag in ((mid, "208"), (small, "16")):
        for p in range(3):
            n = len(base.planes[p].chunks)
            for where, k in (("first", 0), ("mid", n // 2 + 1), ("last", n - 1)):
                if tag == "16" and (where == "mid" or (p and where == "first")):
                    continue
                lay = base.copy()
                hc = sum(len(c) for c in lay.planes[p].chunks[:k + 1]) - 1
                lay.planes[p].hc = hc
                f = _overrun_fault(base, p, hc)
                assert min(f.detect) == base.cum()[p] + k
                reject(f"overrun_p{p}_{where}_{tag}", lay, "strict", (9, f.bad_block),
                       "decode_group: rel+s > content_size", base, faults=[f])

    # ---- two faults ----------------------------------------------------------
    def two_chunk(name, spots, branch):
        lay = mid.copy()
        fs = []
        for p, k, bname in spots:
            lay.set(p, k, bad[bname][0])
            fs.append(_chunk_fault(mid, p, k, bad[bname][1]))
        f = min(fs, key=lambda f: f.key)
        reject(name, lay, "strict", (f.code, f.bad_block), branch, mid, faults=fs)

    two_chunk("two_groups_p0", [(0, 200, "size1"), (0, 70, "bits_out_len2")], "order: lowest block of two bad chunks")
    two_chunk("two_planes_p2_p1", [(2, 5, "nomatch_8left"), (1, 70, "group_overrun")],
              "order: lowest block of two bad chunks")
    two_chunk("two_same_group", [(0, 190, "nomatch_7left"), (0, 130, "nbits65535")],
              "order: lowest block of two bad chunks")
    for name, p_over, spots in (("overrun_p1_between_bad", 1, [(1, 3, "size0"), (1, 70, "bits_out_len4")]),
                                ("overrun_p0_between_bad", 0, [(0, 10, "nomatch_8left"), (0, 300, "size2")]),
                                ("overrun_p1_after_bad_p0", 1, [(0, 250, "bits_out_len5")]),
                                ("overrun_p1_before_bad_p2", 1, [(2, 1, "short_by_one")])):
        lay = mid.copy()
        fs = []
        for p, k, bname in spots:
            lay.set(p, k, bad[bname][0])
            fs.append(_chunk_fault(mid, p, k, bad[bname][1]))
        n = len(lay.planes[p_over].chunks)
        hc = sum(len(c) for c in lay.planes[p_over].chunks[:n // 2]) - 1
        lay.planes[p_over].hc = hc
        fo = _overrun_fault(lay, p_over, hc)
        fs.append(fo)
        f = min(fs, key=lambda f: f.key)
        reject(name, lay, "strict", (f.code, f.bad_block), "order: content overrun against chunk errors", mid,
               faults=fs)
    # the precedence case: a bad chunk in plane 0, a short hn in plane 2.
    # Every header check comes before any chunk: 8, not 10.
    # (16x16 cannot hold it: a chroma plane of one block short by one is hn == 0)
    for p_hn, k in ((2, 5), (1, 63)):
        lay = mid.copy()
        lay.set(0, k, bad["bits_out_len3"][0])
        lay.planes[p_hn].hn = len(lay.planes[p_hn].chunks) - 1
        reject(f"precedence_hn{p_hn}_chunk0_208", lay, "strict", (8, -1), "order: header fault against chunk fault",
               mid)

    # ---- accepted layouts ----------------------------------------------------
    for base, tag in ((small, "16"), (mid, "208")):
        lay = base.copy()
        lay.trailing = _junk(37, 1)
        accept(f"trailing_{tag}", lay, "accept: trailing bytes after plane 2")
        lay = base.copy()
        for p in range(3):
            lay.planes[p].slack = _junk(5 + 11 * p, 2 + p)
        accept(f"slack_{tag}", lay, "accept: slack at a plane's end")
        lay = base.copy()
        for p in range(3):
            lay.planes[p].extra_sizes = _junk(1 + 16 * p, 5 + p)
        accept(f"hn_larger_{tag}", lay, "accept: hn > blocks")
        lay = base.copy()
        for p in range(3):
            lay.planes[p].filler = _junk(3 + 40 * p, 8 + p)
        accept(f"hc_larger_{tag}", lay, "accept: content_size > sum of sizes")
        lay = base.copy()
        for p in range(3):
            n = len(lay.planes[p].chunks)
            for k in {0, n // 2, n - 1}:
                lay.set(p, k, _pad(lay.planes[p].chunks[k], 255 if k == 0 else 64 + k % 100, 20 + k))
        accept(f"padded_{tag}", lay, "accept: chunks longer than their message, junk after the bits")
    # the odd chunks: each at a position of 208x96, all of them in 16x16's planes
    for i, name in enumerate(sorted(odd)):
        ch, blk, branch = odd[name]
        p, k = POSITIONS_208[(i + 3) % len(POSITIONS_208)]
        lay = mid.copy()
        lay.set(p, k, ch, blk)
        accept(f"odd_{name}_p{p}k{k}", lay, branch)
        lay = small.copy()
        p, k = ((0, i % 4), (1, 0), (2, 0))[i % 3]
        lay.set(p, k, ch, blk)
        accept(f"odd_{name}_16", lay, branch)
    # a 16x16 frame made of odd chunks only, one per block
    lay = small.copy()
    for (p, k), name in zip(((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0)),
                            ("table80_split", "table66_regular", "len7_x64", "kraft_wrap", "zero3", "extremes")):
        lay.set(p, k, odd[name][0], odd[name][1])
    accept("odd_all_16", lay, "accept: table of more than 64 entries")

    # ---- 256x192: 64 chunks of 255 B in one group (four staging rounds) -----
    big = base_layout(256, 192, chunks)
    lay = big.copy()
    for p, lo in ((0, 192), (1, 64)):
        for k in range(lo, lo + 64):
            lay.set(p, k, _pad(lay.planes[p].chunks[k], 255, 3000 + 7 * k + p))
    accept("group_255x64_256", lay, "accept: 64 chunks of 255 B in one group")
    full = lay
    lay = full.copy()
    ch, code, kind, branch = bad["bits_out_len7"]
    lay.set(0, 255, ch)
    reject("group_255x64_bad_lane63", lay, kind, (code, 255), branch, full, faults=[_chunk_fault(full, 0, 255, code)])

    names = [c.name for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


_CASES = None


def cases(oracle):
    """The case list, built once and shared (not to be modified)."""
    global _CASES
    if _CASES is None:
        _CASES = build(oracle)
    return _CASES


def names():
    """The case names without building the streams twice: for parametrising."""
    from oracle import oracle as O

    return [c.name for c in cases(O)]

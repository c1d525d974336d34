"""Coefficient-domain inputs: blocks built to K2's own boundaries, block lists
placed at the overflow passes' regime switches, and DCTYUV streams assembled
from the oracle's chunks that no pixel frame produces.

Everything is seeded and deterministic.  Blocks are int16[64] in ZIG-ZAG order
(what Codec.huff_encode_blocks takes); oracle.huff_encode_block and
oracle.idct_block take NATURAL order (`natural`).

Terms (codec_common.hpp class_of, k_huff_encode.hip sort_key):
  msz       1 + zig-zag index of the last nonzero coefficient (0: all zero);
  nnz       nonzero coefficients;
  nub       nnz + (1 if a zero lies inside the message), the symbol-slot
            estimate K2 classifies by: single (msz <= 1), r4 (nub <= 4), r8
            (<= 8), r8x (< ovf_nub), ovf;
  distinct  distinct values of the message, which is what the CAP-8 and CAP-16
            builds can or cannot hold: a block is LISTED for the overflow
            passes when its class is ovf, or r8x with distinct > 8, and the
            CAP-16 tier lists it AGAIN when distinct > 16.
"""
import struct

import numpy as np

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
               41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15,
               23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
OVF_NUB = 16           # codec_common.hpp kOvfNub (myyuv_hip.k2_constants()["ovf_nub"])
MSZ_EDGES = (6, 12, 20)  # sort_key's length buckets: <= 6, <= 12, <= 20, longer
MAX_CHUNK = 160


def natural(zz_blocks):
    """Zig-zag ordered blocks [..., 64] -> natural (row-major) order."""
    zz_blocks = np.asarray(zz_blocks, np.int16)
    out = np.zeros_like(zz_blocks)
    out[..., ZZ] = zz_blocks
    return out


# ---- single blocks ---------------------------------------------------------
def block(nub, distinct, msz, zero_inside, rng):
    """A zig-zag block with message length `msz`, nnz + (msz > nnz) == `nub`
    and exactly `distinct` distinct values in the message (a zero inside the
    message counts as one); ValueError when no such block exists.  The
    all-zero block is block(0, 0, 0, False, rng)."""
    nub, distinct, msz = int(nub), int(distinct), int(msz)
    if not (0 <= msz <= 64 and 0 <= nub <= 64):
        raise ValueError("msz and nub lie in 0..64")
    out = np.zeros(64, np.int16)
    if msz == 0:
        if nub or distinct or zero_inside:
            raise ValueError("the all-zero block has nub = distinct = 0 and no zero inside a message")
        return out
    zi = 1 if zero_inside else 0
    nnz = nub - zi
    if nnz < 1:
        raise ValueError("a message ends in a nonzero coefficient: nnz >= 1")
    if zero_inside and msz <= nnz:
        raise ValueError(f"a zero inside the message needs msz > nnz = {nnz}")
    if not zero_inside and msz != nnz:
        raise ValueError(f"without a zero inside, msz = nnz = nub = {nub}")
    if not 1 <= distinct - zi <= nnz:
        raise ValueError(f"distinct - {zi} must lie in 1..{nnz}")
    cand = np.concatenate([np.arange(-1024, 0), np.arange(1, 1024)])
    vals = rng.choice(cand, distinct - zi, replace=False)
    body = np.concatenate([vals, rng.choice(vals, nnz - len(vals))])
    rng.shuffle(body)
    pos = np.concatenate([np.sort(rng.choice(msz - 1, nnz - 1, replace=False)), [msz - 1]]).astype(int)
    out[pos] = body
    return out


def describe(b):
    """(nub, distinct, msz) of a zig-zag block, by definition."""
    b = np.asarray(b)
    nz = np.nonzero(b)[0]
    msz = int(nz[-1]) + 1 if len(nz) else 0
    nnz = len(nz)
    return nnz + (1 if msz > nnz else 0), len(set(b[:msz].tolist())), msz


def klass(b, ovf_nub=OVF_NUB):
    nub, _, msz = describe(b)
    if msz <= 1:
        return "single"
    return "r4" if nub <= 4 else "r8" if nub <= 8 else "r8x" if nub < ovf_nub else "ovf"


def listed(b, ovf_nub=OVF_NUB):
    """K2 puts the block on the overflow worklist."""
    c = klass(b, ovf_nub)
    return c == "ovf" or (c == "r8x" and describe(b)[1] > 8)


def listed_again(b, ovf_nub=OVF_NUB):
    """... and the CAP-16 tier lists it again."""
    return listed(b, ovf_nub) and describe(b)[1] > 16


# ---- expected chunks -------------------------------------------------------
class Chunks:
    """The oracle's chunk per distinct block, computed once and shared."""

    def __init__(self, encode_natural):
        self.encode = encode_natural
        self.memo = {}

    def one(self, zz_block):
        b = np.ascontiguousarray(zz_block, np.int16)
        key = b.tobytes()
        ch = self.memo.get(key)
        if ch is None:
            ch = self.memo[key] = bytes(self.encode(natural(b)))
        return ch

    def padded(self, zz_blocks):
        """(uint8[n, 160] zero-padded chunks, uint8[n] sizes)."""
        zz_blocks = np.asarray(zz_blocks, np.int16).reshape(-1, 64)
        out = np.zeros((len(zz_blocks), MAX_CHUNK), np.uint8)
        sizes = np.zeros(len(zz_blocks), np.uint8)
        for i, b in enumerate(zz_blocks):
            ch = self.one(b)
            out[i, :len(ch)] = np.frombuffer(ch, np.uint8)
            sizes[i] = len(ch)
        return out, sizes


class Case:
    """A block list as a pool of distinct blocks and an index per position,
    so large lists cost one oracle call per pool entry."""

    def __init__(self, pool, idx=None):
        self.pool = np.asarray(pool, np.int16).reshape(-1, 64)
        self.idx = np.arange(len(self.pool)) if idx is None else np.asarray(idx, np.int64)

    @property
    def blocks(self):
        return self.pool[self.idx]

    def expected(self, chunks):
        c, s = chunks.padded(self.pool)
        return c[self.idx], s[self.idx]

    def listed_mask(self, ovf_nub=OVF_NUB):
        return np.array([listed(b, ovf_nub) for b in self.pool])[self.idx]

    def counts(self, ovf_nub=OVF_NUB):
        """(blocks K2 lists, blocks the CAP-16 tier lists again), by design."""
        a = np.array([listed(b, ovf_nub) for b in self.pool])
        b = np.array([listed_again(b, ovf_nub) for b in self.pool])
        return int(a[self.idx].sum()), int(b[self.idx].sum())


# ---- section 3: K2's classes, buckets, windows and shapes -------------------
NUBS = (1, 2, 4, 5, 8, 9, 15, 16, 17, 40, 64)
MSZS = (1, 2, 6, 7, 12, 13, 20, 21, 63, 64)
DISTINCTS = (1, 2, 3, 4, 5, 7, 8, 9, 10, 15, 16, 17, 33, 64)


def class_bucket_blocks(seed=101, reps=2):
    """Every feasible (nub, distinct, msz, zero inside) with nub in NUBS (or
    nub = msz, which a message without a zero needs), msz in MSZS and distinct
    in DISTINCTS or at its own ends; `reps` draws each, and the all-zero block.
    Returns [(name, block)]."""
    rng = np.random.default_rng(seed)
    out = [("all_zero", block(0, 0, 0, False, rng))]
    for msz in MSZS:
        for zi in (False, True):
            for nub in sorted(set(NUBS) | {msz}):
                lo, hi = (2, nub) if zi else (1, nub)
                for d in sorted(set(DISTINCTS) | {lo, hi, hi - 1}):
                    for r in range(reps):
                        try:
                            b = block(nub, d, msz, zi, rng)
                        except ValueError:
                            break
                        assert describe(b) == (nub, d, msz)
                        out.append((f"nub{nub}_d{d}_msz{msz}_{'z' if zi else 'n'}_{r}", b))
    return out


def dc_blocks():
    """msz = 1 for every DC in -1024..1023 (DC 0: the all-zero block)."""
    b = np.zeros((2048, 64), np.int16)
    b[:, 0] = np.arange(-1024, 1024)
    return b


def _bucket_msz(bucket):
    lo = (1,) + tuple(e + 1 for e in MSZ_EDGES)
    hi = MSZ_EDGES + (64,)
    return lo[bucket], hi[bucket]


def key_pool(cls, bucket, rng, n=24):
    """n blocks of one K2 sort key: class `cls` (single, r4, r8, r8x:
    with message lengths of length bucket 0..3; ovf: any length).  r8x pools
    mix blocks the CAP-8 build holds (distinct <= 8) with ones it declines."""
    out = []
    while len(out) < n:
        if cls == "single":
            b = np.zeros(64, np.int16)
            b[0] = rng.integers(-1024, 1024)
            out.append(b)
            continue
        nub_lo, nub_hi = {"r4": (2, 4), "r8": (5, 8), "r8x": (9, OVF_NUB - 1), "ovf": (OVF_NUB, 64)}[cls]
        mlo, mhi = (2, 64) if cls == "ovf" else _bucket_msz(bucket)
        msz = int(rng.integers(max(mlo, 2), mhi + 1))
        zi = bool(rng.integers(0, 2))
        nub = int(rng.integers(nub_lo, nub_hi + 1))
        if not zi:
            nub = msz
        if not (nub_lo <= nub <= nub_hi and nub <= msz):
            continue
        dmax = nub
        d = int(rng.integers(2 if zi else 1, dmax + 1))
        if cls == "r8x" and len(out) % 2 == 0:
            d = min(d, 8)
        try:
            b = block(nub, d, msz, zi, rng)
        except ValueError:
            continue
        assert klass(b) == cls
        out.append(b)
    return np.stack(out)


def sort_keys():
    """(name, class, bucket) of K2's sort keys that hold live blocks."""
    keys = [("single", "single", 0)]
    for cls in ("r4", "r8", "r8x"):
        for bkt in range(len(MSZ_EDGES) + 1):
            lo, hi = _bucket_msz(bkt)
            if cls == "r8x" and hi < 9:
                continue  # nub >= 9 needs msz >= 9: the r8x class has no block this short
            keys.append((f"{cls}_b{bkt}", cls, bkt))
    keys.append(("ovf", "ovf", 0))
    return keys


def window_cases(window, seed=202):
    """[(name, Case)] of one K2 window (`window` blocks) each."""
    rng = np.random.default_rng(seed)
    zero = np.zeros((1, 64), np.int16)
    out = []
    pools = {}
    for name, cls, bkt in sort_keys():
        pool = pools[name] = key_pool(cls, bkt, rng)
        # the whole window of one key
        out.append((f"whole_{name}", Case(pool, rng.integers(0, len(pool), window))))
        # 63 / 64 / 65 of the key anywhere in an all-zero window: the sorted
        # order ends in a run that does or does not straddle the two keys
        for n in (63, 64, 65):
            idx = np.zeros(window, np.int64)
            at = rng.choice(window, n, replace=False)
            idx[at] = 1 + rng.integers(0, len(pool), n)
            out.append((f"{n}_of_{name}", Case(np.concatenate([zero, pool]), idx)))
    # the five classes interleaved by position: the sort's stable order
    five = [pools["single"], pools["r4_b1"], pools["r8_b2"], pools["r8x_b3"], pools["ovf"]]
    pool = np.concatenate(five)
    n = window + 5 * 13  # (and a partial second window)
    idx = np.array([(i % 5) * len(five[0]) + rng.integers(0, len(five[0])) for i in range(n)])
    out.append(("interleaved_i_mod_5", Case(pool, idx)))
    # 63 single-class blocks and one r8x block of msz 64: the run's longest
    # message drives the short ones through the long loop
    for d, tag in ((8, "builds"), (9, "declined")):
        long_blk = block(OVF_NUB - 1, d, 64, True, rng)
        pool = np.concatenate([pools["single"], long_blk[None]])
        for at in (0, 31, 63):
            idx = rng.integers(0, len(pools["single"]), 64)
            idx[at] = len(pool) - 1
            out.append((f"63_single_one_r8x_msz64_{tag}_at{at}", Case(pool, idx)))
    return out


def mixed_pool(seed=303, per_key=12):
    """Blocks of every sort key."""
    rng = np.random.default_rng(seed)
    return np.concatenate([key_pool(cls, bkt, rng, per_key) for _, cls, bkt in sort_keys()])


def shape_cases(group, seed=404):
    """[(name, Case)]: block counts around the run, the tile (`group` blocks)
    and the window: partial tiles, and 1, 2 or 3 tiles in the last window."""
    rng = np.random.default_rng(seed)
    pool = mixed_pool()
    ns = (1, 63, 64, 65, group - 1, group, group + 1, 4 * group - 1, 4 * group, 4 * group + 1, 5 * group + 1,
          6 * group + 7, 7 * group)
    return [(f"n{n}", Case(pool, rng.integers(0, len(pool), n))) for n in ns]


# ---- section 4: list lengths at the regime switches -------------------------
def gate_pools(seed=505, n=64):
    """(unlisted, listed with at most 16 distinct symbols, listed with more)."""
    rng = np.random.default_rng(seed)
    free = np.concatenate([key_pool(cls, bkt, rng, 8) for _, cls, bkt in sort_keys() if cls in ("single", "r4", "r8")])
    low, high = [], []
    while len(low) < n:
        if len(low) % 2:  # r8x, declined by the CAP-8 build
            nub = int(rng.integers(9, OVF_NUB))
            d = int(rng.integers(9, nub + 1))
        else:             # ovf class, within CAP 16 (also with 8 or fewer: never built by K2)
            nub = int(rng.integers(OVF_NUB, 65))
            d = int(rng.integers(2, 17))
        msz = int(rng.integers(nub, 65))
        zi = msz > nub or (bool(rng.integers(0, 2)) and d >= 2)
        try:
            low.append(block(nub, d, msz, zi, rng))
        except ValueError:
            continue
    while len(high) < n:
        nub = int(rng.integers(17, 65))
        d = (17, nub)[len(high) % 2] if len(high) % 4 < 2 else int(rng.integers(17, nub + 1))
        msz = int(rng.integers(nub, 65))
        try:
            high.append(block(nub, d, msz, msz > nub, rng))
        except ValueError:
            continue
    low, high = np.stack(low), np.stack(high)
    assert not any(listed(b) for b in free)
    assert all(listed(b) and not listed_again(b) for b in low)
    assert all(listed_again(b) for b in high)
    return free, low, high


def gate_case(nblk, n_ovf, n17, seed, pools=None):
    """nblk blocks at shuffled positions, n_ovf of them listed by K2, n17 of
    those with more than 16 distinct symbols."""
    assert 0 <= n17 <= n_ovf <= nblk
    free, low, high = pools or gate_pools()
    rng = np.random.default_rng(seed)
    idx = np.concatenate([len(free) + len(low) + rng.integers(0, len(high), n17),
                          len(free) + rng.integers(0, len(low), n_ovf - n17),
                          rng.integers(0, len(free), nblk - n_ovf)])
    rng.shuffle(idx)
    return Case(np.concatenate([free, low, high]), idx)


def single_frame_gate_cases(gate, limit):
    """The issue's table a-g: [(name, nblk, n_ovf, n17)] for the single-frame
    gate (kR16GateSingle) and wave-pass limit (kWaveEncodeLimit)."""
    return [("a_no_tier_launched", gate, gate, 0),
            ("b_tier_launched_empty_list", gate + 1, 0, 0),
            ("c_tier_returns_wave_takes_work", gate + 1, gate, gate // 3),
            ("d_tier_takes_all_work2_empty", gate + 1 + 333, gate + 1, 0),
            ("e_every_listed_block_goes_on", gate + 1 + 333, gate + 1, gate + 1),
            ("f_wave_pass_on_work2", limit + 1 + 777, limit + 1 + 444, limit),
            ("g_lane_pass_on_work2", limit + 1 + 777, limit + 1 + 444, limit + 1)]


# ---- section 5: streams ----------------------------------------------------
def build_payload(plane_blocks, oracle):
    """The DCTYUV payload of three planes' zig-zag blocks (in each plane's
    row-major block order): three little-endian u32 plane sizes, then per
    plane u32 nblk, u32 content_size, nblk size bytes, the chunks.  `oracle`
    supplies huff_encode_block (or is a Chunks)."""
    ch = oracle if isinstance(oracle, Chunks) else Chunks(oracle.huff_encode_block)
    planes = []
    for blocks in plane_blocks:
        chunks = [ch.one(b) for b in np.asarray(blocks, np.int16).reshape(-1, 64)]
        content = b"".join(chunks)
        planes.append(struct.pack("<II", len(chunks), len(content)) + bytes(len(c) for c in chunks) + content)
    assert len(planes) == 3
    return struct.pack("<III", *(len(p) for p in planes)) + b"".join(planes)


def plane_counts(w, h):
    return (w // 8) * (h // 8), (w // 16) * (h // 16), (w // 16) * (h // 16)


def compose(plane_blocks, w, h, q, oracle):
    """The frame the stream must decode to: oracle.idct_block of every block
    at its place (the builder's self-check, and the decoder's reference built
    without the oracle's stream parser)."""
    out = np.zeros(w * h * 3 // 2, np.uint8)
    off = 0
    memo = {}
    for p, blocks in enumerate(plane_blocks):
        pw, ph = (w, h) if p == 0 else (w // 2, h // 2)
        Q = oracle.qtable(q[p], p != 0)
        plane = np.zeros((ph, pw), np.uint8)
        blocks = np.asarray(blocks, np.int16).reshape(-1, 64)
        assert len(blocks) == (pw // 8) * (ph // 8)
        for k, b in enumerate(blocks):
            key = b.tobytes()
            px = memo.get((p, key))
            if px is None:
                px = memo[(p, key)] = oracle.idct_block(natural(b), Q).reshape(8, 8).copy()
            by, bx = divmod(k, pw // 8)
            plane[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = px
        out[off:off + pw * ph] = plane.ravel()
        off += pw * ph
    return out.tobytes()


def saturated_fraction(frame):
    a = np.frombuffer(frame, np.uint8)
    return float(np.count_nonzero((a == 0) | (a == 255))) / a.size


def in_range_blocks(n, Q_natural, rng):
    """Coefficients a decoder may meet within the pixel range: a dequantised
    amplitude N(0, sigma = 400 / (1 + z)) per zig-zag index z, divided by Q,
    rounded (about 4-5 % of the decoded pixels saturate at any quality)."""
    z = np.arange(64)
    amp = rng.normal(0.0, 1.0, (n, 64)) * (400.0 / (1.0 + z))
    Qzz = np.asarray(Q_natural, np.float64)[ZZ]
    return np.clip(np.rint(amp / Qzz), -1024, 1023).astype(np.int16)


def _dct_basis():
    n = np.arange(8)
    return np.array([[(np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in n]
                     for u in n])


def extreme_blocks(n, rng):
    """All 64 coefficients at the format's extremes: all 1023, all -1024, the
    two alternations, then the signs of the DCT of random +-1 pixel patterns
    (with Q = 1, at quality 100, equal or random signs put most of a block's
    energy into few pixels and leave a third of them unclamped; these decode
    to about 93 % clamped pixels, and all of them do at Q = 255)."""
    C = _dct_basis()
    out = np.empty((n, 64), np.int16)
    for i in range(n):
        pat = rng.choice([-1.0, 1.0], (8, 8))
        out[i] = np.where(C @ pat @ C.T >= 0, 1023, -1024).ravel()[ZZ]
    for i, v in enumerate(([1023] * 64, [-1024] * 64, [1023, -1024] * 32, [-1024, 1023] * 32)):
        if i < n:
            out[i] = v
    return out


def _fill(n, blocks, rng=None):
    """n blocks: `blocks` first, then zero blocks (or repeats when rng)."""
    blocks = np.asarray(blocks, np.int16).reshape(-1, 64)
    assert len(blocks) <= n, (len(blocks), n)
    out = np.zeros((n, 64), np.int16)
    out[:len(blocks)] = blocks
    if rng is not None and len(blocks) < n:
        out[len(blocks):] = blocks[rng.integers(0, len(blocks), n - len(blocks))]
    return out


def one_coefficient_blocks():
    """Each of the 64 positions x {+-1, +-2, +-3, +-7, +-64, 1023, -1024}."""
    vals = (1, -1, 2, -2, 3, -3, 7, -7, 64, -64, 1023, -1024)
    out = np.zeros((64 * len(vals), 64), np.int16)
    for z in range(64):
        for j, v in enumerate(vals):
            out[z * len(vals) + j, z] = v
    return out


GROUP_K = (0, 1, 7, 8, 9, 56, 57, 63, 64)


def group_composition_blocks(Q_natural, seed=606):
    """64-block decoder groups with exactly k blocks that are not DC-only,
    k in GROUP_K, in the first k lanes, the last k lanes, and spread; the
    other lanes DC-only (some with DC 0).  Returns blocks [27 * 64, 64]."""
    rng = np.random.default_rng(seed)
    groups = []
    for k in GROUP_K:
        for place in ("first", "last", "spread"):
            g = np.zeros((64, 64), np.int16)
            g[:, 0] = rng.integers(-200, 200, 64)
            g[rng.integers(0, 64, 6), 0] = 0
            lanes = {"first": np.arange(k), "last": np.arange(64 - k, 64),
                     "spread": np.sort(rng.choice(64, k, replace=False))}[place]
            rest = in_range_blocks(k, Q_natural, rng)
            for b in rest:  # not DC-only, whatever the draw
                if not b[1:].any():
                    b[int(rng.integers(1, 64))] = 1
            g[lanes] = rest
            assert int((g[:, 1:] != 0).any(axis=1).sum()) == k
            groups.append(g)
    return np.concatenate(groups)


def sized_pool(chunks, seed=707):
    """{chunk size: block} over the sizes a seeded random search finds."""
    rng = np.random.default_rng(seed)
    by = {}
    for d in range(1, 65):
        for _ in range(24):
            nub = int(rng.integers(d, min(64, d + 12) + 1))
            msz = int(rng.integers(nub, 65))
            try:
                b = block(nub, d, msz, msz > nub, rng)
            except ValueError:
                continue
            by.setdefault(len(chunks.one(b)), b)
    return by


def group_of_total(by, total):
    """64 blocks whose chunk sizes sum to `total`: two neighbouring sizes."""
    base, extra = divmod(total, 64)
    assert base in by and (extra == 0 or base + 1 in by), (total, sorted(by))
    return np.stack([by[base + 1]] * extra + [by[base]] * (64 - extra))


STAGE_TOTALS = (5119, 5120, 5121, 5103, 5104, 5105)


def stage_boundary_groups(chunks, by):
    """64-block groups for the fused decoder's 5 KiB chunk stage (kStageQuads =
    320 quads; a round stages 319 quads from the 16-byte line of its first
    chunk): groups whose chunk bytes total 5,119 / 5,120 / 5,121 (the stage)
    and 5,103 / 5,104 / 5,105 (319 quads), a group of 64 longest chunks, and
    one longest chunk at lane 0 / lane 63 among 4-symbol chunks.
    Returns [(name, blocks[64, 64])]."""
    out = []
    for t in STAGE_TOTALS:
        g = group_of_total(by, t)
        assert sum(len(chunks.one(b)) for b in g) == t
        out.append((f"total_{t}", g))
    longest = by[max(by)]
    rng = np.random.default_rng(708)
    four = np.stack([block(4, 4, 4, False, rng) for _ in range(64)])
    out.append(("all_longest", np.stack([longest] * 64)))
    for lane in (0, 63):
        g = four.copy()
        g[lane] = longest
        out.append((f"longest_at_lane{lane}", g))
    return out


class Stream:
    def __init__(self, name, w, h, q, planes):
        self.name, self.w, self.h, self.q = name, w, h, tuple(q)
        self.planes = [np.asarray(p, np.int16).reshape(-1, 64) for p in planes]
        assert tuple(len(p) for p in self.planes) == plane_counts(w, h), (name, [len(p) for p in self.planes])
        self.kind = None  # "in_range" / "extreme": the saturation the test asserts

    def payload(self, chunks):
        return build_payload(self.planes, chunks)


def decoder_streams(oracle, chunks):
    """Every stream of the decoder tests: [Stream]."""
    out = []
    rng = np.random.default_rng(808)
    # DC sweep: all 2,048 DC-only blocks in the luma plane (512x256), and in
    # a chroma plane (1024x512)
    dc = dc_blocks()
    for q in (1, 25, 50, 88, 100):
        ny, nc, _ = plane_counts(512, 256)
        out.append(Stream(f"dc_sweep_luma_q{q}", 512, 256, (q, q, q),
                          [dc[rng.permutation(2048)], dc[rng.integers(0, 2048, nc)], np.zeros((nc, 64), np.int16)]))
        ny, nc, _ = plane_counts(1024, 512)
        out.append(Stream(f"dc_sweep_chroma_q{q}", 1024, 512, (q, q, q),
                          [dc[np.arange(ny) % 2048], dc, dc[::-1][rng.permutation(2048)]]))
    # one coefficient: 768 blocks in Y and in U of 512x384 (Y: 3,072 = 4 x 768)
    one = one_coefficient_blocks()
    ny, nc, _ = plane_counts(512, 384)
    assert nc == len(one)
    for q in (1, 50, 100):
        out.append(Stream(f"one_coefficient_q{q}", 512, 384, (q, q, q),
                          [np.concatenate([one, one[::-1], one[rng.permutation(nc)], one]), one,
                           one[rng.permutation(nc)]]))
    # group composition: 27 groups in Y of 512x256 (32 groups), 8 in each chroma plane
    for q in (50, 100):
        gy = group_composition_blocks(oracle.qtable(q, 0))
        gc = group_composition_blocks(oracle.qtable(q, 1), seed=607)
        ny, nc, _ = plane_counts(512, 256)
        out.append(Stream(f"group_composition_q{q}", 512, 256, (q, q, q),
                          [_fill(ny, gy, rng), gc[9 * 64:9 * 64 + nc], gc[-nc:]]))
    # stage boundary: 9 groups in Y of 256x192 (12 groups), the rest in range;
    # three of them in each chroma plane
    by = sized_pool(chunks)
    groups = stage_boundary_groups(chunks, by)
    ny, nc, _ = plane_counts(256, 192)
    gb = np.concatenate([g for _, g in groups])
    tail = in_range_blocks(ny - len(gb), oracle.qtable(50, 0), rng)
    out.append(Stream("stage_boundary", 256, 192, (50, 50, 50),
                      [np.concatenate([gb, tail]), np.concatenate([groups[1][1], groups[6][1], groups[0][1]]),
                       np.concatenate([groups[8][1], groups[2][1], groups[7][1]])]))
    # (the same groups behind one of 64 x 20 + 9 bytes: the groups' first
    # chunks on other bytes of their 16-byte lines)
    shim = group_of_total(by, 64 * 20 + 9)
    out.append(Stream("stage_boundary_shifted", 256, 192, (50, 50, 50),
                      [np.concatenate([shim, gb, tail[64:]]),
                       np.concatenate([groups[3][1], groups[4][1], groups[5][1]]),
                       np.concatenate([groups[6][1], groups[5][1], groups[3][1]])]))
    # magnitude: the clamp (all-extreme) and the arithmetic (in range)
    for q in (1, 100):
        ny, nc, _ = plane_counts(128, 128)
        s = Stream(f"extreme_q{q}", 128, 128, (q, q, q),
                   [extreme_blocks(ny, rng), extreme_blocks(nc, rng), extreme_blocks(nc, rng)[::-1]])
        s.kind = "extreme"
        out.append(s)
    for q in (1, 50, 100):
        ny, nc, _ = plane_counts(128, 128)
        s = Stream(f"in_range_q{q}", 128, 128, (q, q, q),
                   [in_range_blocks(ny, oracle.qtable(q, 0), rng), in_range_blocks(nc, oracle.qtable(q, 1), rng),
                    in_range_blocks(nc, oracle.qtable(q, 1), rng)])
        s.kind = "in_range"
        out.append(s)
    # geometry: groups of 4 + 1 + 1 blocks; plane block counts that are no multiple of 64
    pool = np.concatenate([mixed_pool(), in_range_blocks(64, oracle.qtable(50, 0), rng), extreme_blocks(8, rng)])
    for w, h in ((16, 16), (144, 272)):
        out.append(Stream(f"geometry_{w}x{h}", w, h, (50, 60, 70),
                          [pool[rng.integers(0, len(pool), n)] for n in plane_counts(w, h)]))
    return out


def batch_pair(oracle):
    """Two different streams of one geometry and quality for one 2-frame
    decompress_batch_device call."""
    rng = np.random.default_rng(909)
    w, h, q = 144, 272, (50, 50, 50)
    pool = np.concatenate([mixed_pool(), in_range_blocks(64, oracle.qtable(50, 0), rng), extreme_blocks(8, rng),
                           dc_blocks()[::37]])
    return [Stream(f"batch_{i}", w, h, q, [pool[rng.integers(0, len(pool), n)] for n in plane_counts(w, h)])
            for i in range(2)]



# ---- what the test modules share -------------------------------------------
class Shared:
    """Built once per session: the oracle's chunks, the decoder streams, their
    payloads and the oracle's decode of each (never modified)."""

    def __init__(self, oracle):
        self.chunks = Chunks(oracle.huff_encode_block)
        self.streams = decoder_streams(oracle, self.chunks) + batch_pair(oracle)
        self.by_name = {s.name: s for s in self.streams}
        self._oracle = oracle
        self._decoded = {}

    def payload(self, name):
        return self.decoded(name)[0]

    def decoded(self, name):
        """(payload, oracle.decompress of it)."""
        if name not in self._decoded:
            s = self.by_name[name]
            pay = s.payload(self.chunks)
            self._decoded[name] = (pay, self._oracle.decompress(pay, s.w, s.h, s.q))
        return self._decoded[name]


_SHARED = None


def shared(oracle):
    global _SHARED
    if _SHARED is None:
        _SHARED = Shared(oracle)
    return _SHARED


def stream_names():
    """The names of decoder_streams() (for parametrising: needs no oracle;
    test_coef_domain.py checks the two agree)."""
    return ([f"dc_sweep_{p}_q{q}" for q in (1, 25, 50, 88, 100) for p in ("luma", "chroma")] +
            [f"one_coefficient_q{q}" for q in (1, 50, 100)] + [f"group_composition_q{q}" for q in (50, 100)] +
            ["stage_boundary", "stage_boundary_shifted", "extreme_q1", "extreme_q100"] +
            [f"in_range_q{q}" for q in (1, 50, 100)] + ["geometry_16x16", "geometry_144x272"])

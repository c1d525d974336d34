"""Inputs and the host check for K1's zero-row rule (csrc/fdct_bfly.h "Zero
rows", bfly_zero_row): a wave whose 16 blocks all pass the rule for rows 4..7
leaves those rows' stage 2 out.

tools/diag/fdct_zero_rows_check.cpp runs the rule through the shared header
(the kernel's operations) and says, per block, which of rows 4..7 pass
(`votes`, 15 = the block qualifies) and the four decision values bit for bit;
it also checks that a passing row is zero in the fast path's emulation and in
the reference transform and that the existing per-row proof passes for it.
Expected values are never stored: the tests compute them with this tool, the
emulation (fdctgen) and the oracle."""
import os
import shutil
import struct
import subprocess
from collections import namedtuple

import numpy as np

import fdctgen as G

CHECK_SRC = os.path.join(G.ROOT, "tools", "diag", "fdct_zero_rows_check.cpp")
QUALITIES = (1, 10, 50, 75, 90, 100)


def build_check(outdir, mutant=0, sanitize=False):
    """Compiles the check as fdctgen.build_emulation compiles its tool;
    mutant 3: the rule's constant halved; sanitize: -fsanitize=address,undefined
    (a stand-alone host program).  None without a C++ compiler."""
    cxx = shutil.which("g++")
    if not cxx:
        return None
    exe = os.path.join(str(outdir), f"fdct_zero_rows_check{mutant}{'_san' if sanitize else ''}")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-fno-fast-math", f"-DMYYUV_BFLY_MUTANT={mutant}", *san, "-o",
                    exe, CHECK_SRC, "-lm"], check=True)
    return exe


# votes: bit i - 4 set when row i of the block passes; dec[:, i - 4]: the rule's
# decision value of row i (float32, bit for bit; the row passes when < 0.5)
Rule = namedtuple("Rule", "votes dec summary")


def run_check(exe, px, Q, expect_violations=False):
    px = np.ascontiguousarray(px, np.uint8).reshape(-1, 64)
    blocks = np.concatenate([px, np.zeros((len(px), 1), np.uint8)], 1)
    qt = np.ascontiguousarray(Q, np.float32).reshape(64)
    data = struct.pack("<I", len(px)) + blocks.tobytes() + np.tile(qt, 3).tobytes()
    r = subprocess.run([exe], input=data, capture_output=True, timeout=600)
    assert r.returncode == 0 or (expect_violations and r.returncode == 1), \
        r.stdout.decode()[:300] + r.stderr.decode()[-2000:]
    lines = r.stdout.decode().split("\n")
    f = lines[0].split()
    summary = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
    rows = [ln.split() for ln in lines[1:] if ln]
    assert len(rows) == len(px) == summary["blocks"]
    votes = np.array([int(x[1]) for x in rows], np.int64)
    dec = np.array([[int(v, 16) for v in x[2:6]] for x in rows], np.uint32).reshape(-1, 4).view(np.float32)
    assert summary["blocks_pass"] == (votes == 15).sum()
    return Rule(votes, dec, summary)


def qualifies(exe, px, Q):
    """Per block: rows 4..7 all pass (what the block's lanes vote in fdct_fast)."""
    return run_check(exe, px, Q).votes == 15


def tested(exe, Q):
    """The plane's units are tested at all (fdct_bfly.h bfly_zero_rows_tested:
    planes whose row 4 has an entry below 6 are not)."""
    return bool(run_check(exe, np.zeros((0, 64), np.uint8), Q).summary["tested"] & 1)


def units_skip(qual, nblocks=None):
    """Per 16-block unit: every live block qualifies (the wave skips)."""
    q = np.asarray(qual, bool)
    n = len(q) if nblocks is None else nblocks
    return np.array([q[u:min(u + 16, n)].all() for u in range(0, n, 16)])


# ---- tables -----------------------------------------------------------------
def quality_tables(oracle):
    """{name: Q} for q in QUALITIES, luma and chroma."""
    return {f"q{q}_{'luma' if p == 0 else 'chroma'}": oracle.qtable(q, p) for q in QUALITIES for p in (0, 1)}


# ---- blocks -----------------------------------------------------------------
_M = np.arange(8)


def basis(f):
    """cos((2m + 1) f pi / 16), m = 0..7: the shape of DCT row f."""
    return np.cos((2 * _M + 1) * f * np.pi / 16)


def pattern_block(base, amp, f, v):
    """A flat block of level `base` plus amp * (vertical frequency f) x
    (horizontal frequency v), rounded and clamped to pixels: its energy lands
    in row f of T, and in output (f, v) of that row."""
    p = base + amp * np.outer(basis(f), basis(v) / np.abs(basis(v)).max())
    return np.clip(np.rint(p), 0, 255).astype(np.uint8).reshape(64)


def largest_reciprocal_column(Q, f):
    return int(np.argmin(np.asarray(Q, np.float32).reshape(8, 8)[f]))


def spoiler_block(exe, Q, f, base=128):
    """The weakest pattern block of frequency f whose row f fails the rule
    under Q while the other three rows pass: a block that alone keeps its unit
    from skipping, because of row f."""
    v = largest_reciprocal_column(Q, f)
    amps = np.arange(0.25, 140.0, 0.25)
    px = np.stack([pattern_block(base, a, f, v) for a in amps])
    votes = run_check(exe, px, Q).votes
    want = 15 & ~(1 << (f - 4))
    hit = np.flatnonzero(votes == want)
    assert len(hit), (f, "no block fails in row f alone")
    return px[hit[0]]


def sparse_blocks(f, base=128):
    """Level `base` with 1 to 3 pixels of one column (column 0) moved by 1, 2
    or 3 in the direction of basis(f): row f of T gets S = a * sum |N[f][m]|
    over the moved rows, fine steps from 0.1 up (the threshold at Q = 1 is
    S ~ 1)."""
    from itertools import combinations
    sgn = np.sign(basis(f)).astype(np.int64)
    out = []
    for n in (1, 2, 3):
        for rows in combinations(range(8), n):
            for a in (1, 2, 3):
                b = np.full((8, 8), base, np.int64)
                for m in rows:
                    b[m, 0] += a * sgn[m]
                out.append(b.reshape(64))
    return np.array(out, np.uint8)


def threshold_family(exe, Q, bases=(128, 96, 171), step=0.125, top=140.0):
    """Blocks whose row f = 4, 5, 6, 7 straddles the rule's threshold.  Per
    frequency, base level, sign and width w in (8, 4, 2, 1) an amplitude ramp
    of pattern blocks (the energy in the column with the row's largest
    reciprocal; only the first w pixel columns carry the pattern, so that S
    moves in steps finer than a whole row of +-1 pixels), and sparse_blocks.
    Kept: the blocks with row f's decision value in [0.25, 1): the last passing
    and the first failing amplitudes, and the values on either side up to a
    factor of two.  Returns (blocks, f per block)."""
    amps = np.arange(step, top, step)
    px, fs = [], []
    for f in (4, 5, 6, 7):
        v = largest_reciprocal_column(Q, f)
        pat = np.outer(basis(f), basis(v) / np.abs(basis(v)).max())  # pattern_block's, every amplitude at once
        series = [sparse_blocks(f, base) for base in bases]
        for w in (8, 4, 2, 1):
            pw = pat * (np.arange(8) < w)[None, :]
            for base in bases:
                for sign in (1.0, -1.0):
                    ramp = np.clip(np.rint(base + sign * amps[:, None, None] * pw[None]), 0, 255).astype(np.uint8)
                    series.append(ramp.reshape(-1, 64))
        blocks = np.unique(np.concatenate(series), axis=0)
        px.append(blocks)
        fs.append(np.full(len(blocks), f))
    px, fs = np.concatenate(px), np.concatenate(fs)
    dec = run_check(exe, px, Q).dec[np.arange(len(px)), fs - 4]
    keep = (dec >= 0.25) & (dec < 1.0)
    return px[keep], fs[keep]


def flat(level, n=1):
    return np.full((n, 64), level, np.uint8)

"""Pixel-domain edge inputs for K1 (the forward DCT, k_fdct_quant and its exact
path k_fdct_fix) and the host emulation they are judged by.

K1's fast path is proven per block by a bound (csrc/fdct_bfly.h); the blocks
it cannot prove are listed for the exact path.  tools/diag/fdct_bfly_check.cpp
emulates the fast path operation for operation; with --per-block it says, per
block, whether the block is proven (`ok`), which output decided, and the
decision value fma(A, kb[row], max |e|) bit for bit.  The families here put
blocks where that emulation and a GPU build can part: at the decision's
threshold, at the reference's rounding ties, at tiny and saturated A, and at
every Q.  Expected values are never stored: the tests compute them with the
emulation and the oracle.

The searched blocks (threshold, AC near ties) are in tests/golden/
fdct_edges.npz, made by tests/golden/make_fdct_edges.py; everything else is
generated here, deterministically."""
import json
import os
import shutil
import struct
import subprocess
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHECK_SRC = os.path.join(ROOT, "tools", "diag", "fdct_bfly_check.cpp")
FIXTURE = os.path.join(HERE, "golden", "fdct_edges.npz")

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                   13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,
                   52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ---- tables ---------------------------------------------------------------
TABLE_NAMES = ["q50_luma", "q90_luma", "q100_luma", "q50_chroma", "uniform1", "uniform2", "spiky"]
TIE_TABLES = ["q50_luma", "q90_luma", "uniform1", "uniform2", "spiky"]  # AC near ties are searched for these
SPIKY_COLUMN = 3


def uniform(k):
    return np.full(64, k, np.float32)


def spiky():
    """255 everywhere except one column of 1: the largest 1/Q of every row, so
    every row's bound factor kb, comes from a single output."""
    q = np.full((8, 8), 255, np.float32)
    q[:, SPIKY_COLUMN] = 1
    return q.reshape(64)


def tables(oracle):
    return {"q50_luma": oracle.qtable(50, 0), "q90_luma": oracle.qtable(90, 0), "q100_luma": oracle.qtable(100, 0),
            "q50_chroma": oracle.qtable(50, 1), "uniform1": uniform(1), "uniform2": uniform(2), "spiky": spiky()}


# ---- the emulation --------------------------------------------------------
def build_emulation(outdir, mutant=0):
    """Compiles tools/diag/fdct_bfly_check.cpp as test_numerics.py does;
    mutant 1 / 2: the deliberately wrong builds of fdct_bfly.h.  None without
    a C++ compiler."""
    cxx = shutil.which("g++")
    if not cxx:
        return None
    exe = os.path.join(str(outdir), f"fdct_bfly_check{mutant}")
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-fno-fast-math", f"-DMYYUV_BFLY_MUTANT={mutant}", "-o", exe,
                    CHECK_SRC, "-lm"], check=True)
    return exe


# per block: ok; the deciding row and column; dec = the largest fma(A, kb[row],
# max |e|) and t = the deciding output's quantised value (float32, bit for
# bit); where the reference's fl(Y_ref / Q) is nearest to a half-integer and
# how near.  index: the block's position in the input (all of them unless a
# window was given).  maxratio: the largest |t - fl(Y_ref / Q)| / (A kb[row]).
Emu = namedtuple("Emu", "index ok row col dec t tie_row tie_col tie summary maxratio")


def emulate(exe, px, Q, dec_window=None, tie_window=None):
    px = np.ascontiguousarray(px, np.uint8).reshape(-1, 64)
    blocks = np.concatenate([px, np.zeros((len(px), 1), np.uint8)], 1)
    qt = np.ascontiguousarray(Q, np.float32).reshape(64)
    data = struct.pack("<I", len(px)) + blocks.tobytes() + np.tile(qt, 3).tobytes()
    cmd = [exe, "--per-block"]
    if dec_window is not None:
        cmd += ["--dec-window", repr(float(dec_window))]
    if tie_window is not None:
        cmd += ["--tie-window", repr(float(tie_window))]
    r = subprocess.run(cmd, input=data, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[:500] + r.stderr.decode()[-2000:]
    lines = r.stdout.decode().split("\n")
    f = lines[0].split()
    summary = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
    assert lines[1].startswith("maxratio ")
    maxratio = float(lines[1].split()[1])
    rows = [ln.split() for ln in lines[2:] if ln]
    ints = np.array([[int(x[0]), int(x[1]), int(x[2]), int(x[3]), int(x[6]), int(x[7])] for x in rows],
                    np.int64).reshape(-1, 6)
    bits = np.array([[int(x[4], 16), int(x[5], 16), int(x[8], 16)] for x in rows], np.uint32).reshape(-1, 3)
    fl = bits.view(np.float32)
    return Emu(ints[:, 0], ints[:, 1].astype(bool), ints[:, 2], ints[:, 3], fl[:, 0].copy(), fl[:, 1].copy(),
               ints[:, 4], ints[:, 5], fl[:, 2].copy(), summary, maxratio)


def on_threshold(dec, t):
    """The threshold family's condition: the decision value within 4 ulps of
    the deciding t, and within 2^-20, of 0.5 (e = t - rint(t) moves in steps of
    ulp(t), so a one-ulp difference in t crosses such a margin)."""
    dec = np.asarray(dec, np.float32)
    ulp = np.spacing(np.abs(np.asarray(t, np.float32)))
    w = np.minimum(4.0 * ulp.astype(np.float64), 2.0 ** -20)
    return np.abs(dec.astype(np.float64) - 0.5) <= w


TIE_WINDOW = 2.0 ** -18
K_BFLY = np.float32(7.946e-7)  # fdct_bfly.h kBflyK (used only to select near ties, below)


def block_a(px):
    return np.abs(np.asarray(px, np.int64).reshape(-1, 64) - 128).sum(1)


def tie_margin_ok(px, Q, tie_row, tie):
    """A near tie at distance d from the half-integer is listed by the fast
    path when d + |t_fast - fl(Y_ref / Q)| <= A kb[row]: the searched near
    ties keep d <= A kb[row] / 2 (kb: fdct_bfly.h bfly_row_bounds), half the
    bound left for the fast path's own error."""
    r = (np.float32(1) / np.asarray(Q, np.float32)).reshape(8, 8).astype(np.float64)
    kb = float(K_BFLY) * r.max(1) * (1 + 2.0 ** -20) * (1 + 2.0 ** -22)
    return np.asarray(tie, np.float64) <= 0.5 * block_a(px) * kb[np.asarray(tie_row)]


# ---- generated families ---------------------------------------------------
def flat_blocks():
    """All 256 flat blocks.  At a DC entry of 16 the odd offsets from 128 are
    ties of the reference's roundf (8 d / 16); at 2, 4 and 8 the quotient is
    an integer."""
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 64, 1)


FLAT_TIE_DC = (2, 4, 8, 16)


def small_a_blocks():
    """A = sum |x - 128| in 1..16: every single pixel at +-1..+-4, and 512
    pairs of pixels with |a| + |b| <= 16."""
    out = []
    for i in range(64):
        for a in (1, 2, 3, 4, -1, -2, -3, -4):
            b = np.full(64, 128, np.int64)
            b[i] += a
            out.append(b)
    rng = np.random.default_rng(41)
    for _ in range(512):
        i, j = rng.choice(64, 2, replace=False)
        a = int(rng.integers(1, 16))
        c = int(rng.integers(1, 17 - a))
        b = np.full(64, 128, np.int64)
        b[i] += a * int(rng.choice([-1, 1]))
        b[j] += c * int(rng.choice([-1, 1]))
        out.append(b)
    out = np.array(out, np.uint8)
    a = block_a(out)
    assert a.min() >= 1 and a.max() <= 16
    return out


def saturated_blocks():
    """Pixels 0 or 255 only (A = 8,192 - n255): stripes of period 2, 4 and 8 in
    both orientations and both phases, checkers of cell 1, 2 and 4 in both
    phases, the two flat ones, and 192 random binary blocks."""
    y, x = np.mgrid[0:8, 0:8]
    out = [np.zeros((8, 8), bool), np.ones((8, 8), bool)]
    for cell in (1, 2, 4):
        for ph in (0, 1):
            out.append((x // cell + ph) % 2 == 1)
            out.append((y // cell + ph) % 2 == 1)
            out.append((x // cell + y // cell + ph) % 2 == 1)
    rng = np.random.default_rng(43)
    for i in range(192):
        out.append(rng.random((8, 8)) < (0.5 if i < 128 else rng.random()))
    return (np.array(out).reshape(-1, 64) * 255).astype(np.uint8)


# ---- the fixture ----------------------------------------------------------
def load_fixture():
    """{"threshold" / "near_tie": {table name: uint8[n, 64]}, "manifest": dict}"""
    z = np.load(FIXTURE)
    out = {"manifest": json.loads(str(z["manifest"]))}
    for fam, key in (("threshold", "thr"), ("near_tie", "tie")):
        px, tb = z[key + "_px"], z[key + "_table"]
        out[fam] = {name: px[tb == i] for i, name in enumerate(TABLE_NAMES) if (tb == i).any()}
    return out


def threshold_manifest(emu, flips):
    """What the threshold blocks of one table reach, from a fresh emulation
    run (emu: all blocks; flips: per mutant, how many blocks it lists
    otherwise)."""
    on = on_threshold(emu.dec, emu.t)
    m = {"blocks": int(len(emu.ok)), "off_threshold": int((~on).sum())}
    for side, sel in (("listed", ~emu.ok), ("proven", emu.ok)):
        m[side] = int(sel.sum())
        m["rows_" + side] = sorted(set(int(r) for r in emu.row[sel]))
        m["cols_" + side] = sorted(set(int(c) for c in emu.col[sel]))
    m["mutant_flips"] = [int(f) for f in flips]
    return m


def near_tie_manifest(emu):
    return {"blocks": int(len(emu.ok)), "listed": int((~emu.ok).sum()),
            "ac": int(((emu.tie_row != 0) & (emu.tie_col != 0)).sum()),
            "rows": sorted(set(int(r) for r in emu.tie_row)), "cols": sorted(set(int(c) for c in emu.tie_col))}


def every_q_pool(fix):
    """64 blocks drawn from the families, for the uniform tables Q = 1..255."""
    thr = np.concatenate([fix["threshold"][n][i::40][:4] for i, n in enumerate(TABLE_NAMES)])[:24]
    tie = np.concatenate([fix["near_tie"][n][:2] for n in TIE_TABLES])[:8]
    pool = np.concatenate([thr, tie, flat_blocks()[[0, 1, 127, 128, 129, 131, 254, 255]],
                           small_a_blocks()[5::80][:12], saturated_blocks()[::19][:12]])
    assert pool.shape == (64, 64), pool.shape
    return pool


# ---- units (block_geom: 16 consecutive blocks) ------------------------------
def fix_list_cap(units):
    """csrc/codec_common.hpp fix_list_cap: 16 entries per unit of a list, the
    units dealt to 32 lists."""
    return 16 * ((units + 31) // 32)


LISTED_BLOCK = np.full(64, 129, np.uint8)  # at Q = 16 a tie of the reference's roundf (8 / 16): never proven
PROVEN_BLOCK = np.full(64, 128, np.uint8)  # A = 0: every decision value is 0


# ---- every family and table -------------------------------------------------
def case_names():
    out = ["threshold-" + n for n in TABLE_NAMES] + ["near_tie-" + n for n in TIE_TABLES]
    out += [f"flat-uniform{dc}" for dc in FLAT_TIE_DC] + ["small_a-uniform1", "small_a-uniform2"]
    return out + ["saturated-" + n for n in TABLE_NAMES]


def case(name, fix, tabs):
    """(pixel blocks, Q table) of one family and table."""
    fam, tab = name.split("-")
    if fam == "flat":
        return flat_blocks(), uniform(int(tab[len("uniform"):]))
    if fam in ("threshold", "near_tie"):
        return fix[fam][tab], tabs[tab]
    return {"small_a": small_a_blocks, "saturated": saturated_blocks}[fam](), tabs[tab]


def plane_from_blocks(blocks, pw, ph):
    """A pw x ph plane whose 8x8 blocks, in raster order, are `blocks` in turn
    (repeated as often as it takes)."""
    n = (pw // 8) * (ph // 8)
    b = np.asarray(blocks, np.uint8).reshape(-1, 64)
    b = b[np.arange(n) % len(b)].reshape(ph // 8, pw // 8, 8, 8)
    return b.transpose(0, 2, 1, 3).reshape(ph, pw)


def plane_blocks(plane):
    ph, pw = plane.shape
    return plane.reshape(ph // 8, 8, pw // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)

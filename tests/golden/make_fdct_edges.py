"""Generates tests/golden/fdct_edges.npz: the searched inputs of tests/fdctgen.py
(inputs only; expected values are computed at test time).

Per table of fdctgen.TABLE_NAMES, a random and directed search with the host
emulation (tools/diag/fdct_bfly_check.cpp --per-block) for
  threshold blocks: the decision value fma(A, kb[row], max |e|) within 4 ulps
    of the deciding t, and within 2^-20, of 0.5 (fdctgen.on_threshold), at
    least PER_SIDE listed and PER_SIDE proven; for uniform1 the deciding
    outputs cover all 8 rows and all 8 columns on each side; and for each
    mutant build of the emulation (fdct_bfly.h MYYUV_BFLY_MUTANT) at least
    MIN_FLIPS blocks that it lists otherwise;
  near ties (fdctgen.TIE_TABLES): the reference's fl(Y_ref / Q) within 2^-18
    of a half-integer at a row and a column other than 0, with the margin of
    fdctgen.tie_margin_ok.
What was reached is stored as the manifest; tests/test_fdct_edges.py checks it
against a fresh emulation run.
Run from the repo root: python tests/golden/make_fdct_edges.py"""
import json
import os
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fdctgen as G  # noqa: E402
from oracle import oracle as O  # noqa: E402

PER_SIDE, MIN_FLIPS, N_TIES, CHUNK, MAX_CHUNKS = 64, 2, 32, 400_000, 60


def basis(u, v):
    k = np.arange(8)
    c = lambda w: np.cos((2 * k + 1) * w * np.pi / 16) * (np.sqrt(0.125) if w == 0 else 0.5)
    return np.outer(c(u), c(v))


def candidates(rng, n, round_):
    """n mixed blocks: noise, low noise around a level, gradients, and one
    basis function at a random amplitude plus +-0..3 noise (every fourth round
    the basis functions of row or column 4, which are what kC4 reaches)."""
    q = n // 4
    out = [rng.integers(0, 256, (q, 64))]
    lvl = rng.integers(8, 248, (q, 1))
    out.append(lvl + rng.integers(-8, 9, (q, 64)) * rng.integers(0, 2, (q, 1)) + rng.integers(-2, 3, (q, 64)))
    gx, gy = rng.integers(-12, 13, (2, q, 1))
    yy, xx = np.mgrid[0:8, 0:8].reshape(2, 1, 64)
    out.append(128 + gx * (xx - 3) + gy * (yy - 3) + rng.integers(-3, 4, (q, 64)))
    u, v = rng.integers(0, 8, (2, n - 3 * q))
    if round_ % 4 == 3:
        four = rng.integers(0, 2, len(u)).astype(bool)
        u = np.where(four, 4, u)
        v = np.where(~four, 4, v)
    B = np.array([[basis(a, b).reshape(64) for b in range(8)] for a in range(8)])
    amp = rng.uniform(-1000, 1000, (len(u), 1))
    out.append(np.rint(128 + amp * B[u, v]) + rng.integers(-3, 4, (len(u), 64)) * rng.integers(0, 2, (len(u), 1)))
    return np.clip(np.concatenate(out), 0, 255).astype(np.uint8)


def covers(name, emu):
    if name != "uniform1":
        return True
    return all(len(set(x[sel])) == 8 for sel in (emu.ok, ~emu.ok) for x in (emu.row, emu.col))


def pick(name, emu, flips):
    """Indices into the threshold candidates: the mutants' flips, the rows and
    columns each side can cover, then the first found up to PER_SIDE a side."""
    chosen = []
    for f in flips:
        chosen += list(np.flatnonzero(f)[:MIN_FLIPS + 2])
    for sel in (emu.ok, ~emu.ok):
        for x in (emu.row, emu.col):
            for val in range(8):
                hit = np.flatnonzero(sel & (x == val))
                if len(hit) and not any(i in chosen for i in hit):
                    chosen.append(hit[0])
    chosen = list(dict.fromkeys(int(i) for i in chosen))
    for sel in (emu.ok, ~emu.ok):
        have = sum(1 for i in chosen if sel[i])
        for i in np.flatnonzero(sel):
            if have >= PER_SIDE:
                break
            if int(i) not in chosen:
                chosen.append(int(i))
                have += 1
    return sorted(chosen)


def search(name, Q, exes, seed):
    rng = np.random.default_rng(seed)
    thr = np.zeros((0, 64), np.uint8)
    ties = np.zeros((0, 64), np.uint8)
    want_ties = name in G.TIE_TABLES
    for round_ in range(MAX_CHUNKS):
        px = candidates(rng, CHUNK, round_)
        need_ties = want_ties and len(ties) < N_TIES
        e = G.emulate(exes[0], px, Q, dec_window=2.0 ** -20, tie_window=G.TIE_WINDOW if need_ties else None)
        assert e.summary["mismatches"] == 0
        sel = G.on_threshold(e.dec, e.t)
        thr = np.unique(np.concatenate([thr, px[e.index[sel]]]), axis=0)
        if need_ties:
            t = (e.tie <= G.TIE_WINDOW) & (e.tie_row != 0) & (e.tie_col != 0)
            t &= G.tie_margin_ok(px[e.index], Q, e.tie_row, e.tie)
            ties = np.unique(np.concatenate([ties, px[e.index[t]]]), axis=0)
        full = G.emulate(exes[0], thr, Q)
        flips = [G.emulate(x, thr, Q).ok != full.ok for x in exes[1:]]
        done = (full.ok.sum() >= PER_SIDE and (~full.ok).sum() >= PER_SIDE and covers(name, full)
                and all(f.sum() >= MIN_FLIPS for f in flips) and (not want_ties or len(ties) >= N_TIES))
        print(f"{name}: round {round_} proven {full.ok.sum()} listed {(~full.ok).sum()} flips "
              f"{[int(f.sum()) for f in flips]} ties {len(ties)}", flush=True)
        if done:
            break
    keep = pick(name, full, flips)
    if len(ties):  # one of each tie position in turn, so the positions spread
        e = G.emulate(exes[0], ties, Q)
        pos = e.tie_row * 8 + e.tie_col
        rank = np.array([np.sum(pos[:i] == pos[i]) for i in range(len(pos))])
        ties = ties[np.sort(np.lexsort((pos, rank))[:N_TIES])]
    return thr[keep], ties


def main():
    tabs = G.tables(O)
    with tempfile.TemporaryDirectory() as d:
        exes = [G.build_emulation(d, m) for m in (0, 1, 2)]
        with ThreadPoolExecutor(len(tabs)) as ex:
            found = list(ex.map(lambda it: search(it[1], tabs[it[1]], exes, 100 + it[0]), enumerate(G.TABLE_NAMES)))
        man = {}
        for name, (thr, ties) in zip(G.TABLE_NAMES, found):
            full = G.emulate(exes[0], thr, tabs[name])
            flips = [(G.emulate(x, thr, tabs[name]).ok != full.ok).sum() for x in exes[1:]]
            man[name] = {"threshold": G.threshold_manifest(full, flips)}
            if len(ties):
                man[name]["near_tie"] = G.near_tie_manifest(G.emulate(exes[0], ties, tabs[name]))
            print(name, json.dumps(man[name]))
    cat = lambda k: np.concatenate([f[k] for f in found])
    idx = lambda k: np.concatenate([np.full(len(f[k]), i, np.uint8) for i, f in enumerate(found)])
    out = os.path.join(HERE, "fdct_edges.npz")
    np.savez_compressed(out, thr_px=cat(0), thr_table=idx(0), tie_px=cat(1), tie_table=idx(1),
                        manifest=np.array(json.dumps(man, sort_keys=True)))
    print(len(cat(0)), "threshold blocks,", len(cat(1)), "near ties,", os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 128 * 1024


if __name__ == "__main__":
    main()

"""K1's zero-row rule on the host (csrc/fdct_bfly.h bfly_zero_row; tests/
zerorows.py): whenever the rule passes for a row i in 4..7 of a block, the
fast path's emulation and the reference transform give 0 for the row's eight
outputs and the row's existing proof passes (its decision value < 0.5), and
every block the emulation proves equals the reference.  So a wave that leaves
rows 4..7 out stores and lists what it would have otherwise.  Checked by
tools/diag/fdct_zero_rows_check.cpp (a stand-alone program, also run built with
-fsanitize=address,undefined) on every family and table of the edge tests, on
the uniform tables Q = 1..255, and on a family searched to straddle the rule's
threshold; a build with the rule's constant halved is told from the real one."""
import numpy as np
import pytest

import fdctgen as G
import zerorows as Z


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("fdct_zero_rows")
    out = {"real": Z.build_check(d), "mutant": Z.build_check(d, mutant=3), "san": Z.build_check(d, sanitize=True)}
    if out["real"] is None:
        pytest.skip("no C++ compiler")
    return out


@pytest.fixture(scope="module")
def fix():
    return G.load_fixture()


@pytest.fixture(scope="module")
def families(exes, oracle):
    """{table name: (blocks, f per block, Q)}: the threshold family at the
    quality tables q in {1, 10, 50, 75, 90, 100}, luma and chroma."""
    return {name: Z.threshold_family(exes["real"], Q) + (Q,) for name, Q in Z.quality_tables(oracle).items()}


def test_rule_implies_proof_on_edge_families(exes, fix, oracle):
    """violations == 0 over every family of the edge tests at its tables and
    over the pool at Q = 1..255; the rule both passes and fails there."""
    tabs = G.tables(oracle)
    runs = [(n,) + G.case(n, fix, tabs) for n in G.case_names()]
    pool = G.every_q_pool(fix)
    runs += [(f"every_q-{k}", pool, G.uniform(k)) for k in range(1, 256)]
    rows_pass = rows_fail = 0
    for name, px, Q in runs:
        s = Z.run_check(exes["real"], px, Q).summary
        assert s["violations"] == 0, name
        rows_pass += s["rows_pass"]
        rows_fail += s["rows_fail"]
    print(f"\nrows 4..7 over {len(runs)} runs: {rows_pass} pass the rule, {rows_fail} fail")
    assert rows_pass > 1000 and rows_fail > 1000


def test_threshold_family(exes, families):
    """The searched family: no violation; at least 64 blocks whose row f
    passes and 64 whose row f fails, all with the rule's decision value within
    a factor of two of 0.5, and on each side blocks within 10 % of it."""
    npass = nfail = near_pass = near_fail = 0
    for name, (px, fs, Q) in families.items():
        r = Z.run_check(exes["real"], px, Q)
        assert r.summary["violations"] == 0, name
        dec = r.dec[np.arange(len(px)), fs - 4]
        ok = (r.votes >> (fs - 4)) & 1 == 1
        assert np.array_equal(ok, dec < 0.5) and (dec >= 0.25).all() and (dec < 1.0).all(), name
        npass, nfail = npass + ok.sum(), nfail + (~ok).sum()
        near_pass, near_fail = near_pass + (ok & (dec >= 0.45)).sum(), near_fail + (~ok & (dec < 0.55)).sum()
        for f in (4, 5, 6, 7):
            if not name.startswith("q100"):  # (at Q = 1 a single pixel step crosses the threshold)
                assert ok[fs == f].any() and (~ok[fs == f]).any(), (name, f)
    print(f"\nthreshold family: {npass} pass, {nfail} fail; within 10 %: {near_pass} pass, {near_fail} fail")
    assert npass >= 64 and nfail >= 64
    assert near_pass >= 64 and near_fail >= 64


def test_q100_only_flat_rows_pass(exes, oracle):
    """At Q = 1 a row passes only when it is (all but) empty: every flat block
    qualifies, and no block of the saturated family with energy in rows 4..7."""
    Q = oracle.qtable(100, 0)
    assert (Q == 1).all()
    assert Z.qualifies(exes["real"], G.flat_blocks(), Q).all()
    assert not Z.qualifies(exes["real"], Z.threshold_family(exes["real"], Q)[0], Q).all()


def test_sanitized_build_agrees(exes, families):
    """The same program built with -fsanitize=address,undefined: clean, and
    the same verdicts."""
    for name in ("q50_luma", "q100_chroma", "q1_luma"):
        px, _, Q = families[name]
        a, b = Z.run_check(exes["real"], px, Q), Z.run_check(exes["san"], px, Q)
        assert a.summary == b.summary and np.array_equal(a.votes, b.votes), name
        assert np.array_equal(a.dec.view(np.uint32), b.dec.view(np.uint32)), name
    r = Z.run_check(exes["san"], np.zeros((0, 64), np.uint8), G.uniform(1))
    assert r.summary["blocks"] == 0


def test_threshold_family_sees_a_halved_constant(exes, families):
    """fdct_bfly.h with kZeroRowK halved passes rows that are not zero: on the
    family the check finds violations with it and none without."""
    seen = 0
    for name, (px, _, Q) in families.items():
        assert Z.run_check(exes["real"], px, Q).summary["violations"] == 0
        seen += Z.run_check(exes["mutant"], px, Q, expect_violations=True).summary["violations"] > 0
    assert seen >= len(families) // 2, seen

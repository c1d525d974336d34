"""K1's edge inputs (tests/fdctgen.py) on the host: the emulation of the fast
path (tools/diag/fdct_bfly_check.cpp, csrc/fdct_bfly.h) equals the reference
transform on every block it proves, in every family and at every table; the
fixture tests/golden/fdct_edges.npz is what its manifest says; the near ties
are all left to the exact path; and the threshold family tells two
deliberately wrong builds of the emulation from the real one, so a GPU build
that departs from fdct_bfly.h by as little is seen by
tests/test_gpu_fdct_edges.py, which compares K1's listing with the emulation's."""
import numpy as np
import pytest

import fdctgen as G


@pytest.fixture(scope="module")
def emus(tmp_path_factory):
    d = tmp_path_factory.mktemp("fdct_edges")
    exes = [G.build_emulation(d, m) for m in (0, 1, 2)]
    if exes[0] is None:
        pytest.skip("no C++ compiler")
    return exes


@pytest.fixture(scope="module")
def fix():
    return G.load_fixture()


@pytest.fixture(scope="module")
def tabs(oracle):
    return G.tables(oracle)


def test_emulation_equals_reference_on_every_family(emus, fix, tabs):
    """mismatches == 0 over every family and table (and Q = 1..255 over the
    pool), and the bound itself: the largest |t_fast - fl(Y_ref / Q)| /
    (A kb[row]) stays below 1.  Observed: 0.218, in the small-A family
    (DESIGN.md §4)."""
    worst, blocks = 0.0, 0
    runs = [(n,) + G.case(n, fix, tabs) for n in G.case_names()]
    pool = G.every_q_pool(fix)
    runs += [(f"every_q-{k}", pool, G.uniform(k)) for k in range(1, 256)]
    for name, px, Q in runs:
        e = G.emulate(emus[0], px, Q)
        assert e.summary["mismatches"] == 0, name
        assert e.summary["blocks"] == len(px) == len(e.ok) and e.summary["fixblocks"] == (~e.ok).sum(), name
        worst = max(worst, e.maxratio)
        blocks += len(px)
    print(f"\nlargest |t_fast - fl(Y_ref/Q)| / (A kb[row]) over {blocks} blocks: {worst:.4f}")
    assert 0.0 < worst < 1.0


def test_fixture_manifest(emus, fix, tabs):
    """The stored manifest is what a fresh emulation run finds, and it says
    what the families promise: every threshold block on the threshold, at
    least 64 listed and 64 proven per table, at uniform1 all 8 rows and all 8
    columns deciding on each side."""
    man = fix["manifest"]
    assert sorted(man) == sorted(G.TABLE_NAMES)
    for name in G.TABLE_NAMES:
        px = fix["threshold"][name]
        e = G.emulate(emus[0], px, tabs[name])
        flips = [(G.emulate(x, px, tabs[name]).ok != e.ok).sum() for x in emus[1:]]
        m = G.threshold_manifest(e, flips)
        assert m == man[name]["threshold"], name
        assert m["off_threshold"] == 0 and m["listed"] >= 64 and m["proven"] >= 64, (name, m)
        if name in G.TIE_TABLES:
            assert G.near_tie_manifest(G.emulate(emus[0], fix["near_tie"][name], tabs[name])) == man[name]["near_tie"]
    m = man["uniform1"]["threshold"]
    for k in ("rows_listed", "cols_listed", "rows_proven", "cols_proven"):
        assert m[k] == list(range(8)), k


def test_near_ties_are_all_left_to_the_exact_path(emus, fix, tabs):
    """Every block whose fl(Y_ref / Q) lies within 2^-18 of a half-integer is
    unproven: the searched AC near ties (tie at a row and a column other than
    0, within the margin of fdctgen.tie_margin_ok), and the flat blocks, which
    at a DC entry of 16 are ties for every odd offset from 128."""
    for name in G.TIE_TABLES:
        px = fix["near_tie"][name]
        e = G.emulate(emus[0], px, tabs[name])
        assert len(px) >= 32
        assert (e.tie <= G.TIE_WINDOW).all() and (e.tie_row != 0).all() and (e.tie_col != 0).all(), name
        assert G.tie_margin_ok(px, tabs[name], e.tie_row, e.tie).all(), name
        assert not e.ok.any(), name
    for dc in G.FLAT_TIE_DC:
        e = G.emulate(emus[0], G.flat_blocks(), G.uniform(dc))
        near = e.tie <= G.TIE_WINDOW
        assert not e.ok[near].any(), dc
        if dc == 16:
            assert near.sum() == 128 and near[1::2].all()
            assert ((e.tie_row == 0) & (e.tie_col == 0))[near].all()


@pytest.mark.parametrize("mutant", [1, 2])
def test_threshold_family_sees_each_mutant(emus, fix, tabs, mutant):
    """fdct_bfly.h with the FMA chains as separate multiplies and adds (1), and
    with kC4 = kC0 (2): on every table's threshold blocks the mutant lists a
    different set than the real emulation."""
    for name in G.TABLE_NAMES:
        px = fix["threshold"][name]
        real, mut = G.emulate(emus[0], px, tabs[name]), G.emulate(emus[mutant], px, tabs[name])
        assert (real.ok != mut.ok).sum() >= 1, name

"""K1 (k_fdct_quant and its exact path k_fdct_fix) on the edge inputs of
tests/fdctgen.py.

The forward DCT is bit-exact through two links: the host emulation of the fast
path (tools/diag/fdct_bfly_check.cpp, csrc/fdct_bfly.h) equals the reference
on every block it proves (tests/test_numerics.py, tests/test_fdct_edges.py),
and the gfx950 build of fdct_fast computes what the emulation computes.  The
second link is checked here: Codec.fdct_blocks_listed returns which blocks K1
listed for the exact path, the one GPU-observable quantity that follows the
fast path's arithmetic ulp for ulp, and it must equal the emulation's `!ok`
block for block, on blocks searched to sit on the decision's threshold.  Every
coefficient of every block is compared with the oracle's.  Then the lists
themselves: every slot of a unit, partial last units, full lists, both count
parities with stale entries behind them, and whole frames."""
import numpy as np
import pytest

import fdctgen as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expect(tmp_path_factory, oracle):
    """expect(px, Q) -> (the emulation's `!ok` per block, the oracle's
    coefficients in zig-zag order), kept per input so both kernel arrangements
    share one computation."""
    exe = G.build_emulation(tmp_path_factory.mktemp("fdct_gpu_edges"))
    assert exe, "no C++ compiler: the emulation is the reference of these tests"
    memo = {}

    def run(px, Q):
        px = np.ascontiguousarray(px, np.uint8).reshape(-1, 64)
        Q = np.ascontiguousarray(Q, np.float32)
        key = (px.tobytes(), Q.tobytes())
        if key not in memo:
            e = G.emulate(exe, px, Q)
            assert e.summary["mismatches"] == 0 and len(e.ok) == len(px)
            memo[key] = (~e.ok, np.stack([oracle.fdct_block(b, Q)[G.ZIGZAG] for b in px]))
        return memo[key]

    return run


@pytest.fixture(scope="module")
def fix():
    return G.load_fixture()


@pytest.fixture(scope="module")
def tabs(oracle):
    return G.tables(oracle)


def longest_list(listed):
    """Unit ua's blocks go to list ua % 32 (csrc/codec_common.hpp)."""
    per_unit = np.add.reduceat(listed.astype(np.int64), np.arange(0, len(listed), 16))
    return max(int(per_unit[c::32].sum()) for c in range(32))


def check(codec, expect, px, Q, tag=None):
    want_listed, want_coef = expect(px, Q)
    coef, listed, counts = codec.fdct_blocks_listed(px, Q)
    bad = np.flatnonzero(listed != want_listed)
    assert len(bad) == 0, (tag, "K1 lists other blocks than the emulation", bad[:8], want_listed[bad[:8]])
    assert counts == (int(want_listed.sum()), longest_list(want_listed)), tag
    bad = np.flatnonzero((coef != want_coef).any(1))
    assert len(bad) == 0, (tag, "coefficients differ from the oracle's", bad[:8])
    return want_listed, counts


@pytest.mark.parametrize("name", G.case_names())
def test_listed_set_equals_emulation(codec, expect, fix, tabs, name):
    """Every family at every table: listed == the emulation's !ok block for
    block, and every block's coefficients == the oracle's."""
    px, Q = G.case(name, fix, tabs)
    want, _ = check(codec, expect, px, Q, name)
    if name.startswith("threshold"):
        assert want.sum() >= 64 and (~want).sum() >= 64
    if name.startswith("near_tie"):
        assert want.all()


def test_listed_set_equals_emulation_at_every_q(codec, expect, fix):
    """Uniform tables Q = 1..255 over a pool of 64 blocks from the families."""
    pool = G.every_q_pool(fix)
    for k in range(1, 256):
        check(codec, expect, pool, G.uniform(k), k)


Q16 = G.uniform(16)


def all_listed(n):
    return np.tile(G.LISTED_BLOCK, (n, 1))


def test_unit_slots(codec, expect):
    """One listed block at each slot 0..15 of a unit among proven ones (unit u
    lists its slot u), and a unit with all 16 listed."""
    px = np.tile(G.PROVEN_BLOCK, (256, 1))
    px[np.arange(16) * 16 + np.arange(16)] = G.LISTED_BLOCK
    want, counts = check(codec, expect, px, Q16)
    assert np.array_equal(np.flatnonzero(want), np.arange(16) * 17) and counts == (16, 1)
    want, counts = check(codec, expect, all_listed(16), Q16)
    assert want.all() and counts == (16, 16)


@pytest.mark.parametrize("nblocks", [1, 15, 17, 31])
@pytest.mark.parametrize("last_listed", [True, False])
def test_partial_last_unit(codec, expect, nblocks, last_listed):
    """nblocks % 16 in {1, 15}: the last live block listed, and proven; the
    dead lanes of the last unit (which reload its last block) add nothing."""
    px = np.tile(G.PROVEN_BLOCK, (nblocks, 1))
    px[::3] = G.LISTED_BLOCK
    px[-1] = G.LISTED_BLOCK if last_listed else G.PROVEN_BLOCK
    want, counts = check(codec, expect, px, Q16)
    assert want[-1] == last_listed and counts[0] == want.sum()


@pytest.mark.parametrize("units", [1, 31, 32, 33, 64, 65])
def test_full_lists(codec, expect, units):
    """Every block of every unit listed: each list that has units is filled
    to the last entry of its capacity, 16 * ceil(units / 32)."""
    want, counts = check(codec, expect, all_listed(16 * units), Q16)
    assert want.all() and counts == (16 * units, G.fix_list_cap(units))
    if units % 32 == 1:  # the last unit alone in its list's last 16 entries: one block short
        _, counts = check(codec, expect, all_listed(16 * units - 1), Q16)
        assert counts == (16 * units - 1, G.fix_list_cap(units) - 1)


def test_parity_and_stale_lists(codec, expect, fix, tabs):
    """Launches of different lengths on one context alternate between two sets
    of counts, and a shorter launch's lists lie inside what a longer one left
    behind: an all-listed 65-unit launch, a none-listed one, an all-listed
    3-unit one and a mixed one, each right; then the same starting from the
    other parity."""
    mixed = fix["threshold"]["uniform1"]
    none = np.tile(G.PROVEN_BLOCK, (16 * 40 + 5, 1))
    for start in range(2):
        want, counts = check(codec, expect, all_listed(16 * 65), Q16, (start, "65 units"))
        assert counts == (16 * 65, 48)
        want, counts = check(codec, expect, none, Q16, (start, "none"))
        assert counts == (0, 0)
        want, counts = check(codec, expect, all_listed(16 * 3), Q16, (start, "3 units"))
        assert counts == (48, 16)
        want, counts = check(codec, expect, mixed, tabs["uniform1"], (start, "mixed"))
        assert 0 < counts[0] < len(mixed)
        if start == 0:  # an odd number of launches in between: the other parity next
            check(codec, expect, none[:16], Q16, "flip")


# ---- frames ---------------------------------------------------------------
W, H = 256, 128  # 32 + 8 + 8 units per frame: ua % 32 wraps inside a frame and across frames


def frame(y, u, v):
    return np.concatenate([G.plane_from_blocks(y, W, H).ravel(), G.plane_from_blocks(u, W // 2, H // 2).ravel(),
                           G.plane_from_blocks(v, W // 2, H // 2).ravel()]).tobytes()


@pytest.fixture(scope="module")
def frames(expect, oracle, fix, tabs):
    """{name: (frame bytes, q)}: luma all listed next to proven chroma and the
    reverse (flat blocks at odd offsets from 128 under a DC entry of 16: q50
    luma, and the chroma quality whose DC entry is 16), and a frame of
    threshold and near-tie blocks at q50."""
    qc = next(q for q in range(1, 101) if oracle.qtable(q, 1)[0] == 16)
    assert oracle.qtable(50, 0)[0] == 16
    flat = G.flat_blocks()
    odd, even = flat[1::2], flat[0::2]
    luma, chroma = oracle.qtable(50, 0), oracle.qtable(qc, 1)
    assert expect(odd, luma)[0].all() and expect(odd, chroma)[0].all()
    assert not expect(even, luma)[0].any() and not expect(even, chroma)[0].any()
    fam_y = np.concatenate([fix["threshold"]["q50_luma"], fix["near_tie"]["q50_luma"]])
    fam_c = fix["threshold"]["q50_chroma"]
    return {"luma_listed": (frame(odd, even, even[::-1]), (50, qc, qc)),
            "chroma_listed": (frame(even, odd, odd[::-1]), (50, qc, qc)),
            "family": (frame(fam_y, fam_c, fam_c[::-1]), (50, 50, 50))}


def check_frames(enc, oracle, frames):
    for name, (fr, q) in frames.items():
        assert enc.compress(fr, W, H, q) == oracle.compress(fr, W, H, q), name
    q = frames["luma_listed"][1]
    for order in (("luma_listed", "chroma_listed"), ("chroma_listed", "luma_listed")):
        batch = [frames[n][0] for n in order]
        assert enc.compress_batch(batch, W, H, q) == [oracle.compress(f, W, H, q) for f in batch], order


def test_frames(codec, oracle, frames):
    """Whole planes listed next to whole planes proven, single frames and
    2-frame batches in both orders, against the oracle's streams."""
    check_frames(codec, oracle, frames)


def test_frames_fused_encoder(fused_encoder, oracle, frames):
    """The same through k_encode_tile, whose fdct_fast<false> sends a whole
    unit to the exact path when any of its blocks is unproven."""
    check_frames(fused_encoder, oracle, frames)

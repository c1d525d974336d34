"""Coefficient-domain inputs (tests/coefgen.py) on the CPU: the generators do
what they say, the stream builder's payloads decode to the per-block inverse
transform, and the oracle's block coder and decoder equal the REFERENCE's own
(Huffman::fromData / dump, YUV::decompress) on every crafted block and
stream the GPU tests use, not only on what pixel frames produce.  The
reference-side tests skip when oracle/_ref is not built."""
import numpy as np
import pytest

import blockgen
import coefgen


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as R

    if not R.available("serial"):
        pytest.skip("oracle/_ref not built (needs /root/reference; `make -C oracle ref`)")
    return R


@pytest.fixture(scope="module")
def ref_coder(ref):
    """The reference's block coder through ref_harness.cpp.  build() makes
    oracle/_ref from this tree's harness wherever the reference's sources are
    (and fails if the entry point is missing then); an oracle/_ref that was
    brought along from an older harness, on a machine that cannot rebuild it,
    counts as not built."""
    if not ref.has("ref_huff_encode_block", "serial"):
        pytest.skip("oracle/_ref predates ref_huff_encode_block (ref_harness.cpp); `make -C oracle ref` rebuilds it")
    return ref


@pytest.fixture(scope="module")
def sh(oracle):
    return coefgen.shared(oracle)


def k2_and_gate_blocks():
    """Every distinct block of the K2 and gate families (sections 3 and 4)."""
    out = [b for _, b in coefgen.class_bucket_blocks()]
    out += list(coefgen.dc_blocks())
    for _, case in coefgen.window_cases(1024) + coefgen.shape_cases(256):
        out += list(case.pool)
    for pool in coefgen.gate_pools():
        out += list(pool)
    return out


# ---------------------------------------------------------------- generators
def test_block_generator_meets_its_parameters():
    rng = np.random.default_rng(1)
    n = 0
    for nub in range(0, 65):
        for msz in (0, 1, 2, 5, nub, nub + 1, 33, 64):
            for zi in (False, True):
                for d in (0, 1, 2, 8, 9, nub - 1, nub):
                    try:
                        b = coefgen.block(nub, d, msz, zi, rng)
                    except ValueError:
                        continue
                    assert coefgen.describe(b) == (nub, d, msz), (nub, d, msz, zi)
                    nnz = int(np.count_nonzero(b))
                    assert (msz > nnz) == zi and not b[msz:].any()
                    n += 1
    assert n > 500


@pytest.mark.parametrize("args", [(3, 2, 2, False),    # without a zero inside, msz = nub
                                  (3, 3, 2, True),     # a zero inside needs msz > nnz
                                  (1, 1, 1, True),     # nnz would be 0
                                  (5, 6, 5, False),    # more distinct values than coefficients
                                  (5, 1, 9, True),     # the zero inside is a symbol: distinct >= 2
                                  (0, 1, 0, False),    # the all-zero block has no symbol in its message
                                  (65, 3, 64, False)])
def test_block_generator_refuses_impossible_combinations(args):
    with pytest.raises(ValueError):
        coefgen.block(*args, np.random.default_rng(0))


def test_families_cover_the_boundaries_they_name():
    """The class / bucket family has, on both sides, every boundary the K2
    tests are about; the gate pools are what their names say."""
    desc = [coefgen.describe(b) for _, b in coefgen.class_bucket_blocks()]
    nubs = {d[0] for d in desc}
    assert {2, 4, 5, 8, 9, 15, 16, 17, 40, 64} <= nubs
    assert {0, 1, 2, 6, 7, 12, 13, 20, 21, 63, 64} <= {d[2] for d in desc}
    r8x = {d[1] for d in desc if 9 <= d[0] <= 15}
    assert {8, 9} <= r8x
    assert {2, 8, 9, 16, 17, 33, 64} <= {d[1] for d in desc if d[0] >= 16}
    names = [n for n, _ in coefgen.class_bucket_blocks()]
    assert any(n.endswith("_z_0") for n in names) and any(n.endswith("_n_0") for n in names)
    # every sort key has a pool, and each window case the length it says
    assert len(coefgen.sort_keys()) == 1 + 4 + 4 + 3 + 1
    for name, case in coefgen.window_cases(1024):
        assert len(case.idx) in (64, 1024, 1024 + 65), name
    free, low, high = coefgen.gate_pools()
    assert {coefgen.klass(b) for b in free} == {"single", "r4", "r8"}
    assert {coefgen.klass(b) for b in low} == {"r8x", "ovf"}
    assert min(coefgen.describe(b)[1] for b in high) == 17 and max(coefgen.describe(b)[1] for b in low) == 16
    c = coefgen.gate_case(1000, 300, 120, seed=3)
    assert c.counts() == (300, 120) and len(c.idx) == 1000


def test_stream_names_are_the_streams(sh):
    assert coefgen.stream_names() == [s.name for s in coefgen.decoder_streams(sh._oracle, sh.chunks)]
    assert len(set(coefgen.stream_names())) == len(coefgen.stream_names())


def test_stage_boundary_groups_have_their_totals(sh):
    by = coefgen.sized_pool(sh.chunks)
    groups = coefgen.stage_boundary_groups(sh.chunks, by)
    totals = {name: sum(len(sh.chunks.one(b)) for b in g) for name, g in groups}
    for t in (5119, 5120, 5121):
        assert totals[f"total_{t}"] == t
    longest = max(by)
    assert 130 <= longest <= coefgen.MAX_CHUNK
    assert totals["all_longest"] == 64 * longest
    for lane in (0, 63):
        g = dict(groups)[f"longest_at_lane{lane}"]
        assert [len(sh.chunks.one(b)) == longest for b in g] == [i == lane for i in range(64)]
        assert all(coefgen.describe(b)[1] == 4 for i, b in enumerate(g) if i != lane)


def test_group_composition_counts(oracle):
    g = coefgen.group_composition_blocks(oracle.qtable(50, 0)).reshape(-1, 64, 64)
    ks = [int((x[:, 1:] != 0).any(axis=1).sum()) for x in g]
    assert ks == [k for k in coefgen.GROUP_K for _ in range(3)]
    for x, k in zip(g[0::3], coefgen.GROUP_K):  # "first": lanes 0 .. k-1
        assert (x[:k, 1:] != 0).any(axis=1).all()
    for x, k in zip(g[1::3], coefgen.GROUP_K):  # "last"
        assert (x[64 - k:, 1:] != 0).any(axis=1).all()


# ------------------------------------------------- the builder's self-check
@pytest.mark.parametrize("name", coefgen.stream_names() + ["batch_0", "batch_1"])
def test_built_stream_decodes_to_the_block_composition(oracle, sh, name):
    """The payload assembled from the oracle's chunks decodes, through the
    oracle's stream parser, to oracle.idct_block of every block at its place;
    the in-range streams stay a test of arithmetic (at most 10 % of the pixels
    clamp), the extreme ones a test of the clamp (at least 90 %)."""
    s = sh.by_name[name]
    pay, dec = sh.decoded(name)
    assert dec == coefgen.compose(s.planes, s.w, s.h, s.q, oracle)
    if s.kind == "in_range":
        assert coefgen.saturated_fraction(dec) <= 0.10
    if s.kind == "extreme":
        assert coefgen.saturated_fraction(dec) >= 0.90


def test_payload_layout_is_the_encoders(oracle):
    """build_payload over a frame's own coefficient blocks reproduces
    oracle.compress byte for byte (header, size table and chunk order)."""
    w, h, q = 48, 32, (35, 60, 85)
    rng = np.random.default_rng(12)
    fr = rng.integers(0, 256, w * h * 3 // 2).astype(np.uint8)
    planes, off = [], 0
    for p, n in enumerate(coefgen.plane_counts(w, h)):
        pw, ph = (w, h) if p == 0 else (w // 2, h // 2)
        px = fr[off:off + pw * ph].reshape(ph // 8, 8, pw // 8, 8).transpose(0, 2, 1, 3).reshape(n, 64)
        Q = oracle.qtable(q[p], p != 0)
        planes.append(np.stack([oracle.fdct_block(b, Q)[coefgen.ZZ] for b in px]))
        off += pw * ph
    assert coefgen.build_payload(planes, oracle) == oracle.compress(fr.tobytes(), w, h, q)


# ------------------------------------------------------- the reference pins
def test_oracle_chunks_equal_the_references_on_crafted_blocks(oracle, ref_coder, sh):
    """oracle.huff_encode_block == the reference's Huffman::fromData(x).dump()
    for every block of the K2, gate and decoder families and of
    blockgen.edge_blocks(), the same 64 values in the same (natural) order."""
    blocks = k2_and_gate_blocks() + [b for _, b in blockgen.edge_blocks()]
    for s in sh.streams:
        for p in s.planes:
            blocks += list(p)
    seen = set()
    for b in blocks:
        b = np.ascontiguousarray(b, np.int16)
        if b.tobytes() in seen:
            continue
        seen.add(b.tobytes())
        nat = coefgen.natural(b)
        assert oracle.huff_encode_block(nat) == ref_coder.huff_encode_block(nat), coefgen.describe(b)
    assert len(seen) > 4000


@pytest.mark.parametrize("name", coefgen.stream_names() + ["batch_0", "batch_1"])
def test_reference_decodes_built_streams_as_the_oracle(ref, sh, name):
    s = sh.by_name[name]
    pay, dec = sh.decoded(name)
    assert ref.decompress(pay, s.w, s.h, s.q, variant="serial") == dec

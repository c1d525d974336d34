"""K2, its overflow tiers and the decoder on coefficient-domain inputs
(tests/coefgen.py): blocks crafted to K2's own class, bucket, window and run
boundaries; block lists whose overflow-list lengths sit exactly at the regime
switches of the overflow passes; DCTYUV streams assembled from the oracle's
chunks that no pixel frame produces.  Every chunk is compared with the
oracle's (pinned to the reference's own coder on the same blocks by
tests/test_coef_domain.py), every decoded frame with the oracle's decode."""
import numpy as np
import pytest

import coefgen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def consts():
    import myyuv_hip
    k = myyuv_hip.k2_constants()
    # the families are drawn up against these two; a retuned value must fail
    # here, not silently move every case to another class
    assert k["ovf_nub"] == coefgen.OVF_NUB
    assert k["window_blocks"] % k["k2_group"] == 0
    return k


@pytest.fixture(scope="module")
def sh(oracle):
    return coefgen.shared(oracle)


def tier_counts(case, consts, nframes=1):
    """(work[0], work[1]) the launch must report: what K2 lists, and what the
    CAP-16 tier lists again, which runs only past its gate."""
    n_ovf, n17 = case.counts(consts["ovf_nub"])
    gate = consts["r16_gate_single"] if nframes == 1 else consts["r16_gate"]
    runs = len(case.idx) > gate and n_ovf > gate
    return n_ovf, n17 if runs else 0


def check_k2(codec, sh, consts, name, case, nframes=1, want=None):
    """The case through K2 and its overflow passes, twice on the same context
    (nothing may depend on a fresh workspace): every chunk and size equals the
    oracle's, the two list lengths what the case was designed to, and the
    chunk bytes booked in the tiles' info words the listed and the other
    blocks' sizes (a block two passes encode has the right chunk, but is
    booked twice and would shift every later chunk of a stream)."""
    exp_c, exp_s = case.expected(sh.chunks)
    coefs = case.blocks
    lm = case.listed_mask(consts["ovf_nub"])
    booked = (int(exp_s[lm].sum()), int(exp_s[~lm].sum()))
    for rep in range(2):
        got_c, got_s, cnt = codec.huff_encode_blocks_counted(coefs, nframes)
        bad = np.nonzero((got_s != exp_s) | (got_c != exp_c).any(axis=1))[0]
        assert len(bad) == 0, (name, rep, len(bad), bad[:8].tolist(), coefgen.describe(coefs[bad[0]]),
                               int(got_s[bad[0]]), int(exp_s[bad[0]]))
        assert cnt[:2] == (want or tier_counts(case, consts, nframes)), (name, rep)
        assert cnt[2:] == booked, (name, rep)


# ------------------------------------------------------------- K2 structure
def test_classes_and_length_buckets(codec, oracle, sh, consts):
    """nub on both sides of 4/5, 8/9, 15/16, msz on both sides of 6/7, 12/13,
    20/21, distinct on both sides of 8 and 16 (r8x blocks that build and that
    go to the worklist), with and without a zero inside the message; through
    the public entry point and the oracle's natural-order call."""
    named = coefgen.class_bucket_blocks()
    blocks = np.stack([b for _, b in named])
    got = codec.huff_encode_blocks(blocks)
    for (name, b), ch in zip(named, got):
        assert ch == oracle.huff_encode_block(coefgen.natural(b)), name
    check_k2(codec, sh, consts, "class_bucket", coefgen.Case(blocks))


def test_single_class_every_dc(codec, sh, consts):
    """msz = 1 for every DC in -1024..1023: build_single_dc works from the 11
    bits of the DC kept in the block word."""
    check_k2(codec, sh, consts, "every_dc", coefgen.Case(coefgen.dc_blocks()), want=(0, 0))


@pytest.fixture(scope="module")
def windows(consts):
    return coefgen.window_cases(consts["window_blocks"])


@pytest.mark.parametrize("prefix", ["whole_", "63_of_", "64_of_", "65_of_", "interleaved", "63_single_one_r8x"])
def test_window_composition(codec, sh, consts, windows, prefix):
    """One window of one sort key, for each key; each key with 63, 64 and 65
    blocks in an otherwise all-zero window (a run that straddles two keys or
    ends exactly on one); the classes interleaved by position; 63 single-class
    blocks under one r8x block's msz of 64."""
    cases = [(n, c) for n, c in windows if n.startswith(prefix)]
    assert cases
    for name, case in cases:
        check_k2(codec, sh, consts, name, case)


def test_shape_edges(codec, sh, consts):
    """Block counts around the run, the tile and the window: partial tiles and
    1, 2 or 3 tiles in the last window."""
    for name, case in coefgen.shape_cases(consts["k2_group"]):
        check_k2(codec, sh, consts, name, case)


# ----------------------------------------------------------- regime switches
GATE_CASES = [c[0] for c in coefgen.single_frame_gate_cases(0, 0)]


@pytest.fixture(scope="module")
def gate_pools():
    return coefgen.gate_pools()


@pytest.mark.parametrize("name", GATE_CASES)
def test_single_frame_gates(codec, sh, consts, gate_pools, name):
    """The single-frame list lengths at which launch_overflow, the CAP-16 tier,
    the wave pass and the lane pass hand over to one another (each compares
    the length with its gate or limit on its own): exactly kR16GateSingle and
    one more, with the tier's list empty, full, and at kWaveEncodeLimit and one
    more.  Both list lengths are asserted, so a retuned constant fails here."""
    gate, limit = consts["r16_gate_single"], consts["wave_encode_limit"]
    assert gate < limit
    row = {c[0]: c for c in coefgen.single_frame_gate_cases(gate, limit)}[name]
    _, nblk, n_ovf, n17 = row
    case = coefgen.gate_case(nblk, n_ovf, n17, seed=GATE_CASES.index(name), pools=gate_pools)
    assert case.counts(consts["ovf_nub"]) == (n_ovf, n17)
    tier_runs = nblk > gate and n_ovf > gate
    assert tier_runs == (name[0] in "defg")
    check_k2(codec, sh, consts, name, case, want=(n_ovf, n17 if tier_runs else 0))


@pytest.mark.parametrize("name", ["short_list", "at_gate", "past_gate"])
def test_batch_gates(codec, sh, consts, gate_pools, name):
    """Two-frame launches (the block-level entry point with nframes = 2): a
    list of one block goes to the lane pass (kBatchWaveLimit = 0: no wave
    pass for batches); lists of exactly kR16Gate blocks and one more, in a
    batch of more than kR16Gate blocks, on either side of the CAP-16 tier."""
    gate = consts["r16_gate"]
    assert consts["batch_wave_limit"] == 0
    per = (gate + 2 + 350) // 2
    nblk, n_ovf, n17 = {"short_list": (2 * 300 + 2, 1, 1), "at_gate": (2 * per, gate, gate // 2),
                        "past_gate": (2 * per, gate + 1, gate // 2)}[name]
    assert name == "short_list" or nblk > gate + 1
    case = coefgen.gate_case(nblk, n_ovf, n17, seed=40 + len(name), pools=gate_pools)
    check_k2(codec, sh, consts, name, case, nframes=2, want=(n_ovf, n17 if n_ovf > gate else 0))


# ------------------------------------------------------------------ decoder
def first_difference(got, want, s):
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if len(a) != len(b):
        return ("size", len(a), len(b))
    d = np.nonzero(a != b)[0]
    return (s.name, len(d), int(d[0]), int(a[d[0]]), int(b[d[0]])) if len(d) else None


@pytest.mark.parametrize("name", coefgen.stream_names())
def test_decoder_on_built_streams(codec, sh, name):
    """DC-only blocks at every DC (luma and chroma, five qualities); one
    coefficient at each position and magnitude; 64-block groups with exactly k
    blocks for the transform units; groups at the chunk stage's byte
    boundaries; all-extreme and in-range magnitudes; small and ragged
    geometries.  The oracle's decode saturates at most 10 % of the in-range
    streams' pixels and at least 90 % of the extreme ones'."""
    s = sh.by_name[name]
    pay, want = sh.decoded(name)
    if s.kind == "in_range":
        assert coefgen.saturated_fraction(want) <= 0.10
    if s.kind == "extreme":
        assert coefgen.saturated_fraction(want) >= 0.90
    for rep in range(2):
        got = codec.decompress(pay, s.w, s.h, s.q)
        assert first_difference(got, want, s) is None, rep


def test_decoder_two_frame_batch_of_different_streams(codec, sh):
    """One 2-frame decompress_batch_device call over two different built
    streams of one geometry."""
    import torch
    a, b = sh.by_name["batch_0"], sh.by_name["batch_1"]
    pays = [sh.decoded(s.name)[0] for s in (a, b)]
    assert pays[0] != pays[1]
    w, h, q = a.w, a.h, a.q
    fb = w * h * 3 // 2
    cap = (max(len(p) for p in pays) + 3) & ~3
    dev = torch.device("cuda", 0)
    host = np.zeros(2 * cap, np.uint8)
    for i, p in enumerate(pays):
        host[i * cap:i * cap + len(p)] = np.frombuffer(p, np.uint8)
    d_pay = torch.from_numpy(host).to(dev)
    d_sz = torch.tensor([len(p) for p in pays], dtype=torch.int32, device=dev)
    d_out = torch.zeros(2 * fb, dtype=torch.uint8, device=dev)
    sp = torch.cuda.current_stream(dev).cuda_stream
    codec.reserve_batch(w, h, 2)
    codec.decompress_batch_device(d_pay.data_ptr(), d_sz.data_ptr(), cap, 2, w, h, q, d_out.data_ptr(), sp)
    rc, bad = codec.sync_status(sp)
    assert rc == 0, (rc, bad)
    out = d_out.cpu().numpy()
    for i, s in enumerate((a, b)):
        assert first_difference(out[i * fb:(i + 1) * fb].tobytes(), sh.decoded(s.name)[1], s) is None, i

"""K1's zero-row skip on the GPU (csrc/xform_common.hpp fdct_fast, csrc/
fdct_bfly.h "Zero rows"): a wave whose storing blocks all pass the rule for
rows 4..7 leaves those rows' stage 2, packing, counts and store out.  The skip
is not observable by itself (a skipped row is a row of zeros that the full
path would have produced too), so every case first asserts on the CPU, through
the shared host rule (tests/zerorows.py), which 16-block units qualify: a case
cannot pass because the skip never fired, or always did.  Then, as
tests/test_gpu_fdct_edges.py: every coefficient equals the oracle's and K1's
listing equals the emulation's block for block.  Whole streams, through every
kernel that shares the transform, are compared with the oracle's bytes.

(K1's lanes past the plane's end re-read the plane's last block, so in K1 a
dead slot votes as the last live block would; they are still kept out of the
vote, which the BMP and downscale kernels need: their dead slots hold other
pixels.)"""
import numpy as np
import pytest

import fdctgen as G
import zerorows as Z
from test_gpu_fdct_edges import check, expect  # noqa: F401  (expect: the emulation + oracle fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    exe = Z.build_check(tmp_path_factory.mktemp("fdct_gpu_zero_rows"))
    assert exe, "no C++ compiler: the host rule is the reference of these tests"
    return exe


@pytest.fixture(scope="module")
def q50(oracle):
    return oracle.qtable(50, 0)


def run(codec, expect, rule, px, Q, want_skip, tag=None, tested=True):
    """The units that qualify are `want_skip` (host rule) and the table's
    planes are tested at all or not (`tested`: fdct_bfly.h's gate; where not,
    no wave skips and the case checks that nothing else changed), then the
    edge tests' check in calls of at most 64 blocks (whole units)."""
    px = np.ascontiguousarray(px, np.uint8).reshape(-1, 64)
    skip = Z.units_skip(Z.qualifies(rule, px, Q))
    assert np.array_equal(skip, np.asarray(want_skip, bool)), (tag, skip)
    assert Z.tested(rule, Q) == tested, tag
    for i in range(0, len(px), 64):
        check(codec, expect, px[i:i + 64], Q, (tag, i))


def spoiler(oracle, rule, Q, f):
    """A block of level 128 whose only nonzero coefficient (the oracle's) lies
    in row f, and which the rule fails in row f alone."""
    v = Z.largest_reciprocal_column(Q, f)
    for amp in np.arange(1.0, 140.0, 0.5):
        b = Z.pattern_block(128, amp, f, v)
        nz = np.flatnonzero(oracle.fdct_block(b, Q))
        if len(nz) and (nz // 8 == f).all():
            assert Z.run_check(rule, b, Q).votes[0] == 15 & ~(1 << (f - 4)), (f, amp)
            return b
        assert len(nz) == 0, (f, amp, nz)
    raise AssertionError(f)


def gentle(n):
    """n qualifying blocks that are not flat: low-frequency patterns (rows 0..3 of T)."""
    return np.stack([Z.pattern_block(100 + 3 * i, 20 + i, 1 + i % 3, i % 4) for i in range(n)])


def test_all_qualify_next_to_none(codec, expect, rule, oracle, q50):
    sp = np.stack([spoiler(oracle, rule, q50, 4 + i % 4) for i in range(16)])
    run(codec, expect, rule, np.concatenate([gentle(16), sp, sp, gentle(16)]), q50, [True, False, False, True])


@pytest.mark.parametrize("f", [4, 5, 6, 7])
def test_one_spoiler_in_a_qualifying_unit(codec, expect, rule, oracle, q50, f):
    """The spoiler's one nonzero coefficient in row f (lane f - 4's second
    row), at slot 0, 7 and 15 of its unit; a clean unit last."""
    px = np.tile(gentle(16), (4, 1))
    for u, slot in enumerate((0, 7, 15)):
        px[16 * u + slot] = spoiler(oracle, rule, q50, f)
    run(codec, expect, rule, px, q50, [False, False, False, True], f)


@pytest.mark.parametrize("table", ["q50_luma", "q90_chroma", "q10_luma"])
def test_threshold_family(codec, expect, rule, oracle, table):
    """The CPU test's family: the 32 passing and 32 failing blocks nearest to
    the threshold as they come, and then one at a time in a unit of flat
    blocks, where the block just above the threshold alone stops the skip."""
    Q = Z.quality_tables(oracle)[table]
    px, fs = Z.threshold_family(rule, Q)
    r = Z.run_check(rule, px, Q)
    dec = r.dec[np.arange(len(px)), fs - 4]
    qual = r.votes == 15
    below = np.flatnonzero(qual)[np.argsort(0.5 - dec[qual])[:32]]
    above = np.flatnonzero(dec >= 0.5)[np.argsort(dec[dec >= 0.5])[:32]]
    assert len(below) == 32 and len(above) == 32 and (dec[below] > 0.4).all() and (dec[above] < 0.6).all()
    run(codec, expect, rule, np.concatenate([px[below], px[above]]), Q, [True, True, False, False], table)
    units, want = [], []
    for n, i in enumerate(np.concatenate([above[:4], below[:4]])):
        u = Z.flat(128 + n, 16)
        u[(5 * n) % 16] = px[i]
        units.append(u)
        want.append(n >= 4)
    run(codec, expect, rule, np.concatenate(units), Q, want, (table, "alone"))


@pytest.mark.parametrize("live", [1, 8, 15])
def test_partial_last_unit(codec, expect, rule, oracle, q50, live):
    """A last unit of 1, 8 and 15 live blocks that all qualify, alone and after
    a unit that does not; and with a live spoiler in its last slot."""
    sp = spoiler(oracle, rule, q50, 5)
    run(codec, expect, rule, gentle(live), q50, [True], live)
    run(codec, expect, rule, np.concatenate([np.tile(sp, (16, 1)), gentle(live)]), q50, [False, True], live)
    px = gentle(live)
    px[-1] = sp
    run(codec, expect, rule, np.concatenate([gentle(16), px]), q50, [True, False], live)


@pytest.mark.parametrize("q", [1, 50, 90, 100])
@pytest.mark.parametrize("chroma", [0, 1])
def test_quality_tables(codec, expect, rule, oracle, q, chroma):
    """Per table: a flat unit, a unit of the passing blocks nearest to the
    threshold, a unit of the failing ones.  Luma at q90 and both tables at
    q100 have a row-4 entry below 6: their planes are not tested."""
    Q = oracle.qtable(q, chroma)
    tested = q <= 50 or (chroma == 1 and q == 90)
    px, fs = Z.threshold_family(rule, Q)
    r = Z.run_check(rule, px, Q)
    dec = r.dec[np.arange(len(px)), fs - 4]
    qual = r.votes == 15
    below = np.flatnonzero(qual)[np.argsort(0.5 - dec[qual])[:16]]
    above = np.flatnonzero(dec >= 0.5)[np.argsort(dec[dec >= 0.5])[:16]]
    assert len(below) == 16 and len(above) == 16
    run(codec, expect, rule, np.concatenate([G.flat_blocks()[5::16], px[below], px[above]]), Q, [True, True, False],
        (q, chroma), tested)


def test_all_flat(codec, expect, rule, q50):
    """Every unit skips: the hi store never issues."""
    run(codec, expect, rule, G.flat_blocks()[::4], q50, [True] * 4)
    run(codec, expect, rule, G.flat_blocks()[3::4], G.uniform(7), [True] * 4)
    run(codec, expect, rule, G.flat_blocks()[3::4], G.uniform(1), [True] * 4, tested=False)


# ---- whole streams ----------------------------------------------------------
# 16x16: one luma block row, a chroma unit of one live block.  144x32: 18
# blocks per luma row and 9 per chroma row, so the 16-block units wrap the
# block rows and every plane ends in a partial unit (8 and 2 live blocks).
GEOMS = [(16, 16), (144, 32)]
Q50 = (50, 50, 50)


@pytest.fixture(scope="module")
def content(oracle, rule):
    """Blocks of the cases above, cycled over the planes: runs of qualifying
    blocks longer than a unit, spoilers, and threshold blocks of both sides."""
    Q = oracle.qtable(50, 0)
    px, fs = Z.threshold_family(rule, Q)
    dec = Z.run_check(rule, px, Q).dec[np.arange(len(px)), fs - 4]
    near = px[np.argsort(np.abs(dec - 0.5))[:12]]
    sp = np.stack([spoiler(oracle, rule, Q, f) for f in (4, 5, 6, 7)])
    return np.concatenate([gentle(20), sp[:1], Z.flat(131, 17), near, gentle(19), sp[1:], Z.flat(7, 3)])


def iyuv(content, w, h, shift=0):
    planes = [G.plane_from_blocks(np.roll(content, -(shift + 5 * i), 0), pw, ph)
              for i, (pw, ph) in enumerate(((w, h), (w // 2, h // 2), (w // 2, h // 2)))]
    return np.concatenate([p.ravel() for p in planes]).tobytes()


def assert_both_kinds(rule, oracle, frame, w, h):
    """The frame's luma units: some skip and some do not (for 16x16, four
    blocks, at least the rule's verdicts differ or the unit skips)."""
    y = G.plane_blocks(np.frombuffer(frame, np.uint8)[: w * h].reshape(h, w))
    skip = Z.units_skip(Z.qualifies(rule, y, oracle.qtable(50, 0)))
    if len(skip) > 1:
        assert skip.any() and not skip.all(), skip
    return skip


def device_payloads(codec, frames, w, h, q):
    import torch
    import myyuv_hip

    n = len(frames)
    cap = (myyuv_hip.payload_bound(w, h) + 3) & ~3
    d_in = torch.frombuffer(bytearray(b"".join(frames)), dtype=torch.uint8).cuda()
    d_pay = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if n == 1:
        codec.compress_device(d_in.data_ptr(), w, h, q, d_pay.data_ptr(), cap, d_sizes.data_ptr(), stream)
    else:
        codec.reserve_batch(w, h, n)
        codec.compress_batch_device(d_in.data_ptr(), n, w, h, q, d_pay.data_ptr(), cap, d_sizes.data_ptr(), stream)
    rc, bad = codec.sync_status(stream)
    assert rc == 0, (rc, bad)
    sizes = d_sizes.cpu().tolist()
    pay = d_pay.cpu().numpy()
    return [pay[i * cap:i * cap + sizes[i]].tobytes() for i in range(n)]


@pytest.mark.parametrize("w,h", GEOMS)
def test_streams_compress_device(codec, oracle, rule, content, w, h):
    """One frame through compress_device and a 3-frame batch, byte for byte."""
    frames = [iyuv(content, w, h, s) for s in (0, 23, 41)]
    for fr in frames:
        assert_both_kinds(rule, oracle, fr, w, h)
    want = [oracle.compress(fr, w, h, Q50) for fr in frames]
    assert device_payloads(codec, frames[:1], w, h, Q50) == want[:1]
    assert device_payloads(codec, frames, w, h, Q50) == want


@pytest.mark.parametrize("w,h", GEOMS)
def test_streams_fused_encoder(fused_encoder, oracle, content, w, h):
    """k_encode_tile shares fdct_core and pack_quads."""
    for s in (0, 23):
        fr = iyuv(content, w, h, s)
        assert fused_encoder.compress(fr, w, h, Q50) == oracle.compress(fr, w, h, Q50), s


def test_stream_compress_bmp_device(codec, oracle, rule, content):
    """k_bmp_fdct: a grey 144x32 BGRA picture of the content (its luma units
    qualify in part, by the rule on the oracle's own conversion); a strip
    narrower than a unit leaves dead slots of pixel 128."""
    import torch
    import myyuv_hip

    w, h = 144, 32
    grey = G.plane_from_blocks(content, w, h)
    bmp = np.repeat(grey[:, :, None], 4, 2).copy()
    bmp[..., 3] = 255
    data = bmp.tobytes()
    fr = oracle.bmp_to_iyuv(data, w, -h, 32)
    assert_both_kinds(rule, oracle, fr, w, h)
    want = oracle.compress(fr, w, h, Q50)
    cap = myyuv_hip.payload_bound(w, h)
    d_bmp = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_sz = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    codec.compress_bmp_device(d_bmp.data_ptr(), 1, w, -h, 32, Q50, d_pay.data_ptr(), cap, d_sz.data_ptr(), stream)
    assert codec.sync_status(stream) == (0, -1)
    assert d_pay[: int(d_sz.item())].cpu().numpy().tobytes() == want


def test_stream_downscale_device(codec, oracle, rule, content):
    """k_downscale at 1/2: 288x64 -> 144x32; the output's luma units (the
    rule on the reference's scaled frame) qualify in part."""
    import torch
    import myyuv_hip
    import downscaleref as D
    import scaleref as S

    w, h, denom = 288, 64, 2
    up = np.kron(G.plane_from_blocks(content, w // 2, h // 2), np.ones((2, 2), np.uint8))
    fr = np.concatenate([up.ravel(), np.full(w * h // 2, 128, np.uint8)]).tobytes()
    pay = oracle.compress(fr, w, h, Q50)
    small = S.cached(pay, w, h, Q50, denom)
    assert_both_kinds(rule, oracle, bytes(small), w // denom, h // denom)
    want = D.cached(pay, w, h, Q50, denom, Q50)
    cap_out = myyuv_hip.payload_bound(w // denom, h // denom)
    cap = (len(pay) + 3) & ~3
    d_pay = torch.frombuffer(bytearray(pay.ljust(cap, b"\0")), dtype=torch.uint8).cuda()
    d_sizes = torch.tensor([len(pay)], dtype=torch.int32, device="cuda")
    d_out = torch.zeros(cap_out, dtype=torch.uint8, device="cuda")
    d_osz = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    codec.downscale_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 1, w, h, Q50, denom, Q50, d_out.data_ptr(),
                           cap_out, d_osz.data_ptr(), stream)
    assert codec.sync_status(stream) == (0, -1)
    assert d_out[: int(d_osz.item())].cpu().numpy().tobytes() == want

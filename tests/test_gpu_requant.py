"""Requantise on the GPU (k_requant, csrc/k_huff_decode.hip, then K2 and K4
unchanged): every output stream is compared byte for byte with the numpy
restatement (requantref) of the definition in include/myyuv_hip.h, twice on
one context.  Frames are small; the geometries are those of the scaled decode's
tests (where groups start and end), the quality pairs cover the identity (a
wrong divide or rounding shows there and at the .5 ties of 90 -> 50), blocks
that become all-zero (100 -> 1) and coefficients that grow (1 -> 100); the
clamp is reached by coefgen's extreme streams."""
import os
import subprocess

import numpy as np
import pytest

import coefgen
import malformed
import regionref as R
import requantref as Q
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
C90 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-90.myyuv")
AW, AH = 208, 96


def q3(q):
    return (q, q, q) if isinstance(q, int) else tuple(q)


def first_difference(a, b):
    n = min(len(a), len(b))
    x, y = np.frombuffer(a[:n], np.uint8), np.frombuffer(b[:n], np.uint8)
    d = np.nonzero(x != y)[0]
    return (len(a), len(b), int(d[0]) if len(d) else None, len(d))


def check(codec, pay, w, h, qs, qd):
    qs, qd = q3(qs), q3(qd)
    want = Q.cached(bytes(pay), qs, qd)
    for rep in range(2):
        got = codec.requantize(pay, w, h, qs, qd)
        assert got == want, (qs, qd, rep, first_difference(got, want))
    return want


def error_of(fn, *args):
    import myyuv_hip

    with pytest.raises(myyuv_hip.CodecError) as e:
        fn(*args)
    return e.value.code, e.value.bad_block


# ---------------------------------------------------------------- geometries
def test_groups_of_4_1_1_blocks(codec, oracle):
    for qs, qd in ((90, 50), (50, 50), (100, 1)):
        check(codec, R.tiled_stream(16, 16, q3(qs))[0], 16, 16, qs, qd)


def test_several_groups_per_block_row(codec, oracle):
    w, h, q = 2080, 32, (50, 50, 50)
    pay = R.tiled_stream(w, h, q)[0]
    check(codec, pay, w, h, q, 30)
    assert codec.requantize(pay, w, h, q, q) == pay


def test_scan_tile_and_plane_boundaries(codec, oracle):
    """8320 + 2080 + 2080 blocks: the decoder's 4096-block scan tiles and K2's
    256-block tiles and 4-tile windows end inside planes and straddle them."""
    w, h, q = 1040, 512, (50, 50, 50)
    assert R.blocks(w, h) == (8320, 2080, 2080)
    pay = R.tiled_stream(w, h, q)[0]
    check(codec, pay, w, h, q, 30)
    assert codec.requantize(pay, w, h, q, q) == pay


# ------------------------------------------------------------- quality pairs
@pytest.mark.parametrize("q", [90, 50, (90, 50, 20)])
def test_identity_returns_the_input_bytes(codec, oracle, q):
    pay = R.tiled_stream(AW, AH, q3(q))[0]
    assert check(codec, pay, AW, AH, q, q) == pay


@pytest.mark.parametrize("qs,qd", [(90, 50), (50, 90), ((90, 50, 20), (30, 70, 100)), (100, 1), (1, 100),
                                   (100, 99), (20, 5)])
def test_quality_pairs(codec, oracle, qs, qd):
    pay = R.tiled_stream(AW, AH, q3(qs))[0]
    want = check(codec, pay, AW, AH, qs, qd)
    assert want != pay


def test_golden_file_at_its_own_quality(codec, golden):
    f = golden("chef-with-trumpet-DCT-50.myyuv")
    q = tuple(f.params)
    assert q == (50, 50, 50)
    for rep in range(2):
        assert codec.requantize(f.data, f.width, f.height, q, q) == f.data


# --------------------------------------------------------------------- noise
def test_noise_two_staging_rounds_and_overflow_tiers(codec, oracle):
    """q100 noise: about 133 B a chunk, so a 64-block group takes two staging
    rounds in the decoder, and nearly every block has more than 8 (at q100 and
    q90 mostly more than 16) distinct symbols: K2's overflow passes write the
    output."""
    q = (100, 100, 100)
    for w, h in ((AW, AH), (1040, 32)):
        pay = R.noise_stream(w, h)[0]
        for qd in (90, 100):
            want = check(codec, pay, w, h, q, qd)
            assert (want == pay) == (qd == 100)


# ------------------------------------------------- coefficient-domain streams
@pytest.mark.parametrize("name", coefgen.stream_names())
def test_coefficient_domain_streams(codec, oracle, name):
    """coefgen.decoder_streams: extremes (+-1023 / -1024 into the clamp), the DC
    sweep, one coefficient at a time, the 64-block group compositions, the
    stage-boundary groups, 16x16; from the stream's own quality to 1, 50, 100."""
    sh = coefgen.shared(oracle)
    s = sh.by_name[name]
    pay = sh.payload(name)
    for qd in (1, 50, 100):
        check(codec, pay, s.w, s.h, s.q, qd)


# ----------------------------------------------------------- irregular tables
def test_irregular_tables(codec, oracle):
    """Valid streams with tables the encoder never writes (decode_general,
    through the coefficient buffer and back).  The identity is NOT the input
    here: the result is the encoder's stream of the same coefficients."""
    q = (100, 100, 100)
    n = 0
    for pay in (R.noise_stream(AW, AH)[0], R.tiled_stream(AW, AH, q)[0]):
        for name, p in malformed.irregular_cases(pay):
            assert p != pay
            for qd in (100, 50):
                want = check(codec, p, AW, AH, q, qd)
                assert want != p and want != Q.cached(pay, q, q3(qd)), name
            n += 1
    assert n == 4


# ------------------------------------------------------------ malformed input
def test_malformed_streams_fail_as_the_full_decode(codec, oracle):
    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    seen = set()
    for name, p, _kind in malformed.cases(pay):
        seen.add(name)
        want = error_of(codec.decompress, p, AW, AH, q)
        assert want[0] != 0
        for qd in (q, (30, 30, 30)):
            assert error_of(codec.requantize, p, AW, AH, q, qd) == want, (name, qd)
    assert {"tiny", "truncated", "plane_size_zero", "bad_code", "unknown_symbol", "content_too_small",
            "nbits_past_chunk"} <= seen
    check(codec, pay, AW, AH, q, 30)  # the context still works


def test_argument_checks_and_their_order(codec):
    import myyuv_hip

    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    for args, code in (((pay, AW, AH, (0, 50, 50), q), myyuv_hip.E_QUALITY),
                       ((pay, AW, AH, q, (50, 101, 50)), myyuv_hip.E_QUALITY),
                       ((pay[:8], AW, AH, q, (0, 0, 0)), myyuv_hip.E_DCTYUV_SIZE),  # the stream before q_dst
                       ((pay, 204, AH, q, (0, 0, 0)), myyuv_hip.E_WIDTH),          # the dimensions before q_dst
                       ((pay, AW, 100, q, q), myyuv_hip.E_HEIGHT)):
        assert error_of(codec.requantize, *args) == (code, -1), args[1:]


def batch_buffers(pays, cap_out, guard=256):
    import torch

    cap = (max(len(p) for p in pays) + 3) & ~3
    buf = bytearray(len(pays) * cap)
    for f, p in enumerate(pays):
        buf[f * cap:f * cap + len(p)] = p
    d_pay = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    d_sizes = torch.tensor([len(p) for p in pays], dtype=torch.int32, device="cuda")
    d_out = torch.full((len(pays) * cap_out + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    d_osz = torch.full((len(pays),), -1, dtype=torch.int32, device="cuda")
    return cap, d_pay, d_sizes, d_out, d_osz


def test_bad_header_in_frame_0_leaves_frame_1_whole(oracle):
    """A two-frame device batch on a FRESH context (its workspace holds
    whatever the allocator returned) where k_scan_chain rejects frame 0's
    header: every lane of frame 0 must hand K2 an all-zero block, or K2 would
    index by stale words.  The call reports frame 0's error; frame 1 is its
    single-frame result."""
    import myyuv_hip
    import torch

    q, qd = (50, 50, 50), (30, 30, 30)
    good, _ = R.tiled_stream(AW, AH, q)
    bad = dict((n, p) for n, p, _ in malformed.cases(good))["truncated"]
    want = Q.cached(good, q, qd)
    cap_out = myyuv_hip.payload_bound(AW, AH)
    stream = torch.cuda.current_stream().cuda_stream
    fresh = myyuv_hip.Codec(0)
    try:
        cap, d_pay, d_sizes, d_out, d_osz = batch_buffers([bad, good], cap_out)
        fresh.requantize_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 2, AW, AH, q, qd, d_out.data_ptr(),
                                cap_out, d_osz.data_ptr(), stream)
        code, blk = fresh.sync_status(stream)
        assert (code, blk) == error_of(fresh.decompress, bad, AW, AH, q)
        assert code == myyuv_hip.E_DCTYUV_SIZE
        out = bytes(d_out.cpu().numpy())
        sizes = d_osz.cpu().tolist()
        assert sizes[1] == len(want)
        assert out[cap_out:cap_out + sizes[1]] == want
        assert 0 <= sizes[0] <= cap_out  # frame 0: unspecified bytes, inside its slot
        assert out[2 * cap_out:] == b"\x5A" * 256
        assert fresh.requantize(good, AW, AH, q, qd) == want  # the context still works
    finally:
        fresh.close()


# ------------------------------------------------------------------ capacity
def test_capacity(codec, oracle):
    import myyuv_hip

    q, qd = (90, 90, 90), (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    want = Q.cached(pay, q, qd)
    src = np.frombuffer(pay, np.uint8).copy()
    short = np.full(len(want) - 1, 0x5A, np.uint8)
    assert error_of(codec.requantize_into, src, AW, AH, q, qd, short) == (myyuv_hip.E_CAPACITY, -1)
    exact = np.full(len(want), 0x5A, np.uint8)
    assert codec.requantize_into(src, AW, AH, q, qd, exact) == len(want) and exact.tobytes() == want
    full = np.full(myyuv_hip.payload_bound(AW, AH) + 64, 0x5A, np.uint8)
    n = codec.requantize_into(src, AW, AH, q, qd, full)
    assert full[:n].tobytes() == want and (full[n:] == 0x5A).all()


def test_device_capacity_stays_inside_cap(codec, oracle):
    import myyuv_hip
    import torch

    q, qd = (90, 90, 90), (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    want = Q.cached(pay, q, qd)
    cap_out = (len(want) // 2) & ~3
    stream = torch.cuda.current_stream().cuda_stream
    cap, d_pay, d_sizes, d_out, d_osz = batch_buffers([pay], cap_out)
    codec.requantize_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 1, AW, AH, q, qd, d_out.data_ptr(), cap_out,
                            d_osz.data_ptr(), stream)
    assert codec.sync_status(stream) == (myyuv_hip.E_CAPACITY, -1)
    assert bytes(d_out.cpu().numpy())[cap_out:] == b"\x5A" * 256
    check(codec, pay, AW, AH, q, qd)


# -------------------------------------------------------------- device batch
def test_device_batch_of_two(codec, oracle):
    import myyuv_hip
    import torch

    sh = coefgen.shared(oracle)
    a, b = coefgen.batch_pair(oracle)
    w, h, q, qd = a.w, a.h, a.q, (30, 70, 100)
    pays = [sh.payload(a.name), sh.payload(b.name)]
    assert pays[0] != pays[1]
    cap_out = myyuv_hip.payload_bound(w, h)
    stream = torch.cuda.current_stream().cuda_stream
    cap, d_pay, d_sizes, d_out, d_osz = batch_buffers(pays, cap_out)
    codec.requantize_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 2, w, h, q, qd, d_out.data_ptr(), cap_out,
                            d_osz.data_ptr(), stream)
    assert codec.sync_status(stream) == (0, -1)
    out = bytes(d_out.cpu().numpy())
    sizes = d_osz.cpu().tolist()
    for f in range(2):
        got = out[f * cap_out:f * cap_out + sizes[f]]
        assert got == Q.cached(pays[f], q, qd), f
        assert got == codec.requantize(pays[f], w, h, q, qd), f
    assert out[2 * cap_out:] == b"\x5A" * 256  # nothing past the last frame
    # alignment, stride and overlap rules
    p, s, o, z = d_pay.data_ptr(), d_sizes.data_ptr(), d_out.data_ptr(), d_osz.data_ptr()
    for args in ((p + 1, s, cap, 2, w, h, q, qd, o, cap_out, z), (p, s, cap, 2, w, h, q, qd, o + 2, cap_out, z),
                 (p, s, cap + 2, 2, w, h, q, qd, o, cap_out, z), (p, s, cap, 2, w, h, q, qd, o, cap_out + 1, z),
                 (p, s, cap, 2, w, h, q, qd, p + cap, cap_out, z), (p, s, cap, 0, w, h, q, qd, o, cap_out, z)):
        assert error_of(codec.requantize_device, *args, stream)[0] == myyuv_hip.E_ARG
    assert codec.sync_status(stream) == (0, -1)


# ---------------------------------------------------------------- round trip
def test_round_trip_decodes_as_the_reference(codec, oracle):
    q, qd = (90, 90, 90), (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    out = codec.requantize(pay, AW, AH, q, qd)
    assert codec.decompress(out, AW, AH, qd) == oracle.decompress(Q.cached(pay, q, qd), AW, AH, qd)
    # and the context's compress / decompress tables are unharmed by the call in between
    raw = oracle.decompress(pay, AW, AH, q)
    assert codec.compress(raw, AW, AH, q) == oracle.compress(raw, AW, AH, q)
    codec.requantize(pay, AW, AH, q, qd)
    assert codec.decompress(pay, AW, AH, q) == raw


# -------------------------------------------------------------- kernel stats
def test_kernel_stats_name_the_requant_kernel(codec):
    q = (90, 90, 90)
    pay, _ = R.tiled_stream(AW, AH, q)
    codec.profile(True, ["requant", "fdct_quant", "fdct_fix", "dequant_idct", "huff_decode", "huff_encode"])
    try:
        codec.requantize(pay, AW, AH, q, (50, 50, 50))
        stats = codec.kernel_stats()
    finally:
        codec.profile(False)
    assert stats["requant"][1] == 1 and stats["requant"][0] > 0
    assert stats["huff_encode"][1] == 1
    for k in ("fdct_quant", "fdct_fix", "dequant_idct", "huff_decode"):  # no K1, no fix kernel, no K6, no K5
        assert stats[k][1] == 0, k


# ----------------------------------------------------------------------- CLI
def test_cli_requantize(codec, tmp_path, golden):
    import myyuv_file

    f = golden("chef-with-trumpet-DCT-90.myyuv")
    assert tuple(f.params) == (90, 90, 90)
    out = tmp_path / "q50.myyuv"
    r = subprocess.run([CLI, C90, "-requantize", "50", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    assert r.stdout.splitlines()[0].startswith("YUV DCT requantization ( 50 ) : ")
    want = Q.cached(f.data, (90, 90, 90), (50, 50, 50))
    assert out.read_bytes() == myyuv_file.YUVFile(f.fourcc, f.width, f.height, myyuv_file.DCT, bytes([50, 50, 50]),
                                                  want, f.unused).dumps()
    assert out.read_bytes()[:64] == f.compressed((50, 50, 50), want).header_bytes()
    back = tmp_path / "back.myyuv"
    r = subprocess.run([CLI, str(out), "-decompress", "-o", str(back)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    assert len(back.read_bytes()) == 64 + f.width * f.height * 3 // 2

"""Transform on the GPU (k_coef_xform, csrc/k_huff_decode.hip, then K2 and K4
unchanged): every output stream is compared byte for byte with the numpy
restatement (xformref) of the definition in include/myyuv_hip.h, twice on one
context.  Frames are small; the geometries are those where 64-block groups
start and end inside block rows and planes (and, after a swap, land in rows of
2 and 4 blocks), the quality pairs cover the identity, a rescale with .5 ties
and blocks that become all-zero; -1024 reaches the negation clamp through
coefgen's extreme streams; irregular Huffman tables go through the scratch
coefficient image."""
import os
import struct
import subprocess

import numpy as np
import pytest

import coefgen
import malformed
import regionref as R
import requantref as Q
import scaleref as S
import xformref as X
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
C90 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-90.myyuv")
AW, AH = 208, 96
N = X.NAMES
SWAPS = ("transpose", "rot90", "rot270", "transverse")
MIRRORS = ("flip_h", "flip_v", "rot180")


def q3(q):
    return (q, q, q) if isinstance(q, int) else tuple(q)


def first_difference(a, b):
    n = min(len(a), len(b))
    x, y = np.frombuffer(a[:n], np.uint8), np.frombuffer(b[:n], np.uint8)
    d = np.nonzero(x != y)[0]
    return (len(a), len(b), int(d[0]) if len(d) else None, len(d))


def check(codec, pay, w, h, qs, op, qd):
    qs, qd = q3(qs), q3(qd)
    want = X.cached(bytes(pay), w, h, qs, op, qd)
    for rep in range(2):
        got = codec.transform(pay, w, h, qs, op, qd)
        assert got == want, (w, h, qs, op, qd, rep, first_difference(got, want))
    return want


def error_of(fn, *args):
    import myyuv_hip

    with pytest.raises(myyuv_hip.CodecError) as e:
        fn(*args)
    return e.value.code, e.value.bad_block


# ---------------------------------------------------------------- geometries
@pytest.mark.parametrize("op", X.OPS)
def test_groups_of_4_1_1_blocks(codec, oracle, op):
    for qs, qd in ((50, 50), (90, 50), (100, 1)):
        check(codec, R.tiled_stream(16, 16, q3(qs))[0], 16, 16, qs, op, qd)


@pytest.mark.parametrize("op", X.OPS)
def test_partial_last_groups(codec, oracle, op):
    """208x96: 312 + 78 + 78 blocks."""
    assert R.blocks(AW, AH) == (312, 78, 78)
    for qs, qd in ((50, 50), (90, 50), ((90, 50, 20), (90, 50, 20)), (100, 100)):
        check(codec, R.tiled_stream(AW, AH, q3(qs))[0], AW, AH, qs, op, qd)


@pytest.mark.parametrize("w,h", [(2080, 32), (32, 2080)])
def test_many_groups_per_block_row_and_rows_of_4_and_2_blocks(codec, oracle, w, h):
    q = (50, 50, 50)
    pay = R.tiled_stream(w, h, q)[0]
    for name in ("flip_h", "rot90", "transverse"):
        check(codec, pay, w, h, q, N[name], q)


def test_scan_tile_and_plane_boundaries(codec, oracle):
    """8320 + 2080 + 2080 blocks: the decoder's 4096-block scan tiles and K2's
    256-block tiles and 4-tile windows end inside planes and straddle them."""
    w, h, q = 1040, 512, (50, 50, 50)
    assert R.blocks(w, h) == (8320, 2080, 2080)
    pay = R.tiled_stream(w, h, q)[0]
    for name in ("rot180", "rot270"):
        check(codec, pay, w, h, q, N[name], q)


def test_op_none_is_requantise(codec, oracle):
    qs, qd = (90, 90, 90), (50, 50, 50)
    pay = R.tiled_stream(AW, AH, qs)[0]
    want = check(codec, pay, AW, AH, qs, 0, qd)
    assert want == Q.cached(pay, qs, qd) == codec.requantize(pay, AW, AH, qs, qd)


# -------------------------------------------------- involutions and inverses
def test_golden_file_mirrored_twice_is_the_file(codec, oracle, golden):
    f = golden("chef-with-trumpet-DCT-50.myyuv")
    q = tuple(f.params)
    assert q == (50, 50, 50)
    for name in ("rot180", "flip_h"):
        once = check(codec, f.data, f.width, f.height, q, N[name], q)
        assert once != f.data
        assert codec.transform(once, f.width, f.height, q, N[name], q) == f.data, name


@pytest.mark.parametrize("q", [100, 1])
def test_swaps_invert_where_the_luma_table_is_symmetric(codec, oracle, q):
    pay = R.tiled_stream(AW, AH, q3(q))[0]
    r90 = check(codec, pay, AW, AH, q, N["rot90"], q)
    assert codec.transform(r90, AH, AW, q3(q), N["rot270"], q3(q)) == pay
    tr = check(codec, pay, AW, AH, q, N["transpose"], q)
    assert codec.transform(tr, AH, AW, q3(q), N["transpose"], q3(q)) == pay


# --------------------------------------------------------------------- noise
@pytest.mark.parametrize("w,h", [(AW, AH), (1040, 32)])
def test_noise_two_staging_rounds_and_overflow_tiers(codec, oracle, w, h):
    """q100 noise: about 133 B a chunk, so a 64-block group takes two staging
    rounds in the decoder, and nearly every block has more than 16 distinct
    symbols: K2's overflow passes write the output.  Bytes only: on noise the
    decoded pixels are not promised (include/myyuv_hip.h)."""
    q = (100, 100, 100)
    pay = R.noise_stream(w, h)[0]
    for name in ("rot90", "flip_v"):
        check(codec, pay, w, h, q, N[name], q)


# -------------------------------------------------------------------- pixels
@pytest.mark.parametrize("q", [1, 50, 90, 100])
def test_decode_of_the_transform_is_the_moved_decode(codec, oracle, q):
    """On the tiled chef window, where the oracle alone gives 0 differing
    pixels (tests/test_coef_xform_host.py): the mirrors at every quality, the
    swapping operations where the luma table is symmetric."""
    q = q3(q)
    pay = R.tiled_stream(AW, AH, q)[0]
    src = codec.decompress(pay, AW, AH, q)
    for name in MIRRORS + (SWAPS if q[0] in (1, 100) else ()):
        op = N[name]
        ow, oh = X.out_size(AW, AH, op)
        out = codec.transform(pay, AW, AH, q, op, q)
        assert codec.decompress(out, ow, oh, q) == X.move_iyuv(src, AW, AH, op), name


# ------------------------------------------------- coefficient-domain streams
@pytest.mark.parametrize("name", coefgen.stream_names())
def test_coefficient_domain_streams(codec, oracle, name):
    """coefgen.decoder_streams: the extremes carry -1024 into the negation
    clamp; the DC sweep, one coefficient at a time, the 64-block group
    compositions, the stage-boundary groups, 16x16."""
    sh = coefgen.shared(oracle)
    s = sh.by_name[name]
    pay = sh.payload(name)
    for op in (N["flip_h"], N["rot270"], N["transverse"]):
        for qd in (s.q, (50, 50, 50)):
            check(codec, pay, s.w, s.h, s.q, op, qd)


# ----------------------------------------------------------- irregular tables
def test_irregular_tables(codec, oracle):
    """Valid streams with tables the encoder never writes (decode_general,
    through the scratch coefficient image and back)."""
    q = (100, 100, 100)
    n = 0
    for pay in (R.noise_stream(AW, AH)[0], R.tiled_stream(AW, AH, q)[0]):
        for name, p in malformed.irregular_cases(pay):
            assert p != pay
            for op in (N["flip_h"], N["rot90"]):
                check(codec, p, AW, AH, q, op, q)
            n += 1
    assert n == 4


def exact_irregular_chunk(groups, seq):
    ch = malformed._irregular_chunk(groups, seq, 255)
    return ch[:3 + ch[2] + ((ch[0] | ch[1] << 8) + 7) // 8]


def all_irregular_luma(pay):
    """The stream `pay` with EVERY luma chunk replaced by an irregular one, two
    distinct blocks alternating in runs of 1, 2, 3, ... blocks."""
    g = [(3, [-7]), (1, [0]), (3, [1023]), (2, [-1024])]
    a = exact_irregular_chunk(g, [0, -7, 1023, 0, -1024, 0, 0, -7, -1024, 1023] * 3)
    b = exact_irregular_chunk(g, [1023, 0, -7, -7, -1024, 0, 1023] * 4)
    planes = S.parse_planes(pay)
    nblk = len(planes[0][0])
    chunks, run, which = [], 1, 0
    while len(chunks) < nblk:
        chunks += [(a, b)[which]] * run
        run, which = run + 1, which ^ 1
    chunks = chunks[:nblk]
    body = [struct.pack("<II", nblk, sum(map(len, chunks))) + bytes(map(len, chunks)) + b"".join(chunks)]
    for sizes, content in planes[1:]:
        body.append(struct.pack("<II", len(sizes), len(content)) + bytes(sizes) + bytes(content))
    return struct.pack("<III", *(len(p) for p in body)) + b"".join(body)


def test_every_luma_chunk_irregular(codec, oracle):
    """Every wave of the luma plane sends all its blocks through
    decode_general: a hand-off image shared with it (one wave's source slot is
    another wave's destination) shows here."""
    q = (100, 100, 100)
    pay = all_irregular_luma(R.tiled_stream(AW, AH, q)[0])
    luma = S.coefficients(pay)[0]
    assert len(luma) == 312 and len({b.tobytes() for b in luma}) == 2
    assert oracle.decompress(pay, AW, AH, q) == codec.decompress(pay, AW, AH, q)
    for op in (N["flip_h"], N["rot90"]):
        want = check(codec, pay, AW, AH, q, op, q)
        assert want != pay


# ------------------------------------------------------------ malformed input
def test_malformed_streams_fail_as_the_full_decode(codec, oracle):
    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    seen = set()
    for name, p, _kind in malformed.cases(pay):
        seen.add(name)
        want = error_of(codec.decompress, p, AW, AH, q)
        assert want[0] != 0
        for op in (N["flip_v"], N["rot90"]):
            assert error_of(codec.transform, p, AW, AH, q, op, q) == want, (name, op)
    assert {"tiny", "truncated", "plane_size_zero", "bad_code", "unknown_symbol", "content_too_small",
            "nbits_past_chunk"} <= seen
    check(codec, pay, AW, AH, q, N["rot90"], q)  # the context still works


def test_argument_checks_and_their_order(codec):
    import myyuv_hip

    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    for args, code in (((pay[:8], AW, AH, (0, 50, 50), 8, q), myyuv_hip.E_ARG),   # op before q_src and the stream
                       ((pay, AW, AH, q, 8, q), myyuv_hip.E_ARG),
                       ((pay, AW, AH, q, 0xFFFFFFF9, q), myyuv_hip.E_ARG),         # (not its low three bits)
                       ((pay, AW, AH, (0, 50, 50), 5, q), myyuv_hip.E_QUALITY),
                       ((pay, AW, AH, q, 5, (50, 101, 50)), myyuv_hip.E_QUALITY),
                       ((pay[:8], AW, AH, q, 5, (0, 0, 0)), myyuv_hip.E_DCTYUV_SIZE),  # the stream before q_dst
                       ((pay, 204, AH, q, 5, (0, 0, 0)), myyuv_hip.E_WIDTH),          # the dimensions before q_dst
                       ((pay, AW, 100, q, 5, q), myyuv_hip.E_HEIGHT)):
        assert error_of(codec.transform, *args) == (code, -1), args[1:]


# -------------------------------------------------------------- device batch
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
    header: every lane of frame 0 must hand K2 an all-zero block at its
    DESTINATION, or K2 would index by stale words."""
    import myyuv_hip
    import torch

    q, op = (50, 50, 50), N["rot90"]
    good, _ = R.tiled_stream(AW, AH, q)
    bad = dict((n, p) for n, p, _ in malformed.cases(good))["truncated"]
    want = X.cached(good, AW, AH, q, op, q)
    cap_out = myyuv_hip.payload_bound(AW, AH)
    stream = torch.cuda.current_stream().cuda_stream
    fresh = myyuv_hip.Codec(0)
    try:
        cap, d_pay, d_sizes, d_out, d_osz = batch_buffers([bad, good], cap_out)
        fresh.transform_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 2, AW, AH, q, op, q, d_out.data_ptr(),
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
        assert fresh.transform(good, AW, AH, q, op, q) == want  # the context still works
    finally:
        fresh.close()


def test_device_batch_of_three(codec, oracle):
    import myyuv_hip
    import torch

    q, op = (50, 50, 50), N["rot180"]
    pays = [R.tiled_stream(AW, AH, q)[0], R.tiled_stream(AW, AH, q, 40, 500)[0], R.tiled_stream(AW, AH, q, 720, 16)[0]]
    assert len(set(pays)) == 3
    cap_out = myyuv_hip.payload_bound(AW, AH)
    stream = torch.cuda.current_stream().cuda_stream
    cap, d_pay, d_sizes, d_out, d_osz = batch_buffers(pays, cap_out)
    codec.transform_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 3, AW, AH, q, op, q, d_out.data_ptr(), cap_out,
                           d_osz.data_ptr(), stream)
    assert codec.sync_status(stream) == (0, -1)
    out = bytes(d_out.cpu().numpy())
    sizes = d_osz.cpu().tolist()
    for f in range(3):
        got = out[f * cap_out:f * cap_out + sizes[f]]
        assert got == X.cached(pays[f], AW, AH, q, op, q), f
        assert got == codec.transform(pays[f], AW, AH, q, op, q), f
    assert out[3 * cap_out:] == b"\x5A" * 256  # nothing past the last frame
    # alignment, stride and overlap rules, as requantize_device; op with the pointers
    p, s, o, z = d_pay.data_ptr(), d_sizes.data_ptr(), d_out.data_ptr(), d_osz.data_ptr()
    g = (3, AW, AH, q, op, q)
    for args in ((p + 1, s, cap, *g, o, cap_out, z), (p, s, cap, *g, o + 2, cap_out, z),
                 (p, s, cap + 2, *g, o, cap_out, z), (p, s, cap, *g, o, cap_out + 1, z),
                 (p, s, cap, *g, p + cap, cap_out, z), (p, s, cap, 0, AW, AH, q, op, q, o, cap_out, z),
                 (p, s, cap, 3, AW, AH, q, 8, q, o, cap_out, z)):
        assert error_of(codec.transform_device, *args, stream)[0] == myyuv_hip.E_ARG
    assert codec.sync_status(stream) == (0, -1)


# ------------------------------------------------------------------ capacity
def test_capacity(codec, oracle):
    import myyuv_hip

    q, op = (90, 90, 90), N["rot90"]
    pay, _ = R.tiled_stream(AW, AH, q)
    want = X.cached(pay, AW, AH, q, op, q)
    src = np.frombuffer(pay, np.uint8).copy()
    short = np.full(len(want) - 1, 0x5A, np.uint8)
    assert error_of(codec.transform_into, src, AW, AH, q, op, q, short) == (myyuv_hip.E_CAPACITY, -1)
    exact = np.full(len(want), 0x5A, np.uint8)
    assert codec.transform_into(src, AW, AH, q, op, q, exact) == len(want) and exact.tobytes() == want
    full = np.full(myyuv_hip.payload_bound(AW, AH) + 64, 0x5A, np.uint8)
    n = codec.transform_into(src, AW, AH, q, op, q, full)
    assert full[:n].tobytes() == want and (full[n:] == 0x5A).all()


def test_device_capacity_stays_inside_cap(codec, oracle):
    import myyuv_hip
    import torch

    q, op = (90, 90, 90), N["flip_h"]
    pay, _ = R.tiled_stream(AW, AH, q)
    want = X.cached(pay, AW, AH, q, op, q)
    cap_out = (len(want) // 2) & ~3
    stream = torch.cuda.current_stream().cuda_stream
    cap, d_pay, d_sizes, d_out, d_osz = batch_buffers([pay], cap_out)
    codec.transform_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 1, AW, AH, q, op, q, d_out.data_ptr(), cap_out,
                           d_osz.data_ptr(), stream)
    assert codec.sync_status(stream) == (myyuv_hip.E_CAPACITY, -1)
    assert bytes(d_out.cpu().numpy())[cap_out:] == b"\x5A" * 256
    check(codec, pay, AW, AH, q, op, q)


# ------------------------------------------------- the other calls' tables
def test_requantise_and_the_codec_are_unharmed_by_a_swap(codec, oracle):
    """The transform shares the requantiser's table buffer and its cache, with
    the source table held transposed for a swap: the same six qualities without
    the swap must not find that table."""
    qs, qd = (90, 90, 90), (50, 50, 50)
    pay, raw = R.tiled_stream(AW, AH, qs)
    check(codec, pay, AW, AH, qs, N["transpose"], qd)
    assert codec.requantize(pay, AW, AH, qs, qd) == Q.cached(pay, qs, qd)
    check(codec, pay, AW, AH, qs, N["flip_h"], qd)
    check(codec, pay, AW, AH, qs, N["rot90"], qd)
    assert codec.decompress(pay, AW, AH, qs) == raw


# -------------------------------------------------------------- kernel stats
def test_kernel_stats_name_the_transform_kernel(codec):
    q = (90, 90, 90)
    pay, _ = R.tiled_stream(AW, AH, q)
    codec.profile(True, ["coef_xform", "requant", "fdct_quant", "dequant_idct", "huff_decode", "huff_encode"])
    try:
        codec.transform(pay, AW, AH, q, N["rot90"], q)
        stats = codec.kernel_stats()
    finally:
        codec.profile(False)
    assert stats["coef_xform"][1] == 1 and stats["coef_xform"][0] > 0
    assert stats["huff_encode"][1] == 1
    for k in ("requant", "fdct_quant", "dequant_idct", "huff_decode"):
        assert stats[k][1] == 0, k


# ----------------------------------------------------------------------- CLI
def test_cli_transform(codec, tmp_path, golden):
    import myyuv_file

    f = golden("chef-with-trumpet-DCT-90.myyuv")
    q = (90, 90, 90)
    assert tuple(f.params) == q
    out = tmp_path / "r90.myyuv"
    r = subprocess.run([CLI, C90, "-transform", "rot90", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    assert r.stdout.splitlines()[0].startswith("YUV DCT transform ( rot90 ) : ")
    want = X.cached(f.data, f.width, f.height, q, N["rot90"], q)
    assert out.read_bytes() == myyuv_file.YUVFile(f.fourcc, f.height, f.width, myyuv_file.DCT, bytes(q), want,
                                                  f.unused).dumps()
    out2 = tmp_path / "fh50.myyuv"
    r = subprocess.run([CLI, C90, "-transform", "flip_h", "-q", "50", "-o", str(out2)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[0].startswith("YUV DCT transform ( flip_h 50 ) : "), r.stdout
    want = X.cached(f.data, f.width, f.height, q, N["flip_h"], (50, 50, 50))
    assert out2.read_bytes() == myyuv_file.YUVFile(f.fourcc, f.width, f.height, myyuv_file.DCT, bytes([50, 50, 50]),
                                                   want, f.unused).dumps()
    back = tmp_path / "back.myyuv"
    r = subprocess.run([CLI, str(out), "-decompress", "-o", str(back)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    assert len(back.read_bytes()) == 64 + f.width * f.height * 3 // 2

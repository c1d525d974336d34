"""Scaled decode on the GPU (k_decode_scaled, csrc/k_huff_decode.hip): every
result is compared byte for byte with the numpy restatement (scaleref) of the
definition in include/myyuv_hip.h, at 1/2, 1/4 and 1/8, twice on one context.
Frames are small; the geometries are chosen for where groups start and end:
  16x16      one luma group of 4 lanes; a 1x1 chroma plane at 1/8;
  208x96     26 and 13 blocks per row: no row length divides 64, so groups wrap
             block rows mid-wave and output rows are 13..104 bytes wide;
  2080x32    several groups per block row;
  1040x512   the 4096-block scan tiles end inside Y and straddle the plane
             boundaries."""
import os
import subprocess

import numpy as np
import pytest

import coefgen
import colorref as C
import malformed
import regionref as R
import scaleref as S
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
AW, AH = 208, 96


def check(codec, pay, w, h, q):
    for denom in S.DENOMS:
        want = S.cached(bytes(pay), w, h, tuple(q), denom)
        for rep in range(2):
            got = codec.decompress_scaled(pay, w, h, q, denom)
            assert len(got) == w * h * 3 // 2 // denom ** 2
            assert got == want, (denom, rep, first_difference(got, want))


def first_difference(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    d = np.nonzero(a != b)[0]
    return (int(d[0]), int(a[d[0]]), int(b[d[0]]), len(d)) if len(d) else None


# ---------------------------------------------------------------- geometries
@pytest.mark.parametrize("q", [(50, 50, 50), (90, 90, 90), (90, 50, 20)])
def test_rows_that_divide_no_group(codec, oracle, q):
    pay, _ = R.tiled_stream(AW, AH, q)
    check(codec, pay, AW, AH, q)


def test_several_groups_per_block_row(codec, oracle):
    w, h, q = 2080, 32, (50, 50, 50)
    check(codec, R.tiled_stream(w, h, q)[0], w, h, q)


def test_scan_tile_and_plane_boundaries(codec, oracle):
    w, h, q = 1040, 512, (50, 50, 50)
    assert R.blocks(w, h) == (8320, 2080, 2080)
    check(codec, R.tiled_stream(w, h, q)[0], w, h, q)


def test_noise_two_staging_rounds(codec, oracle):
    """q100 noise, about 133 B a chunk: a 64-block group holds 8.5 KB, more
    than the 5.1 KB stage, so it takes two rounds."""
    q = (100, 100, 100)
    check(codec, R.noise_stream(AW, AH)[0], AW, AH, q)
    w, h = 1040, 32
    pay, _ = R.noise_stream(w, h)
    nblk = int.from_bytes(pay[12:16], "little")
    sizes = pay[20:20 + nblk]
    assert min(sum(sizes[k:k + 64]) for k in range(0, nblk - 64, 64)) > 5104
    check(codec, pay, w, h, q)


# ----------------------------------------------------------- irregular tables
def test_irregular_tables(codec, oracle):
    """Valid streams with tables the encoder never writes (decode_general,
    through the coefficient buffer), built as tests/test_gpu_region.py builds
    them: frame A's q100 streams (the cases need a chunk of about 130 B)."""
    q = (100, 100, 100)
    n = 0
    for pay in (R.noise_stream(AW, AH)[0], R.tiled_stream(AW, AH, q)[0]):
        for name, p in malformed.irregular_cases(pay):
            assert p != pay
            assert S.cached(p, AW, AH, q, 2) != S.cached(pay, AW, AH, q, 2), name
            check(codec, p, AW, AH, q)
            n += 1
    assert n == 4


def test_many_irregular_tables_in_one_group(codec, oracle):
    q = (100, 100, 100)
    pay, _ = R.noise_stream(AW, AH)
    nblk = int.from_bytes(pay[12:16], "little")
    sizes = pay[20:20 + nblk]
    groups = [(3, [-7]), (1, [0]), (3, [1023]), (2, [-1024])]
    p = bytearray(pay)
    for k in range(26 + 3, 26 + 23):  # block row 1, columns 3..22
        off = 20 + nblk + sum(sizes[:k])
        seq = [0, -7, 1023, 0, -1024, 0, 0, -7, -1024, 1023][: 1 + k % 10] * 3
        p[off:off + sizes[k]] = malformed._irregular_chunk(groups, seq, sizes[k])
    check(codec, bytes(p), AW, AH, q)


# ------------------------------------------------- coefficient-domain streams
@pytest.mark.parametrize("name", coefgen.stream_names())
def test_coefficient_domain_streams(codec, oracle, name):
    """coefgen.decoder_streams: the DC sweep (the .5 ties), extremes (the
    clamp), one coefficient at a time, the 64-block group compositions, the
    stage-boundary groups, 16x16 (groups of 4 + 1 + 1 blocks)."""
    sh = coefgen.shared(oracle)
    s = sh.by_name[name]
    check(codec, sh.payload(name), s.w, s.h, s.q)


# -------------------------------------------------------------- device batch
def test_device_batch_of_two(codec, oracle):
    import torch

    sh = coefgen.shared(oracle)
    a, b = coefgen.batch_pair(oracle)
    w, h, q = a.w, a.h, a.q
    pays = [sh.payload(a.name), sh.payload(b.name)]
    assert pays[0] != pays[1]
    cap = (max(len(p) for p in pays) + 3) & ~3
    stream = torch.cuda.current_stream().cuda_stream
    for denom in S.DENOMS:
        sb = w * h * 3 // 2 // denom ** 2
        buf = bytearray(2 * cap)
        for f, p in enumerate(pays):
            buf[f * cap:f * cap + len(p)] = p
        d_pay = torch.frombuffer(buf, dtype=torch.uint8).cuda()
        d_sizes = torch.tensor([len(p) for p in pays], dtype=torch.int32, device="cuda")
        d_out = torch.full((2 * sb + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        codec.decompress_scaled_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 2, w, h, q, denom,
                                       d_out.data_ptr(), stream)
        assert codec.sync_status(stream) == (0, -1)
        out = bytes(d_out.cpu().numpy())
        for f in range(2):
            assert out[f * sb:(f + 1) * sb] == S.cached(pays[f], w, h, q, denom), (denom, f)
            assert out[f * sb:(f + 1) * sb] == codec.decompress_scaled(pays[f], w, h, q, denom), (denom, f)
        assert out[2 * sb:] == b"\x5A" * 256  # nothing past the last frame
    # a bad chunk in frame 1: the batch-global block index
    nblk = int.from_bytes(pays[1][12:16], "little")
    sizes = pays[1][20:20 + nblk]
    k = next(k for k in range(70, nblk) if sizes[k] >= 12)
    off = 20 + nblk + sum(sizes[:k])
    p1 = bytearray(pays[1])
    p1[off:off + sizes[k]] = malformed._bits_run_out(bytes(p1[off:off + sizes[k]]), sizes[k])
    buf = bytearray(2 * cap)
    buf[:len(pays[0])] = pays[0]
    buf[cap:cap + len(p1)] = p1
    d_pay = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    codec.decompress_scaled_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 2, w, h, q, 4, d_out.data_ptr(), stream)
    assert codec.sync_status(stream) == (10, sum(coefgen.plane_counts(w, h)) + k)


# -------------------------------------------------------------------- errors
def error_of(fn, *args):
    import myyuv_hip

    with pytest.raises(myyuv_hip.CodecError) as e:
        fn(*args)
    return e.value.code, e.value.bad_block


def test_malformed_streams_fail_as_the_full_decode(codec, oracle):
    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    seen = set()
    for name, p, _kind in malformed.cases(pay):
        seen.add(name)
        want = error_of(codec.decompress, p, AW, AH, q)
        assert want[0] != 0
        for denom in S.DENOMS:
            assert error_of(codec.decompress_scaled, p, AW, AH, q, denom) == want, (name, denom)
    assert {"tiny", "truncated", "plane_size_zero", "bad_code", "unknown_symbol", "content_too_small",
            "nbits_past_chunk"} <= seen
    check(codec, pay, AW, AH, q)  # the context still works


def test_lowest_bad_block_wins(codec, oracle):
    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    one = malformed._replace_chunk(pay, malformed._bits_run_out)
    nblk = int.from_bytes(pay[12:16], "little")
    sizes = pay[20:20 + nblk]
    k1 = next(k for k in range(128, nblk) if sizes[k] >= 12)  # another group
    off = 20 + nblk + sum(sizes[:k1])
    two = bytearray(one)
    two[off:off + sizes[k1]] = malformed._unknown_symbol(bytes(two[off:off + sizes[k1]]), sizes[k1])
    two = bytes(two)
    want = error_of(codec.decompress, two, AW, AH, q)
    assert want[0] == 10 and 0 <= want[1] < k1
    for denom in S.DENOMS:
        assert error_of(codec.decompress_scaled, two, AW, AH, q, denom) == want


@pytest.mark.parametrize("denom", [0, 1, 3, 5, 6, 7, 16, 0xFFFFFFFF])
def test_denom_argument(codec, denom):
    import myyuv_hip

    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    assert error_of(codec.decompress_scaled, pay, AW, AH, q, denom) == (myyuv_hip.E_ARG, -1)
    assert error_of(codec.decompress_scaled_to_bmp, pay, AW, -AH, q, denom)[0] == myyuv_hip.E_ARG


def test_denom_check_comes_last(codec):
    """Quality, stream header and % 8 dimension errors win over a bad denom."""
    import myyuv_hip

    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    for args, code in (((pay, AW, AH, (0, 50, 50), 3), myyuv_hip.E_QUALITY),
                       ((pay[:8], AW, AH, q, 3), myyuv_hip.E_DCTYUV_SIZE),
                       ((pay, 204, AH, q, 3), myyuv_hip.E_WIDTH),
                       ((pay, AW, 100, q, 3), myyuv_hip.E_HEIGHT)):
        assert error_of(codec.decompress_scaled, *args)[0] == code, args[1:]
        assert error_of(codec.decompress_scaled_to_bmp, args[0], args[1], -args[2], args[3], args[4])[0] == code


# -------------------------------------------------------------------- to BMP
@pytest.mark.parametrize("bits", [24, 32])
@pytest.mark.parametrize("mode", [C.NEAREST, C.LINEAR])
def test_scaled_to_bmp(codec, oracle, bits, mode):
    """By definition iyuv_to_bmp of the scaled frame.  256 / 8 = 32 is a
    multiple of 4."""
    w, h, q = 256, 96, (50, 50, 50)
    pay, _ = R.tiled_stream(w, h, q)
    for denom in S.DENOMS:
        frame = S.cached(pay, w, h, q, denom)
        for sw, sh in C.ORIENTS:
            got = codec.decompress_scaled_to_bmp(pay, sw * w, sh * h, q, denom, bits, mode)
            assert got == C.to_bmp(frame, sw * w // denom, sh * h // denom, bits, mode), (denom, sw, sh)


def test_scaled_to_bmp_width_rule(codec, oracle):
    """K8's argument errors apply to the scaled size: 208 / 8 = 26 is no
    multiple of 4, 208 / 4 = 52 is."""
    import myyuv_hip

    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    assert error_of(codec.decompress_scaled_to_bmp, pay, AW, -AH, q, 8) == (myyuv_hip.E_BMP_INVALID, -1)
    got = codec.decompress_scaled_to_bmp(pay, AW, -AH, q, 4, 24, C.NEAREST)
    assert got == C.to_bmp(S.cached(pay, AW, AH, q, 4), AW // 4, -AH // 4, 24, C.NEAREST)
    assert error_of(codec.decompress_scaled_to_bmp, pay, AW, -AH, q, 4, 16)[0] == myyuv_hip.E_BMP_UNSUPPORTED
    assert error_of(codec.decompress_scaled_to_bmp, pay, -AW, -AH, q, 4)[0] == myyuv_hip.E_BMP_SIGN


# ----------------------------------------------------------------------- CLI
def test_cli_scale(codec, tmp_path, golden):
    """992 / 8 = 124 is a multiple of 4, and so is 992 / 4."""
    import myyuv_file

    f = golden("chef-with-trumpet-DCT-50.myyuv")
    q = tuple(f.params)
    assert (f.width, f.height) == (992, 736)
    out = tmp_path / "quarter.myyuv"
    r = subprocess.run([CLI, C50, "-decompress", "-scale", "1/4", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    want = S.cached(f.data, f.width, f.height, q, 4)
    assert out.read_bytes() == myyuv_file.YUVFile(f.fourcc, 248, 184, myyuv_file.NONE, b"", want, f.unused).dumps()
    bmp = tmp_path / "eighth.bmp"
    r = subprocess.run([CLI, C50, "-to_bmp", "-scale", "1/8", "-o", str(bmp)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    frame = S.cached(f.data, f.width, f.height, q, 8)
    assert bmp.read_bytes() == myyuv_file.BMPFile(124, 92, 32, C.to_bmp(frame, 124, 92, 32, C.LINEAR)).dumps()


def test_kernel_stats_name_the_scaled_kernel(codec):
    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    codec.profile(True, ["decode_scaled", "huff_decode", "dequant_idct"])
    try:
        for denom in S.DENOMS:
            codec.decompress_scaled(pay, AW, AH, q, denom)
        stats = codec.kernel_stats()
    finally:
        codec.profile(False)
    assert stats["decode_scaled"][1] == 3 and stats["decode_scaled"][0] > 0
    assert stats["huff_decode"][1] == 0 and stats["dequant_idct"][1] == 0  # the full decoders are not run

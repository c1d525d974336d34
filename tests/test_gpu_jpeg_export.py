"""Export to JPEG on the GPU (k_jpeg_export and k_jpeg_place,
csrc/k_huff_decode.hip): every file is compared byte for byte with the Python
restatement (jpegref.export) of the definition in include/myyuv_hip.h, twice on
one context.  Frames are small: the geometries put group, plane and scan-tile
boundaries where the kernel's paths change, the noise frame makes the byte
stuffing work, and crafted coefficients reach every branch of the block code
(zero runs around 16, coefficient 63, the DC swing of +-2047, the AC clamp) and
intervals longer than the kernel's LDS image."""
import os
import subprocess

import numpy as np
import pytest

import coefgen
import jpegref as J
import malformed
import regionref as R
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
AW, AH = 208, 96


def q3(q):
    return (q, q, q) if isinstance(q, int) else tuple(q)


def first_difference(a, b):
    n = min(len(a), len(b))
    x, y = np.frombuffer(a[:n], np.uint8), np.frombuffer(b[:n], np.uint8)
    d = np.nonzero(x != y)[0]
    return (len(a), len(b), int(d[0]) if len(d) else None, len(d))


def check(codec, pay, w, h, q):
    q = q3(q)
    want = J.export(bytes(pay), w, h, q)
    for rep in range(2):
        got = codec.to_jpeg(pay, w, h, q)
        assert got == want, (w, h, q, rep, first_difference(got, want))
    return want


def error_of(fn, *args):
    import myyuv_hip

    with pytest.raises(myyuv_hip.CodecError) as e:
        fn(*args)
    return e.value.code, e.value.bad_block


# ---------------------------------------------------------------- geometries
def test_groups_of_4_1_1_blocks(codec, oracle):
    want = check(codec, R.tiled_stream(16, 16, (50, 50, 50))[0], 16, 16, 50)
    scans = want[len(J.header(16, 16, J.qtables_of((50, 50, 50)))):]
    assert not any(bytes([0xFF, 0xD0 + m]) in scans for m in range(8))  # partial groups, no RST


def test_several_groups_per_block_row(codec, oracle):
    w, h, q = 2080, 32, (50, 50, 50)
    check(codec, R.tiled_stream(w, h, q)[0], w, h, q)


def test_rst_counter_wraps_and_a_short_last_interval(codec, oracle):
    """1040x64: 1,040 luma blocks are 17 intervals (m wraps twice), each chroma
    plane's 260 blocks are 5, the last with 4 blocks."""
    w, h, q = 1040, 64, (50, 50, 50)
    assert R.blocks(w, h) == (1040, 260, 260)
    want = check(codec, R.tiled_stream(w, h, q)[0], w, h, q)
    assert len(want) == 5896


def test_scan_tile_and_plane_boundaries(codec, oracle):
    """8320 + 2080 + 2080 blocks: the decoder's 4096-block scan tiles end inside planes."""
    w, h, q = 1040, 512, (50, 50, 50)
    assert R.blocks(w, h) == (8320, 2080, 2080)
    check(codec, R.tiled_stream(w, h, q)[0], w, h, q)


def test_three_different_tables(codec, oracle):
    q = (90, 50, 30)
    want = check(codec, R.tiled_stream(AW, AH, q)[0], AW, AH, q)
    assert len(want) == 7075
    _, _, _, qt = J.parse(want)
    assert [t.tolist() for t in qt] == [np.asarray(oracle.qtable(q[p], p != 0)).reshape(64).astype(int).tolist()
                                        for p in range(3)]


def test_golden_file(codec, golden):
    f = golden("chef-with-trumpet-DCT-50.myyuv")
    check(codec, f.data, f.width, f.height, tuple(f.params))


# ------------------------------------------------------------- byte stuffing
def test_noise_byte_stuffing(codec, oracle):
    q = (100, 100, 100)
    pay = R.noise_stream(AW, AH)[0]
    want = J.export(pay, AW, AH, q)
    assert want.count(b"\xff\x00") >= 50
    check(codec, pay, AW, AH, q)
    pay = R.noise_stream(1040, 32)[0]
    check(codec, pay, 1040, 32, q)


# ------------------------------------------------------ crafted coefficients
def crafted_blocks():
    """Zig-zag blocks for every branch of the block code."""
    out = []
    for run in (15, 16, 31, 32, 47):  # exactly `run` zeros, then a coefficient, then EOB
        b = np.zeros(64, np.int16)
        b[0], b[1 + run] = 5, 3
        out.append(b)
        b = np.zeros(64, np.int16)  # ... and the same run twice
        b[0], b[1 + run] = -5, -3
        if 2 + 2 * run < 64:
            b[2 + 2 * run] = 77
        out.append(b)
    b = np.zeros(64, np.int16)  # the only AC is coefficient 63: three ZRL, no EOB
    b[63] = -2
    out.append(b)
    b = np.zeros(64, np.int16)  # coefficient 63 set among others: no EOB
    b[0], b[1], b[40], b[63] = 100, -1, 9, 1
    out.append(b)
    for ac in (1023, -1024, -1023, 512, -512):  # category 10, and the clamp of -1024
        b = np.zeros(64, np.int16)
        b[0], b[1], b[17], b[62] = 1, ac, ac, ac
        out.append(b)
    out.append(np.zeros(64, np.int16))  # the all-zero block
    return np.stack(out)


def dc_swing(blocks):
    """DC alternating -1024 / 1023: differences of -1024, then +-2047."""
    blocks = np.array(blocks, np.int16)
    blocks[0::2, 0] = -1024
    blocks[1::2, 0] = 1023
    return blocks


def maximal_group(sign_seed):
    """64 blocks, every AC +-1023 and the DC swing: the longest interval."""
    rng = np.random.default_rng(sign_seed)
    g = np.where(rng.integers(0, 2, (64, 64)) == 1, 1023, -1023).astype(np.int16)
    return dc_swing(g)


def test_crafted_block_codes(codec, oracle):
    w, h, q = 64, 64, (50, 60, 70)
    ny, nc, _ = coefgen.plane_counts(w, h)
    pool = crafted_blocks()
    rng = np.random.default_rng(31)
    planes = [pool[np.arange(ny) % len(pool)], dc_swing(pool[rng.integers(0, len(pool), nc)]),
              pool[::-1][np.arange(nc) % len(pool)]]
    pay = coefgen.build_payload(planes, oracle)
    want = check(codec, pay, w, h, q)
    _, _, got, _ = J.parse(want)
    for p in range(3):
        nat = coefgen.natural(planes[p])
        clamped = np.where(nat == -1024, -1023, nat)
        clamped[:, 0] = nat[:, 0]  # the DC is not clamped
        assert (got[p] == clamped).all(), p
    assert any((coefgen.natural(planes[p])[:, 1:] == -1024).any() for p in range(3))


def test_dc_swing_of_2047(codec, oracle):
    w, h, q = 128, 32, (50, 50, 50)
    ny, nc, _ = coefgen.plane_counts(w, h)
    planes = [dc_swing(np.zeros((ny, 64), np.int16)), dc_swing(np.zeros((nc, 64), np.int16))[::-1],
              dc_swing(crafted_blocks()[np.arange(nc) % 5])]
    check(codec, coefgen.build_payload(planes, oracle), w, h, q)


def test_maximal_intervals_exceed_the_lds_image(codec, oracle):
    """128x128: four luma groups (maximal, ordinary, maximal, ordinary), a
    maximal Cb group and an ordinary Cr group.  A maximal luma interval is about
    13.3 KB before stuffing: two windows of the kernel's 7 KB image."""
    import myyuv_hip

    w, h, q = 128, 128, (50, 50, 50)
    rng = np.random.default_rng(77)
    ordinary = coefgen.in_range_blocks(64, oracle.qtable(50, 0), rng)
    planes = [np.concatenate([maximal_group(1), ordinary, maximal_group(2), ordinary[::-1]]), maximal_group(3),
              ordinary]
    pay = coefgen.build_payload(planes, oracle)
    want = check(codec, pay, w, h, q)
    assert len(want) > 2 * 13000 + 11000
    assert len(want) <= myyuv_hip.jpeg_bound(w, h)


@pytest.mark.parametrize("name", coefgen.stream_names())
def test_coefficient_domain_streams(codec, oracle, name):
    sh = coefgen.shared(oracle)
    s = sh.by_name[name]
    check(codec, sh.payload(name), s.w, s.h, s.q)


# ----------------------------------------------------------- irregular tables
def test_irregular_tables(codec, oracle):
    """Valid streams with tables the encoder never writes: decode_general
    feeds the exporter through the coefficient buffer."""
    q = (100, 100, 100)
    n = 0
    for pay in (R.noise_stream(AW, AH)[0], R.tiled_stream(AW, AH, q)[0]):
        for name, p in malformed.irregular_cases(pay):
            assert p != pay
            assert check(codec, p, AW, AH, q) != J.export(pay, AW, AH, q), name
            n += 1
    assert n == 4


def test_odd_chunks_of_streamcases(codec, oracle):
    import streamcases

    n = 0
    for c in streamcases.cases(oracle):
        if c.expect[0] != 0:
            continue
        # (from the case's blocks, not from a decode of its chunks)
        want = J.export_planes([coefgen.natural(b) for b in c.blocks], c.w, c.h, J.qtables_of(c.q))
        for rep in range(2):
            got = codec.to_jpeg(c.payload, c.w, c.h, c.q)
            assert got == want, (c.name, rep, first_difference(got, want))
        n += 1
    assert n >= 4


# --------------------------------------------------------------------- errors
def test_malformed_streams_fail_as_the_full_decode(codec, oracle):
    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    seen = set()
    for name, p, _kind in malformed.cases(pay):
        seen.add(name)
        want = error_of(codec.decompress, p, AW, AH, q)
        assert want[0] != 0
        assert error_of(codec.to_jpeg, p, AW, AH, q) == want, name
    assert {"tiny", "truncated", "plane_size_zero", "bad_code", "unknown_symbol", "content_too_small",
            "nbits_past_chunk"} <= seen
    check(codec, pay, AW, AH, q)  # the context still works


def test_capacity(codec, oracle):
    import myyuv_hip

    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    want = J.export(pay, AW, AH, q)
    src = np.frombuffer(pay, np.uint8).copy()
    short = np.full(len(want) - 1, 0x5A, np.uint8)
    with pytest.raises(myyuv_hip.CodecError) as e:
        codec.to_jpeg_into(src, AW, AH, q, short)
    assert (e.value.code, e.value.bad_block, e.value.size) == (myyuv_hip.E_CAPACITY, -1, len(want))
    assert (short == 0x5A).all()
    exact = np.full(len(want), 0x5A, np.uint8)
    assert codec.to_jpeg_into(src, AW, AH, q, exact) == len(want) and exact.tobytes() == want
    full = np.full(len(want) + 64, 0x5A, np.uint8)
    n = codec.to_jpeg_into(src, AW, AH, q, full)
    assert full[:n].tobytes() == want and (full[n:] == 0x5A).all()


def test_dimension_error(codec, oracle):
    import myyuv_hip

    q = (50, 50, 50)
    pay, _ = R.tiled_stream(16, 16, q)
    assert error_of(codec.to_jpeg, pay, 65536, 16, q) == (myyuv_hip.E_JPEG_DIM, -1)
    assert error_of(codec.to_jpeg, pay, 16, 65536, q) == (myyuv_hip.E_JPEG_DIM, -1)
    assert myyuv_hip.error_message(myyuv_hip.E_JPEG_DIM) == "JPEG width and height must not exceed 65535"
    check(codec, pay, 16, 16, q)


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


def test_device_batch_of_three(codec, oracle):
    import myyuv_hip
    import torch

    q = (100, 100, 100)
    pays = [R.tiled_stream(AW, AH, q)[0], R.noise_stream(AW, AH)[0], R.tiled_stream(AW, AH, q, 40, 900)[0]]
    assert len(set(pays)) == 3
    wants = [J.export(p, AW, AH, q) for p in pays]
    cap_out = max(len(x) for x in wants) + 37  # (no alignment is asked of the files' slots)
    stream = torch.cuda.current_stream().cuda_stream
    cap, d_pay, d_sizes, d_out, d_osz = batch_buffers(pays, cap_out)
    for rep in range(2):
        codec.to_jpeg_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 3, AW, AH, q, d_out.data_ptr(), cap_out,
                             d_osz.data_ptr(), stream)
        assert codec.sync_status(stream) == (0, -1)
        out = bytes(d_out.cpu().numpy())
        sizes = d_osz.cpu().tolist()
        assert sizes == [len(x) for x in wants]
        for f in range(3):
            got = out[f * cap_out:f * cap_out + sizes[f]]
            assert got == wants[f], (f, first_difference(got, wants[f]))
            assert out[f * cap_out + sizes[f]:(f + 1) * cap_out] == b"\x5A" * (cap_out - sizes[f]), f  # the canary
        assert out[3 * cap_out:] == b"\x5A" * 256
    p, s, o, z = d_pay.data_ptr(), d_sizes.data_ptr(), d_out.data_ptr(), d_osz.data_ptr()
    for args in ((p + 1, s, cap, 3, AW, AH, q, o, cap_out, z), (p, s, cap + 2, 3, AW, AH, q, o, cap_out, z),
                 (p, s, cap, 3, AW, AH, q, p + cap, cap_out, z), (p, s, cap, 0, AW, AH, q, o, cap_out, z)):
        assert error_of(codec.to_jpeg_device, *args, stream)[0] == myyuv_hip.E_ARG
    assert codec.sync_status(stream) == (0, -1)


def test_device_capacity_writes_nothing_of_that_file(codec, oracle):
    import myyuv_hip
    import torch

    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    want = J.export(pay, AW, AH, q)
    cap_out = len(want) - 1
    stream = torch.cuda.current_stream().cuda_stream
    cap, d_pay, d_sizes, d_out, d_osz = batch_buffers([pay], cap_out)
    codec.to_jpeg_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 1, AW, AH, q, d_out.data_ptr(), cap_out,
                         d_osz.data_ptr(), stream)
    assert codec.sync_status(stream) == (myyuv_hip.E_CAPACITY, -1)
    assert d_osz.cpu().tolist() == [len(want)]
    assert bytes(d_out.cpu().numpy()) == b"\x5A" * (cap_out + 256)
    check(codec, pay, AW, AH, q)


def test_bad_header_in_frame_0_leaves_frame_1_whole(oracle):
    import myyuv_hip
    import torch

    q = (50, 50, 50)
    good, _ = R.tiled_stream(AW, AH, q)
    bad = dict((n, p) for n, p, _ in malformed.cases(good))["truncated"]
    want = J.export(good, AW, AH, q)
    cap_out = len(want) + 512
    stream = torch.cuda.current_stream().cuda_stream
    fresh = myyuv_hip.Codec(0)
    try:
        cap, d_pay, d_sizes, d_out, d_osz = batch_buffers([bad, good], cap_out)
        fresh.to_jpeg_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 2, AW, AH, q, d_out.data_ptr(), cap_out,
                             d_osz.data_ptr(), stream)
        code, blk = fresh.sync_status(stream)
        assert (code, blk) == error_of(fresh.decompress, bad, AW, AH, q)
        out = bytes(d_out.cpu().numpy())
        sizes = d_osz.cpu().tolist()
        assert sizes[1] == len(want) and out[cap_out:cap_out + sizes[1]] == want
        assert 0 <= sizes[0] <= cap_out
        assert out[2 * cap_out:] == b"\x5A" * 256
    finally:
        fresh.close()


# -------------------------------------------------------------- kernel stats
def test_kernel_stats_name_the_export_kernels(codec):
    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    codec.profile(True, ["jpeg_export", "jpeg_place", "requant", "huff_encode", "dequant_idct"])
    try:
        codec.to_jpeg(pay, AW, AH, q)
        stats = codec.kernel_stats()
    finally:
        codec.profile(False)
    assert stats["jpeg_export"][1] == 2 and stats["jpeg_export"][0] > 0  # the sizing and the writing launch
    assert stats["jpeg_place"][1] == 2
    for k in ("requant", "huff_encode", "dequant_idct"):
        assert stats[k][1] == 0, k


# ----------------------------------------------------------------------- CLI
def test_cli_to_jpeg_of_a_compressed_file(tmp_path, golden, oracle):
    f = golden("chef-with-trumpet-DCT-50.myyuv")
    out = tmp_path / "chef.jpg"
    r = subprocess.run([CLI, C50, "-to_jpeg", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    want = J.export(f.data, f.width, f.height, tuple(f.params))
    got = out.read_bytes()
    assert got == want, first_difference(got, want)


def test_cli_to_jpeg_of_a_raw_file(tmp_path, golden, oracle):
    f = golden("chef-with-trumpet.myyuv")
    out = tmp_path / "chef.jpg"
    r = subprocess.run([CLI, RAW, "-to_jpeg", "-q", "50", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    pay = oracle.compress(f.data, f.width, f.height, (50, 50, 50))
    want = J.export(pay, f.width, f.height, (50, 50, 50))
    got = out.read_bytes()
    assert got == want, first_difference(got, want)

"""Region decode on the GPU (k_decode_region, csrc/k_huff_decode.hip): every
result is compared byte for byte with the numpy crop (regionref.crop) of the
ORACLE's full decode.  Frames are small; the geometries are chosen for where
the runs start and end:
  A 208x96    26x12 luma and 13x6 chroma blocks: no row length divides 64, so
              runs start mid-group and cross group boundaries;
  B 2080x32   260 / 130 blocks per row: several 64-block segments per row;
  C 1040x512  8320 + 2080 + 2080 blocks: the 4096-block scan tiles end inside
              Y and straddle the Y/U and U/V boundaries."""
import functools
import os
import subprocess

import numpy as np
import pytest

import colorref as C
import malformed
import regionref as R
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
AW, AH = 208, 96
A_ALL16 = [(x, y, 16, 16) for y in range(0, AH, 16) for x in range(0, AW, 16)]


def check(codec, pay, full, w, h, q, regions):
    for rg in regions:
        got = codec.decompress_region(pay, w, h, q, rg)
        assert got == R.crop(full, w, h, rg), rg


# ------------------------------------------------------ 1. every position, A
@pytest.mark.parametrize("q", [(50, 50, 50), (90, 90, 90), (90, 50, 20)])
def test_every_position(codec, oracle, q):
    pay, full = R.tiled_stream(AW, AH, q)
    assert len(A_ALL16) == 78
    check(codec, pay, full, AW, AH, q, A_ALL16 + [(0, 0, AW, AH), (96, 32, 112, 64)])
    assert codec.decompress_region(pay, AW, AH, q, (0, 0, AW, AH)) == full


# ------------------------------------------- 2. more than one staging round
def test_noise(codec, oracle):
    """q100 noise, about 133 B a chunk.  Frame A's runs are at most 26 blocks
    (3.4 KB: one staging round each, of long chunks at every alignment); the
    1040x32 frame's 64-block runs hold 8.5 KB, more than the 5.1 KB window, so
    they take two rounds."""
    q = (100, 100, 100)
    pay, full = R.noise_stream(AW, AH)
    check(codec, pay, full, AW, AH, q, [(0, 0, AW, AH), (0, 16, AW, 16), (0, 80, AW, 16), (0, 32, AW, 48),
                                         (64, 32, 64, 32)])
    w, h = 1040, 32
    pay, full = R.noise_stream(w, h)
    nblk = int.from_bytes(pay[12:16], "little")
    sizes = pay[20:20 + nblk]
    assert nblk == 130 * 4 and min(sum(sizes[k:k + 64]) for k in range(0, nblk - 64)) > 5104
    check(codec, pay, full, w, h, q, [(0, 0, w, h), (16, 0, 1024, 16), (0, 16, 528, 16), (512, 0, 528, 32)])


# --------------------------------------------------------------- 3. segments
def test_rows_of_several_segments(codec, oracle):
    w, h, q = 2080, 32, (50, 50, 50)
    pay, full = R.tiled_stream(w, h, q)
    # luma runs of 256 blocks (4 segments), chroma of 128 (2); then 64 + 64 + 2 and 64 + 1
    check(codec, pay, full, w, h, q, [(16, 0, 2048, 32), (0, 16, 1040, 16), (0, 0, w, h), (1040, 0, 1040, 16)])


# ------------------------------------------ 4. scan-tile and plane boundaries
CW, CH = 1040, 512


def test_scan_tile_and_plane_boundaries(codec, oracle):
    q = (50, 50, 50)
    pay, full = R.tiled_stream(CW, CH, q)
    assert R.blocks(CW, CH) == (8320, 2080, 2080)
    # frame blocks 4095 | 4096: luma row 31, columns 65 | 66; 8191 | 8192: luma
    # row 63, columns 1 | 2; 12287 | 12288 (a tile boundary inside V): V row 29,
    # columns 2 | 3, luma rows 464..479
    regions = [(512, 240, 32, 16), (0, 240, CW, 16), (0, 496, 48, 16), (0, 496, CW, 16), (0, 464, 112, 16),
               (0, 464, CW, 48)]
    for g, rg in ((4095, regions[0]), (4096, regions[0]), (8191, regions[2]), (8192, regions[2]),
                  (12287, regions[4]), (12288, regions[4])):
        assert R.contains_block(CW, CH, rg, g), (g, rg)
    check(codec, pay, full, CW, CH, q, regions)


def test_random_regions(codec, oracle):
    q = (50, 50, 50)
    pay, full = R.tiled_stream(CW, CH, q)
    rng = np.random.default_rng(20240)
    regions = []
    for _ in range(40):
        rw = 16 * int(rng.integers(1, CW // 16 + 1))
        rh = 16 * int(rng.integers(1, CH // 16 + 1))
        regions.append((16 * int(rng.integers(0, (CW - rw) // 16 + 1)), 16 * int(rng.integers(0, (CH - rh) // 16 + 1)),
                        rw, rh))
    check(codec, pay, full, CW, CH, q, regions)


# ------------------------------------------------------ 5. irregular tables
def replaced_block(clean, changed):
    """Index (plane 0) of the one chunk malformed._replace_chunk rewrote."""
    nblk = int.from_bytes(clean[12:16], "little")
    sizes = clean[20:20 + nblk]
    first = next(i for i in range(len(clean)) if clean[i] != changed[i])
    off = 20 + nblk
    for k in range(nblk):
        if off <= first < off + sizes[k]:
            return k
        off += sizes[k]
    raise AssertionError("the change is outside plane 0's chunks")


def test_irregular_tables(codec, oracle):
    """Valid streams with tables the encoder never writes (decode_general), in
    frame A's q100 streams (the cases need a chunk of about 130 B): the noise
    frame's block 0, the chef window's blocks 0 and 13."""
    q = (100, 100, 100)
    seen = set()
    for pay in (R.noise_stream(AW, AH)[0], R.tiled_stream(AW, AH, q)[0]):
        for name, p in malformed.irregular_cases(pay):
            full = oracle.decompress(p, AW, AH, q)
            k = replaced_block(pay, p)
            seen.add(k)
            rg = R.block_rect(AW, AH, 0, k)
            assert R.contains_block(AW, AH, rg, k)
            # the block's 16x16, its block rows, the whole frame
            check(codec, p, full, AW, AH, q, [rg, (0, rg[1], AW, 16), (0, 0, AW, AH)])
    assert seen == {0, 13}


def test_many_irregular_tables_in_one_run(codec, oracle):
    """20 of a run's 26 blocks take the bit-serial path, which the kernel runs
    16 lanes at a time."""
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
    p = bytes(p)
    full = oracle.decompress(p, AW, AH, q)
    assert full != oracle.decompress(pay, AW, AH, q)
    check(codec, p, full, AW, AH, q, [(0, 0, AW, 16), (16, 0, 176, 32), (0, 0, AW, AH)])
    assert codec.decompress(p, AW, AH, q) == full


# ------------------------------------------------------------------ 6. errors
def full_error(codec, payload, w, h, q):
    import myyuv_hip

    with pytest.raises(myyuv_hip.CodecError) as e:
        codec.decompress(payload, w, h, q)
    return e.value.code, e.value.bad_block


def region_error(codec, payload, w, h, q, rg):
    import myyuv_hip

    with pytest.raises(myyuv_hip.CodecError) as e:
        codec.decompress_region(payload, w, h, q, rg)
    return e.value.code, e.value.bad_block


def test_stream_errors(codec, oracle):
    q = (50, 50, 50)
    pay, full = R.tiled_stream(AW, AH, q)
    seen = set()
    for name, p, _kind in malformed.cases(pay):
        seen.add(name)
        want = full_error(codec, p, AW, AH, q)
        if name in ("tiny", "truncated", "plane_size_zero"):  # header errors: whatever the region
            for rg in ((0, 0, 16, 16), (96, 32, 112, 64)):
                assert region_error(codec, p, AW, AH, q, rg) == want, (name, rg)
        elif name in ("bad_code", "unknown_symbol"):
            k = replaced_block(pay, p)
            assert want[1] == k
            inside = R.block_rect(AW, AH, 0, k)
            for rg in (inside, (0, 0, AW, AH), (0, inside[1], AW, 16)):
                assert region_error(codec, p, AW, AH, q, rg) == want, (name, rg)
            # a region without the block decodes: every other byte is the clean stream's
            for rg in A_ALL16:
                if not R.contains_block(AW, AH, rg, k):
                    assert codec.decompress_region(p, AW, AH, q, rg) == R.crop(full, AW, AH, rg), (name, rg)
        elif name == "content_too_small":
            for rg in ((0, 0, 16, 16), (0, 0, AW, AH)):
                assert region_error(codec, p, AW, AH, q, rg) == want, (name, rg)
        elif name == "nbits_past_chunk":  # block 0
            assert region_error(codec, p, AW, AH, q, (0, 0, 16, 16)) == want
            assert codec.decompress_region(p, AW, AH, q, (16, 0, 16, 16)) == R.crop(full, AW, AH, (16, 0, 16, 16))
    assert {"tiny", "truncated", "plane_size_zero", "bad_code", "unknown_symbol", "content_too_small"} <= seen
    # the context still works
    assert codec.decompress_region(pay, AW, AH, q, (96, 32, 112, 64)) == R.crop(full, AW, AH, (96, 32, 112, 64))


def test_lowest_bad_block_wins(codec, oracle):
    """Two bad chunks in the region: the lower index is reported; a region
    holding only the higher one reports that one."""
    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    one = malformed._replace_chunk(pay, malformed._bits_run_out)
    k0 = replaced_block(pay, one)
    nblk = int.from_bytes(pay[12:16], "little")
    sizes = pay[20:20 + nblk]
    # a second one two block rows further down (outside the first one's 16x16)
    k1 = next(k for k in range((k0 // 26 + 2) * 26, nblk) if sizes[k] >= 12)
    off = 20 + nblk + sum(sizes[:k1])
    two = bytearray(one)
    two[off:off + sizes[k1]] = malformed._unknown_symbol(bytes(two[off:off + sizes[k1]]), sizes[k1])
    two = bytes(two)
    assert full_error(codec, two, AW, AH, q) == (10, k0)
    assert region_error(codec, two, AW, AH, q, (0, 0, AW, AH)) == (10, k0)
    assert region_error(codec, two, AW, AH, q, R.block_rect(AW, AH, 0, k1)) == (11, k1)


@pytest.mark.parametrize("rg", [(8, 0, 16, 16), (0, 8, 16, 16), (0, 0, 24, 16), (0, 0, 16, 24), (0, 0, 0, 16),
                                (0, 0, 16, 0), (AW, 0, 16, 16), (200, 0, 16, 16), (0, AH, 16, 16), (0, 64, 16, 48),
                                (0xFFFFFFF0, 0, 32, 16), (0, 0xFFFFFFF0, 16, 32)])
def test_region_arguments(codec, rg):
    import myyuv_hip

    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    out = np.full(AW * AH * 3 // 2, 0xA5, np.uint8)
    with pytest.raises(myyuv_hip.CodecError) as e:
        codec.decompress_region_into(np.frombuffer(pay, np.uint8), AW, AH, q, rg, out)
    assert (e.value.code, e.value.bad_block) == (myyuv_hip.E_ARG, -1)
    assert (out == 0xA5).all()
    with pytest.raises(myyuv_hip.CodecError) as e:
        codec.decompress_region_to_bmp(pay, AW, -AH, q, rg)
    assert e.value.code == myyuv_hip.E_ARG


def test_region_check_comes_last(codec):
    """Quality, stream header and % 8 dimension errors win over a bad region."""
    import myyuv_hip

    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    bad_rg = (8, 0, 16, 16)
    for args, code in (((pay, AW, AH, (0, 50, 50), bad_rg), myyuv_hip.E_QUALITY),
                       ((pay[:8], AW, AH, q, bad_rg), myyuv_hip.E_DCTYUV_SIZE),
                       ((pay, 204, AH, q, bad_rg), myyuv_hip.E_WIDTH),
                       ((pay, AW, 100, q, bad_rg), myyuv_hip.E_HEIGHT)):
        with pytest.raises(myyuv_hip.CodecError) as e:
            codec.decompress_region(*args)
        assert e.value.code == code, args[1:]


# ------------------------------------------------------------ 7. device batch
def test_device_batch(codec, oracle):
    import torch

    q = (50, 50, 50)
    rg = (32, 16, 128, 64)
    three = [R.tiled_stream(AW, AH, q), R.tiled_stream(AW, AH, q, 0, 0), R.tiled_stream(AW, AH, q, 120, 500)]
    streams, fulls = [t[0] for t in three], [t[1] for t in three]
    assert len(set(streams)) == 3
    nf, rb = 3, rg[2] * rg[3] * 3 // 2
    cap = (max(len(s) for s in streams) + 3) & ~3
    stream = torch.cuda.current_stream().cuda_stream

    def run(payloads):
        buf = bytearray(nf * cap)
        for f, s in enumerate(payloads):
            buf[f * cap:f * cap + len(s)] = s
        d_pay = torch.frombuffer(buf, dtype=torch.uint8).cuda()
        d_sizes = torch.tensor([len(s) for s in payloads], dtype=torch.int32, device="cuda")
        d_out = torch.full((nf * rb + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        codec.decompress_region_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, nf, AW, AH, q, rg,
                                       d_out.data_ptr(), stream)
        rc, bad = codec.sync_status(stream)
        return rc, bad, bytes(d_out.cpu().numpy())

    rc, bad, out = run(streams)
    assert (rc, bad) == (0, -1)
    for f in range(nf):
        assert out[f * rb:(f + 1) * rb] == R.crop(fulls[f], AW, AH, rg), f
        assert out[f * rb:(f + 1) * rb] == codec.decompress_region(streams[f], AW, AH, q, rg), f
    assert out[nf * rb:] == b"\x5A" * 256  # nothing past the last region frame
    # a bad chunk inside frame 1's region
    nblk = int.from_bytes(streams[1][12:16], "little")
    sizes = streams[1][20:20 + nblk]
    k = next(k for k in range(nblk) if sizes[k] >= 12 and R.contains_block(AW, AH, rg, k))
    off = 20 + nblk + sum(sizes[:k])
    p1 = bytearray(streams[1])
    p1[off:off + sizes[k]] = malformed._bits_run_out(bytes(p1[off:off + sizes[k]]), sizes[k])
    rc, bad, _ = run([streams[0], bytes(p1), streams[2]])
    assert (rc, bad) == (10, 1 * sum(R.blocks(AW, AH)) + k)
    # ... and outside it: the batch decodes
    k2 = next(k for k in range(nblk) if sizes[k] >= 12 and not R.contains_block(AW, AH, rg, k))
    off = 20 + nblk + sum(sizes[:k2])
    p2 = bytearray(streams[1])
    p2[off:off + sizes[k2]] = malformed._bits_run_out(bytes(p2[off:off + sizes[k2]]), sizes[k2])
    rc, bad, out2 = run([streams[0], bytes(p2), streams[2]])
    assert (rc, bad) == (0, -1) and out2 == out


# ------------------------------------------------------------------ 8. to BMP
@pytest.mark.parametrize("bits", [24, 32])
@pytest.mark.parametrize("mode", [C.NEAREST, C.LINEAR])
def test_region_to_bmp(codec, oracle, bits, mode):
    q = (50, 50, 50)
    pay, full = R.tiled_stream(AW, AH, q)
    for rg in ((96, 32, 112, 64), (0, 0, AW, AH), (16, 80, 16, 16)):
        rx, ry, rw, rh = rg
        part = R.crop(full, AW, AH, rg)
        for sw, sh in C.ORIENTS:
            got = codec.decompress_region_to_bmp(pay, sw * AW, sh * AH, q, rg, bits, mode)
            assert got == codec.iyuv_to_bmp(part, sw * rw, sh * rh, bits, mode), (rg, sw, sh)
            assert got == C.to_bmp(part, sw * rw, sh * rh, bits, mode), (rg, sw, sh)
            if mode == C.NEAREST:  # the crop of the whole picture (top-down rows), put in the same orientation
                pic = np.frombuffer(codec.decompress_to_bmp(pay, AW, -AH, q, bits, mode), np.uint8)
                cut = pic.reshape(AH, AW, bits // 8)[ry:ry + rh, rx:rx + rw]
                assert got == np.ascontiguousarray(C.orient(cut, sw * rw, sh * rh)).tobytes(), (rg, sw, sh)


# --------------------------------------------------------------------- 9. CLI
def test_cli_crop(codec, tmp_path, golden):
    import myyuv_file

    f = golden("chef-with-trumpet-DCT-50.myyuv")
    q = tuple(f.params)
    rg = (496, 368, 256, 128)
    args = [str(v) for v in rg]
    out = tmp_path / "crop.myyuv"
    r = subprocess.run([CLI, C50, "-decompress", "-crop", *args, "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    part = codec.decompress_region(f.data, f.width, f.height, q, rg)
    assert out.read_bytes() == myyuv_file.YUVFile(f.fourcc, rg[2], rg[3], myyuv_file.NONE, b"", part, f.unused).dumps()
    for opts, bits, mode in (([], 32, C.LINEAR), (["24", "-chroma", "nearest"], 24, C.NEAREST)):
        bmp = tmp_path / f"crop{bits}.bmp"
        r = subprocess.run([CLI, C50, "-to_bmp", *opts, "-crop", *args, "-o", str(bmp)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
        want = codec.decompress_region_to_bmp(f.data, f.width, f.height, q, rg, bits, mode)
        assert bmp.read_bytes() == myyuv_file.BMPFile(rg[2], rg[3], bits, want).dumps()


def test_kernel_stats_name_the_region_kernel(codec):
    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    codec.profile(True, ["decode_region", "huff_decode"])
    try:
        for _ in range(2):
            codec.decompress_region(pay, AW, AH, q, (0, 0, 16, 16))
        stats = codec.kernel_stats()
    finally:
        codec.profile(False)
    assert stats["decode_region"][1] == 2 and stats["decode_region"][0] > 0
    assert stats["huff_decode"][1] == 0  # the full decoders are not run

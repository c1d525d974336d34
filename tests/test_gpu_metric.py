"""Compare on the GPU (k_decode_compare, csrc/k_huff_decode.hip; k_frame_compare,
csrc/k_color.hip): every result is compared as integers — the three plane
records and the whole per-block map — with the exact-integer restatement
(metricref) of the definition in include/myyuv_hip.h, applied to the oracle's
decode of the stream.  Every call is made twice on one context (a stale
accumulator shows on the second), with and without the map, and the fused
result, the raw-against-raw kernel on the decoded frame and metricref must all
agree.  Frames are small; the geometries are those of tests/test_gpu_scaled.py:
  16x16      one luma group of 4 lanes; 1-block chroma planes;
  208x96     26 and 13 blocks per row: groups wrap block rows mid-wave;
  2080x32    several groups per block row;
  1040x512   the 4096-block scan tiles end inside Y and straddle the plane
             boundaries; more than one 16-block unit per group."""
import functools
import os
import subprocess

import numpy as np
import pytest

import coefgen
import malformed
import metricref as M
import regionref as R
import synth
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
C90 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-90.myyuv")
AW, AH = 208, 96


@functools.lru_cache(maxsize=None)
def want(ref, test, w, h):
    """metricref's (records, map) of two frames (bytes), computed once."""
    return M.frame_metric(ref, test, w, h)


def source_pixels(w, h, ox=400, oy=300):
    f = R.chef()
    return synth.tiled_frame(f.data, f.width, f.height, w, h, ox, oy).tobytes()


def noise(w, h, seed=77):
    return synth.noise_frame(w, h, seed).tobytes()


def same_map(got, exp):
    return got.dtype == exp.dtype and got.tobytes() == exp.tobytes()


def first_difference(got, exp):
    d = np.nonzero((got["sse"] != exp["sse"]) | (got["ssim"] != exp["ssim"]))[0]
    return (int(d[0]), got[d[0]].tolist(), exp[d[0]].tolist(), len(d)) if len(d) else None


def check(codec, pay, dec, w, h, q, refs):
    """The stream `pay` (its oracle decode: dec) against each reference."""
    pay, dec = bytes(pay), bytes(dec)
    for name, ref in refs:
        recs, bmap = want(bytes(ref), dec, w, h)
        for rep in range(2):
            got, gmap = codec.compare_stream(pay, w, h, q, ref, want_map=True)
            assert got == recs, (name, rep, got, recs)
            assert same_map(gmap, bmap), (name, rep, first_difference(gmap, bmap))
            assert codec.compare_stream(pay, w, h, q, ref) == recs, (name, rep, "no map")
        # raw against raw on the decoded frame: the unfused kernel, and in both directions
        got, gmap = codec.compare_frames(ref, dec, w, h, want_map=True)
        assert got == recs and same_map(gmap, bmap), (name, "frames", first_difference(gmap, bmap))
        assert codec.compare_frames(dec, ref, w, h) == recs, (name, "frames swapped")
        if ref == dec:
            ny, nc, _ = R.blocks(w, h)
            assert recs == ((0, ny * M.ONE, ny, 0), (0, nc * M.ONE, nc, 0), (0, nc * M.ONE, nc, 0))


def three_refs(w, h, dec, ox=400, oy=300):
    return [("source", source_pixels(w, h, ox, oy)), ("own decode", bytes(dec)), ("noise", noise(w, h))]


# ---------------------------------------------------------------- geometries
def test_one_small_group(codec, oracle):
    w, h, q = 16, 16, (50, 50, 50)
    pay, dec = R.tiled_stream(w, h, q)
    check(codec, pay, dec, w, h, q, three_refs(w, h, dec))


@pytest.mark.parametrize("q", [(50, 50, 50), (90, 90, 90), (90, 50, 20)])
def test_rows_that_divide_no_group(codec, oracle, q):
    pay, dec = R.tiled_stream(AW, AH, q)
    check(codec, pay, dec, AW, AH, q, three_refs(AW, AH, dec))


def test_several_groups_per_block_row(codec, oracle):
    w, h, q = 2080, 32, (50, 50, 50)
    pay, dec = R.tiled_stream(w, h, q)
    check(codec, pay, dec, w, h, q, three_refs(w, h, dec))


def test_scan_tile_and_plane_boundaries(codec, oracle):
    w, h, q = 1040, 512, (50, 50, 50)
    assert R.blocks(w, h) == (8320, 2080, 2080)
    pay, dec = R.tiled_stream(w, h, q)
    check(codec, pay, dec, w, h, q, three_refs(w, h, dec))


def test_noise_two_staging_rounds(codec, oracle):
    """q100 noise, about 133 B a chunk: a 64-block group takes two rounds of
    the 5.1 KB stage (tests/test_gpu_scaled.py asserts the sizes)."""
    q = (100, 100, 100)
    for w, h in ((AW, AH), (1040, 32)):
        pay, dec = R.noise_stream(w, h)
        check(codec, pay, dec, w, h, q, [("source", synth.noise_frame(w, h).tobytes()), ("own decode", bytes(dec)),
                                         ("noise", noise(w, h))])


def test_anticorrelated_reference_gives_negative_ssim(codec, oracle):
    """255 - decode: the covariance term is negative on every textured block,
    so the device's floor towards minus infinity is exercised."""
    q = (50, 50, 50)
    pay, dec = R.tiled_stream(AW, AH, q)
    inv = (255 - np.frombuffer(dec, np.uint8)).tobytes()
    recs, bmap = want(inv, bytes(dec), AW, AH)
    assert (bmap["ssim"] < 0).sum() > 100 and recs[0][1] < 0
    check(codec, pay, dec, AW, AH, q, [("inverse", inv)])


# -------------------------------------------- the DC-only shortcut, short units
@pytest.mark.parametrize("name", ["dc_sweep_luma_q50", "dc_sweep_chroma_q50", "group_composition_q50",
                                  "group_composition_q100", "geometry_16x16", "geometry_144x272", "extreme_q1"])
def test_coefficient_domain_streams(codec, oracle, name):
    """coefgen.decoder_streams: frames whose blocks are all DC-only (the
    shortcut alone), 64-block groups with exactly 0, 1, 7, 8, 9, 56, 57, 63 and
    64 blocks that are not (the 8-block unit with fewer than 8 blocks left, the
    16-block units), odd geometries, the clamp."""
    sh = coefgen.shared(oracle)
    s = sh.by_name[name]
    pay, dec = sh.decoded(name)
    check(codec, pay, dec, s.w, s.h, s.q, [("own decode", bytes(dec)), ("noise", noise(s.w, s.h))])


def test_irregular_tables(codec, oracle):
    """Valid streams with tables the encoder never writes: their blocks go
    through the coefficient buffer (decode_general)."""
    q = (100, 100, 100)
    n = 0
    for pay in (R.noise_stream(AW, AH)[0], R.tiled_stream(AW, AH, q)[0]):
        for name, p in malformed.irregular_cases(pay):
            dec = oracle.decompress(p, AW, AH, q)
            assert dec != oracle.decompress(pay, AW, AH, q), name
            check(codec, p, dec, AW, AH, q, [("own decode", bytes(dec)), ("noise", noise(AW, AH))])
            n += 1
    assert n == 4


# ------------------------------------------------------------- 64-bit totals
@functools.lru_cache(maxsize=None)
def flat_zero_stream():
    """1040x512, every block DC-only with the lowest DC: decodes to flat 0."""
    from oracle import oracle as O

    w, h, q = 1040, 512, (50, 50, 50)
    b = np.zeros(64, np.int16)
    b[0] = -1024
    pay = coefgen.build_payload([np.tile(b, (n, 1)) for n in coefgen.plane_counts(w, h)], O)
    dec = O.decompress(pay, w, h, q)
    assert dec == bytes(w * h * 3 // 2)
    return pay, dec, w, h, q


def test_luma_sse_above_32_bits(codec, oracle):
    pay, dec, w, h, q = flat_zero_stream()
    white = b"\xff" * (w * h * 3 // 2)
    recs, _ = want(white, dec, w, h)
    assert recs[0][0] == 532480 * 65025 > 1 << 32 and recs[0][3] == 255
    assert recs[0][1] == 8320 * 1677  # 0 against 255, every block
    check(codec, pay, dec, w, h, q, [("white", white)])


def test_flat_zero_against_a_stripe(codec, oracle):
    """Columns 0, 255, 0, 255 ... against flat 0 (by the definition A2 = C2
    here, so these quotients are small and positive; the negative ones are in
    test_anticorrelated_reference_gives_negative_ssim)."""
    pay, dec, w, h, q = flat_zero_stream()
    stripe = np.tile(np.array([0, 255], np.uint8), w * h * 3 // 4).tobytes()
    recs, bmap = want(stripe, dec, w, h)
    assert recs[0][0] == 532480 // 2 * 65025 and 0 < int(bmap["ssim"].max()) < M.ONE // 100
    check(codec, pay, dec, w, h, q, [("stripe", stripe)])


# -------------------------------------------------------------- device batch
def device_batch(codec, pays, refs, decs, w, h, q, with_map):
    import torch

    n, nref = len(pays), len(refs)
    nblk = sum(R.blocks(w, h))
    cap = (max(len(p) for p in pays) + 3) & ~3
    stream = torch.cuda.current_stream().cuda_stream
    buf = bytearray(n * cap)
    for f, p in enumerate(pays):
        buf[f * cap:f * cap + len(p)] = p
    d_pay = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    d_sizes = torch.tensor([len(p) for p in pays], dtype=torch.int32, device="cuda")
    d_ref = torch.frombuffer(bytearray(b"".join(refs)), dtype=torch.uint8).cuda()
    d_dec = torch.frombuffer(bytearray(b"".join(decs)), dtype=torch.uint8).cuda()
    exp = [want(bytes(refs[f % nref]), bytes(decs[f]), w, h) for f in range(n)]
    out = []
    for fused in (True, False):
        # (dirty buffers: the call clears the records itself; guard bytes behind both)
        d_out = torch.full((n * 72 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        d_map = torch.full((n * nblk * 8 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        mp = d_map.data_ptr() if with_map else None
        for rep in range(2):
            if fused:
                codec.compare_stream_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, n, w, h, q, d_ref.data_ptr(),
                                            nref, d_out.data_ptr(), mp, stream)
            else:
                codec.compare_frames_device(d_ref.data_ptr(), d_dec.data_ptr(), n, nref, w, h, d_out.data_ptr(), mp,
                                            stream)
            assert codec.sync_status(stream) == (0, -1)
            o = d_out.cpu().numpy()
            m = d_map.cpu().numpy()
            assert (o[n * 72:] == 0x5A).all() and (m[n * nblk * 8:] == 0x5A).all()
            recs = o[:n * 72].view([("sse", "<u8"), ("ssim_sum", "<i8"), ("nblocks", "<u4"), ("max_abs", "<u4")])
            for f in range(n):
                got = tuple(tuple(int(v) for v in recs[3 * f + p].tolist()) for p in range(3))
                assert got == exp[f][0], (fused, rep, f, got, exp[f][0])
                if with_map:
                    gm = m[f * nblk * 8:(f + 1) * nblk * 8].view(M.BLOCK)
                    assert same_map(gm, exp[f][1]), (fused, rep, f, first_difference(gm, exp[f][1]))
            if not with_map:
                assert (m == 0x5A).all()
        out.append(o[:n * 72].tobytes())
    assert out[0] == out[1]
    return out[0]


def test_device_batches(codec, oracle):
    q = (50, 50, 50)
    origins = ((400, 300), (96, 48), (640, 208))
    streams = [R.tiled_stream(AW, AH, q, ox, oy) for ox, oy in origins]
    pays, decs = [s[0] for s in streams], [s[1] for s in streams]
    assert len(set(pays)) == 3
    srcs = [source_pixels(AW, AH, ox, oy) for ox, oy in origins]
    a = device_batch(codec, pays, srcs, decs, AW, AH, q, True)       # pairwise
    assert device_batch(codec, pays, srcs, decs, AW, AH, q, False) == a   # a null map: the same records
    b = device_batch(codec, pays, srcs[1:2], decs, AW, AH, q, True)  # every frame against one reference
    assert device_batch(codec, pays, srcs[1:2], decs, AW, AH, q, False) == b
    assert a != b and a[72:144] == b[72:144]


def test_device_batch_with_a_rejected_frame(codec, oracle):
    """Frame 1's header is rejected (a rejected stream, not a fault): the
    error comes through sync_status with the batch-global block, frame 1's
    records are zero whatever the workspace held, frame 0's are right."""
    import torch

    q = (50, 50, 50)
    pay, dec = R.tiled_stream(AW, AH, q)
    ref = source_pixels(AW, AH)
    recs, _ = want(ref, bytes(dec), AW, AH)
    nblk = sum(R.blocks(AW, AH))
    cap = (len(pay) + 3) & ~3
    stream = torch.cuda.current_stream().cuda_stream
    d_pay = torch.frombuffer(bytearray(pay + bytes(cap - len(pay))) * 2, dtype=torch.uint8).cuda()
    d_ref = torch.frombuffer(bytearray(ref), dtype=torch.uint8).cuda()
    d_out = torch.full((2 * 72,), 0x5A, dtype=torch.uint8, device="cuda")
    for sizes, status in (((len(pay), len(pay)), (0, -1)), ((len(pay), 8), (6, nblk))):
        d_sizes = torch.tensor(sizes, dtype=torch.int32, device="cuda")
        codec.compare_stream_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 2, AW, AH, q, d_ref.data_ptr(), 1,
                                    d_out.data_ptr(), None, stream)
        assert codec.sync_status(stream) == status
        r = d_out.cpu().numpy().view([("sse", "<u8"), ("ssim_sum", "<i8"), ("nblocks", "<u4"), ("max_abs", "<u4")])
        got = [tuple(tuple(int(v) for v in r[3 * f + p].tolist()) for p in range(3)) for f in range(2)]
        assert got[0] == recs
        assert got[1] == (recs if status[0] == 0 else ((0, 0, 0, 0),) * 3)


def test_device_argument_errors(codec):
    import myyuv_hip
    import torch

    q = (50, 50, 50)
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    for nframes, ref_frames in ((3, 2), (2, 0), (1, 2)):
        with pytest.raises(myyuv_hip.CodecError) as e:
            codec.compare_stream_device(p, p, 64, nframes, 16, 16, q, p, ref_frames, p, None, None)
        assert e.value.code == myyuv_hip.E_ARG
        with pytest.raises(myyuv_hip.CodecError) as e:
            codec.compare_frames_device(p, p, nframes, ref_frames, 16, 16, p, None, None)
        assert e.value.code == myyuv_hip.E_ARG
    for args, code in (((p, p, 64, 1, 20, 16, q, p, 1, p), myyuv_hip.E_WIDTH),
                       ((p, p, 64, 1, 16, 20, q, p, 1, p), myyuv_hip.E_HEIGHT),
                       ((p, p, 64, 1, 16, 16, (0, 50, 50), p, 1, p), myyuv_hip.E_QUALITY),
                       ((p, p, 64, 1, 16, 16, q, p + 4, 1, p), myyuv_hip.E_ARG),
                       ((p, p, 64, 1, 16, 16, q, p, 1, p + 4), myyuv_hip.E_ARG)):
        with pytest.raises(myyuv_hip.CodecError) as e:
            codec.compare_stream_device(*args)
        assert e.value.code == code, args


# -------------------------------------------------------------------- errors
def error_of(fn, *args):
    import myyuv_hip

    with pytest.raises(myyuv_hip.CodecError) as e:
        fn(*args)
    return e.value


def test_malformed_streams_fail_as_the_full_decode(codec, oracle):
    """Rejected streams: the full decode's code and bad_block, the record left
    zeroed; the context works afterwards."""
    q = (50, 50, 50)
    pay, dec = R.tiled_stream(AW, AH, q)
    ref = source_pixels(AW, AH)
    seen = set()
    for name, p, _kind in malformed.cases(pay):
        seen.add(name)
        full = error_of(codec.decompress, p, AW, AH, q)
        assert full.code != 0
        for with_map in (False, True):
            e = error_of(codec.compare_stream, p, AW, AH, q, ref, with_map)
            assert (e.code, e.bad_block) == (full.code, full.bad_block), (name, with_map)
            assert e.metric == ((0, 0, 0, 0),) * 3, (name, with_map)
    assert {"tiny", "truncated", "plane_size_zero", "bad_code", "unknown_symbol", "content_too_small",
            "nbits_past_chunk"} <= seen
    check(codec, pay, dec, AW, AH, q, [("source", ref)])


def test_argument_checks_in_the_full_decodes_order(codec):
    import myyuv_hip

    q = (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, q)
    ref = source_pixels(AW, AH)
    for args, code in (((pay, AW, AH, (0, 50, 50), ref), myyuv_hip.E_QUALITY),
                       ((pay[:8], AW, AH, q, ref), myyuv_hip.E_DCTYUV_SIZE),
                       ((pay, 204, AH, q, ref), myyuv_hip.E_WIDTH),
                       ((pay, AW, 100, q, ref + bytes(4096)), myyuv_hip.E_HEIGHT)):
        e = error_of(codec.compare_stream, *args)
        assert (e.code, e.bad_block) == (code, -1) and e.metric == ((0, 0, 0, 0),) * 3
    e = error_of(codec.compare_frames, ref, ref, 204, AH)
    assert e.code == myyuv_hip.E_WIDTH


def test_kernel_stats_name_the_compare_kernels(codec):
    q = (50, 50, 50)
    pay, dec = R.tiled_stream(AW, AH, q)
    ref = source_pixels(AW, AH)
    codec.profile(True, ["decode_compare", "frame_compare", "metric_reduce", "huff_decode", "dequant_idct",
                         "scan_tiles"])
    try:
        codec.compare_stream(pay, AW, AH, q, ref)
        codec.compare_stream(pay, AW, AH, q, ref, want_map=True)
        codec.compare_frames(ref, dec, AW, AH)
        stats = codec.kernel_stats()
    finally:
        codec.profile(False)
    assert stats["decode_compare"][1] == 2 and stats["decode_compare"][0] > 0
    assert stats["frame_compare"][1] == 1 and stats["frame_compare"][0] > 0
    assert stats["scan_tiles"][1] == 2 and stats["metric_reduce"][1] == 3
    assert stats["huff_decode"][1] == 0 and stats["dequant_idct"][1] == 0  # no full decoder runs


# ----------------------------------------------------------------------- CLI
def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


@functools.lru_cache(maxsize=None)
def chef_frames():
    """(raw pixels, decode of -DCT-50, decode of -DCT-90, w, h, file fields)."""
    import myyuv_file
    from oracle import oracle as O

    raw = myyuv_file.YUVFile.load(RAW)
    out = [bytes(raw.data)]
    for path in (C50, C90):
        f = myyuv_file.YUVFile.load(path)
        assert (f.width, f.height) == (raw.width, raw.height)
        out.append(O.decompress(f.data, f.width, f.height, tuple(f.params)))
    return out[0], out[1], out[2], raw.width, raw.height, raw


def test_cli_compare(oracle, tmp_path):
    raw, d50, d90, w, h, _ = chef_frames()
    rec50, map50 = M.frame_metric(raw, d50, w, h)
    rec90, map90 = M.frame_metric(raw, d90, w, h)
    for path, recs, bmap in ((C50, rec50, map50), (C90, rec90, map90)):
        text = M.report(recs, bmap, w, h)
        rep = tmp_path / "report.txt"
        r = cli(RAW, "-compare", path, "-o", str(rep))
        assert r.returncode == 0 and r.stdout == text + "Success!\n", r.stdout + r.stderr
        assert rep.read_text() == text
        rep.unlink()
        r = cli(path, "-compare", RAW)  # swapped operands: the same figures
        assert r.returncode == 0 and r.stdout == text + "Success!\n", r.stdout + r.stderr
    samples = (w * h, w * h // 4, w * h // 4)
    for p in range(3):  # q90 is closer to the original than q50, on every plane
        assert M.psnr(rec90[p][0], samples[p]) > M.psnr(rec50[p][0], samples[p])
        assert M.ssim(rec90[p][1], rec90[p][2]) > M.ssim(rec50[p][1], rec50[p][2])
    assert len(M.report(rec50, map50, w, h).splitlines()) == 5


def test_cli_compare_raw_and_stream_pairs(oracle, tmp_path):
    import myyuv_file

    raw, d50, d90, w, h, f = chef_frames()
    dec50 = tmp_path / "dec50.myyuv"
    dec50.write_bytes(myyuv_file.YUVFile(f.fourcc, w, h, myyuv_file.NONE, b"", d50, f.unused).dumps())
    # raw against raw: the decoded q50 frame against the original equals the stream against it
    text = M.report(*M.frame_metric(raw, d50, w, h), w, h)
    for a, b in ((RAW, str(dec50)), (str(dec50), RAW)):
        r = cli(a, "-compare", b)
        assert r.returncode == 0 and r.stdout == text + "Success!\n", r.stdout + r.stderr
    # stream against stream, both orders; and a stream against its own decode
    text = M.report(*M.frame_metric(d50, d90, w, h), w, h)
    for a, b in ((C50, C90), (C90, C50)):
        r = cli(a, "-compare", b)
        assert r.returncode == 0 and r.stdout == text + "Success!\n", r.stdout + r.stderr
    r = cli(C50, "-compare", str(dec50))
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[0] == "Y: psnr inf dB ssim 1.000000 sse 0 max 0", r.stdout
    assert lines[3] == "all: psnr inf dB ssim 1.000000"
    assert lines[4] == "worst block: plane Y x 0 y 0 sse 0 ssim 1.000000"


def test_cli_compare_decode_error(tmp_path):
    """A stream that does not decode: one fixed first line, exit 1, no file."""
    import myyuv_file

    f = myyuv_file.YUVFile.load(C50)
    bad = tmp_path / "bad.myyuv"
    bad.write_bytes(myyuv_file.YUVFile(f.fourcc, f.width, f.height, myyuv_file.DCT, f.params,
                                       malformed._replace_chunk(bytes(f.data), malformed._bits_run_out),
                                       f.unused).dumps())
    rep = tmp_path / "report.txt"
    for a, b in ((RAW, str(bad)), (str(bad), RAW), (C90, str(bad))):
        r = cli(a, "-compare", b, "-o", str(rep))
        assert r.returncode == 1 and r.stdout.splitlines()[0] == "Error comparing: Huffman bad code", r.stdout
        assert not rep.exists()

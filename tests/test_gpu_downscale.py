"""Downscale on the GPU (k_downscale<N>, csrc/k_huff_decode.hip, then K2 and K4
unchanged): every output stream is compared byte for byte, no tolerance, with

    oracle.compress(scaleref.cached(payload, w, h, q_src, denom), w // denom, h // denom, q_dst)

(downscaleref.cached), twice on one context.  All streams come from
regionref.tiled_stream / noise_stream.  Geometries, for where a wave's runs and
units start and end:
  128x128 at 1/2, 1/4, 1/8   the smallest frame valid for all three; at 1/8 the
                             output is 16x16 (4 + 1 + 1 blocks) and a wave's
                             runs have 16 and 8 live lanes;
  416x192 at 1/2, 832x384 at 1/4, 1664x768 at 1/8
                             output 208x96: 26 and 13 output blocks per row, no
                             row length divides 64 and every wave has a
                             partial unit;
  2080x64 at 1/2, 2112x64 at 1/4, 2176x128 at 1/8
                             several segments per band, the last one narrow;
  1056x512 at 1/2            8448 / 2112 / 2112 source blocks: the 4096-block
                             scan tiles end inside Y and straddle both plane
                             boundaries."""
import numpy as np
import pytest

import downscaleref as D
import malformed
import regionref as R
import scaleref as S

pytestmark = pytest.mark.gpu

Q50 = (50, 50, 50)
Q100 = (100, 100, 100)
# the three sources of a 208x96 output
OUT_208x96 = [(416, 192, 2), (832, 384, 4), (1664, 768, 8)]


def first_difference(a, b):
    n = min(len(a), len(b))
    x, y = np.frombuffer(a[:n], np.uint8), np.frombuffer(b[:n], np.uint8)
    d = np.nonzero(x != y)[0]
    return (len(a), len(b), int(d[0]) if len(d) else None, len(d))


def check(codec, pay, w, h, qs, denom, qd):
    want = D.cached(bytes(pay), w, h, tuple(qs), denom, tuple(qd))
    for rep in range(2):
        got = codec.downscale(pay, w, h, qs, denom, qd)
        assert got == want, (w, h, qs, denom, qd, rep, first_difference(got, want))
    return want


def error_of(fn, *args):
    import myyuv_hip

    with pytest.raises(myyuv_hip.CodecError) as e:
        fn(*args)
    return e.value.code, e.value.bad_block


def luma_sizes(pay):
    nblk = int.from_bytes(pay[12:16], "little")
    return nblk, pay[20:20 + nblk]


# ---------------------------------------------------------------- geometries
@pytest.mark.parametrize("denom", D.DENOMS)
def test_smallest_frame(codec, oracle, denom):
    check(codec, R.tiled_stream(128, 128, Q50)[0], 128, 128, Q50, denom, Q50)


@pytest.mark.parametrize("w,h,denom", OUT_208x96)
def test_rows_that_divide_no_unit(codec, oracle, w, h, denom):
    check(codec, R.tiled_stream(w, h, Q50)[0], w, h, Q50, denom, Q50)


@pytest.mark.parametrize("w,h,denom", [(2080, 64, 2), (2112, 64, 4), (2176, 128, 8)])
def test_several_segments_per_band(codec, oracle, w, h, denom):
    assert -(-(w // 8) // 64) > 1 and (w // 8) % 64 in (4, 8, 16)  # the last luma segment is narrow
    check(codec, R.tiled_stream(w, h, Q50)[0], w, h, Q50, denom, Q50)


def test_scan_tile_and_plane_boundaries(codec, oracle):
    w, h = 1056, 512
    assert R.blocks(w, h) == (8448, 2112, 2112)
    check(codec, R.tiled_stream(w, h, Q50)[0], w, h, Q50, 2, Q50)


def test_416x96_at_half_is_a_valid_208x48_frame(codec, oracle):
    """416 x 96 at 1/2 is a 208 x 48 frame: 96 = 16 * 2 * 3, so compress takes
    a frame of that size (planes of 26 x 6 and 13 x 3 blocks) and the rule of
    include/myyuv_hip.h (the codes compress gives for the scaled size) gives no
    error.  The bytes are the definition's; test_argument_checks_and_their_order
    has a height that compress does refuse."""
    check(codec, R.tiled_stream(416, 96, Q50)[0], 416, 96, Q50, 2, Q50)


# ----------------------------------------------------------------- qualities
@pytest.mark.parametrize("w,h,denom", OUT_208x96)
@pytest.mark.parametrize("qs,qd", [(Q50, Q50), ((90, 50, 20), (20, 60, 100)), (Q50, Q100), (Q50, (1, 1, 1))])
def test_quality_pairs(codec, oracle, w, h, denom, qs, qd):
    want = check(codec, R.tiled_stream(w, h, qs)[0], w, h, qs, denom, qd)
    nblk, sizes = luma_sizes(want)
    assert nblk == 26 * 12
    if qd == Q100:  # long chunks: K2's overflow tiers write them
        assert max(sizes) > 100
    if qd == (1, 1, 1):  # 7-byte single-class chunks
        assert min(sizes) == 7


def test_noise_to_q1_is_nearly_all_single_class(codec, oracle):
    """The q50 noise frame at 1/2 to q1: in the reference's stream 304 of the
    312 luma blocks are single-class (nothing but a DC: a 7-byte chunk in closed
    form, K2 builds nothing for them)."""
    w, h = 416, 192
    want = check(codec, R.noise_stream(w, h, Q50)[0], w, h, Q50, 2, (1, 1, 1))
    luma = S.coefficients(want)[0]
    assert len(luma) == 312 and int((~(luma[:, 1:] != 0).any(axis=1)).sum()) == 304


def test_noise_to_q100_takes_the_exact_path_and_the_overflow_tiers(codec, oracle):
    w, h = 416, 192
    want = check(codec, R.noise_stream(w, h, Q50)[0], w, h, Q50, 2, Q100)
    assert max(luma_sizes(want)[1]) > 100


def test_noise_two_staging_rounds(codec, oracle):
    """q100 noise, about 133 B a chunk: a run of 52 luma chunks holds more than
    the 5.1 KB stage, so every luma run takes two staging rounds."""
    w, h = 416, 192
    pay, _ = R.noise_stream(w, h)
    nblk, sizes = luma_sizes(pay)
    bw = w // 8
    assert min(sum(sizes[k:k + bw]) for k in range(0, nblk, bw)) > 5104
    for qd in (Q100, Q50):
        check(codec, pay, w, h, Q100, 2, qd)


# ----------------------------------------------------------- irregular tables
def test_irregular_tables(codec, oracle):
    """Valid streams with tables the encoder never writes (decode_general_to,
    in the value-position table in LDS)."""
    w, h = 416, 192
    n = 0
    for pay in (R.noise_stream(w, h)[0], R.tiled_stream(w, h, Q100)[0]):
        for name, p in malformed.irregular_cases(pay):
            assert p != pay
            assert S.cached(p, w, h, Q100, 2) != S.cached(pay, w, h, Q100, 2), name
            check(codec, p, w, h, Q100, 2, Q50)
            n += 1
    assert n == 4


def test_many_irregular_tables_in_both_rows_of_a_band(codec, oracle):
    w, h = 416, 192
    pay, _ = R.noise_stream(w, h)
    nblk, sizes = luma_sizes(pay)
    bw = w // 8
    groups = [(3, [-7]), (1, [0]), (3, [1023]), (2, [-1024])]
    p = bytearray(pay)
    for row in (2, 3):  # the two rows of band 1 at 1/2
        for k in range(row * bw + 3, row * bw + 23):  # more than 16: two rounds of the bit-serial path
            off = 20 + nblk + sum(sizes[:k])
            seq = [0, -7, 1023, 0, -1024, 0, 0, -7, -1024, 1023][: 1 + k % 10] * 3
            p[off:off + sizes[k]] = malformed._irregular_chunk(groups, seq, sizes[k])
    p = bytes(p)
    assert S.cached(p, w, h, Q100, 2) != S.cached(pay, w, h, Q100, 2)
    check(codec, p, w, h, Q100, 2, Q50)
    check(codec, p, w, h, Q100, 2, Q100)


# -------------------------------------------------------------------- errors
def test_bad_chunk_in_the_second_row_of_a_band(codec, oracle):
    w, h = 416, 192
    pay, _ = R.tiled_stream(w, h, Q50)
    nblk, sizes = luma_sizes(pay)
    bw = w // 8
    k = next(k for k in range(bw + 5, 2 * bw) if sizes[k] >= 12)  # block row 1: run 1 of band 0 at 1/2
    off = 20 + nblk + sum(sizes[:k])
    p = bytearray(pay)
    p[off:off + sizes[k]] = malformed._bits_run_out(bytes(p[off:off + sizes[k]]), sizes[k])
    p = bytes(p)
    want = error_of(codec.decompress, p, w, h, Q50)
    assert want == (10, k)
    assert error_of(codec.downscale, p, w, h, Q50, 2, Q50) == want
    # a second bad chunk further on: the lowest block wins, whatever order the waves run in
    k2 = next(k for k in range(5 * bw, nblk) if sizes[k] >= 12)
    off = 20 + nblk + sum(sizes[:k2])
    two = bytearray(p)
    two[off:off + sizes[k2]] = malformed._unknown_symbol(bytes(two[off:off + sizes[k2]]), sizes[k2])
    assert error_of(codec.downscale, bytes(two), w, h, Q50, 2, Q50) == want
    check(codec, pay, w, h, Q50, 2, Q50)  # the context still works


def test_bad_chunk_in_a_later_row_of_a_band_at_every_denom(codec, oracle):
    """128 x 128: block row 1 is run 1 of band 0 at every denom."""
    w, h = 128, 128
    pay, _ = R.tiled_stream(w, h, Q50)
    nblk, sizes = luma_sizes(pay)
    k = next(k for k in range(16 + 3, 32) if sizes[k] >= 12)
    off = 20 + nblk + sum(sizes[:k])
    p = bytearray(pay)
    p[off:off + sizes[k]] = malformed._unknown_symbol(bytes(p[off:off + sizes[k]]), sizes[k])
    p = bytes(p)
    want = error_of(codec.decompress, p, w, h, Q50)
    assert want == (11, k)
    for denom in D.DENOMS:
        assert error_of(codec.downscale, p, w, h, Q50, denom, Q50) == want, denom


def test_malformed_streams_fail_as_the_full_decode(codec, oracle):
    w, h = 128, 128  # (valid at every denom: a chunk's error is found on the device, after the size checks)
    pay, _ = R.tiled_stream(w, h, Q50)
    seen = set()
    for name, p, _kind in malformed.cases(pay):
        seen.add(name)
        want = error_of(codec.decompress, p, w, h, Q50)
        assert want[0] != 0
        for denom in D.DENOMS:
            assert error_of(codec.downscale, p, w, h, Q50, denom, (30, 30, 30)) == want, (name, denom)
    assert {"tiny", "truncated", "plane_size_zero", "bad_code", "unknown_symbol", "content_too_small",
            "nbits_past_chunk"} <= seen
    check(codec, pay, w, h, Q50, 2, Q50)


def test_argument_checks_and_their_order(codec, oracle):
    import myyuv_hip

    w, h = 416, 192
    pay, _ = R.tiled_stream(w, h, Q50)
    E = myyuv_hip
    assert error_of(codec.downscale, pay, w, h, Q50, 3, Q50) == (E.E_ARG, -1)
    for denom in (0, 1, 5, 16, 0xFFFFFFFF):
        assert error_of(codec.downscale_into, np.frombuffer(pay, np.uint8).copy(), w, h, Q50, denom, Q50,
                        np.zeros(64, np.uint8)) == (E.E_ARG, -1), denom
    # the scaled size, as compress checks a frame of it
    assert error_of(codec.downscale, R.tiled_stream(208, 96, Q50)[0], 208, 96, Q50, 2, Q50) == (E.E_WIDTH, -1)
    assert error_of(codec.downscale, R.tiled_stream(416, 80, Q50)[0], 416, 80, Q50, 2, Q50) == (E.E_HEIGHT, -1)
    assert error_of(codec.downscale, pay, w, h, Q50, 4, Q50) == (E.E_WIDTH, -1)  # 104 x 48
    assert error_of(codec.downscale, pay, w, h, Q50, 2, (0, 50, 50)) == (E.E_QUALITY, -1)
    assert error_of(codec.downscale, pay, w, h, Q50, 2, (50, 50, 101)) == (E.E_QUALITY, -1)
    # the order: q_src, the stream, the dimensions, q_dst, denom, the scaled size
    for args, code in (((pay, w, h, (0, 50, 50), 3, (0, 0, 0)), E.E_QUALITY),
                       ((pay[:8], w, h, Q50, 3, (0, 0, 0)), E.E_DCTYUV_SIZE),
                       ((pay, 412, h, Q50, 3, (0, 0, 0)), E.E_WIDTH),
                       ((pay, w, 196, Q50, 3, (0, 0, 0)), E.E_HEIGHT),
                       ((pay, w, h, Q50, 3, (0, 0, 0)), E.E_QUALITY),
                       ((R.tiled_stream(208, 96, Q50)[0], 208, 96, Q50, 3, Q50), E.E_ARG)):
        assert error_of(codec.downscale, *args) == (code, -1), args[1:]


def test_capacity(codec, oracle):
    import myyuv_hip

    w, h, qs, qd = 416, 192, (90, 90, 90), Q50
    pay, _ = R.tiled_stream(w, h, qs)
    want = D.cached(pay, w, h, qs, 2, qd)
    src = np.frombuffer(pay, np.uint8).copy()
    short = np.full(len(want) - 1 + 64, 0x5A, np.uint8)  # `cap` one byte short, a canary after it
    with pytest.raises(myyuv_hip.CodecError) as e:
        codec.downscale_into(src, w, h, qs, 2, qd, short[:len(want) - 1])
    assert (e.value.code, e.value.bad_block, e.value.need) == (myyuv_hip.E_CAPACITY, -1, len(want))
    assert (short[len(want) - 1:] == 0x5A).all()
    exact = np.full(len(want), 0x5A, np.uint8)
    assert codec.downscale_into(src, w, h, qs, 2, qd, exact) == len(want) and exact.tobytes() == want
    full = np.full(myyuv_hip.payload_bound(w // 2, h // 2) + 64, 0x5A, np.uint8)
    n = codec.downscale_into(src, w, h, qs, 2, qd, full)
    assert full[:n].tobytes() == want and (full[n:] == 0x5A).all()


# -------------------------------------------------------------- device batch
def batch_buffers(pays, cap_out, guard=256, pad=0):
    import torch

    cap = ((max(len(p) for p in pays) + 3) & ~3) + pad
    buf = bytearray(len(pays) * cap)
    for f, p in enumerate(pays):
        buf[f * cap:f * cap + len(p)] = p
    d_pay = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    d_sizes = torch.tensor([len(p) for p in pays], dtype=torch.int32, device="cuda")
    d_out = torch.full((len(pays) * cap_out + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    d_osz = torch.full((len(pays),), -1, dtype=torch.int32, device="cuda")
    return cap, d_pay, d_sizes, d_out, d_osz


def test_truncated_frame_0_leaves_frame_1_whole(oracle):
    """A two-frame device batch on a FRESH context (its workspace holds
    whatever the allocator returned) where k_scan_chain rejects frame 0's
    header: every output block of frame 0 must still get its mask and info word
    (the zero-block rule), or K2 would index by stale words.  The call reports
    frame 0's error; frame 1 is its single-frame result."""
    import myyuv_hip
    import torch

    w, h, qs, qd, denom = 416, 192, Q50, (30, 30, 30), 2
    good, _ = R.tiled_stream(w, h, qs)
    bad = dict((n, p) for n, p, _ in malformed.cases(good))["truncated"]
    want = D.cached(good, w, h, qs, denom, qd)
    cap_out = myyuv_hip.payload_bound(w // denom, h // denom)
    stream = torch.cuda.current_stream().cuda_stream
    fresh = myyuv_hip.Codec(0)
    try:
        cap, d_pay, d_sizes, d_out, d_osz = batch_buffers([bad, good], cap_out)
        fresh.downscale_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 2, w, h, qs, denom, qd, d_out.data_ptr(),
                               cap_out, d_osz.data_ptr(), stream)
        code, blk = fresh.sync_status(stream)
        assert (code, blk) == error_of(fresh.decompress, bad, w, h, qs)
        assert code == myyuv_hip.E_DCTYUV_SIZE
        out = bytes(d_out.cpu().numpy())
        sizes = d_osz.cpu().tolist()
        assert sizes[1] == len(want)
        assert out[cap_out:cap_out + sizes[1]] == want
        assert 0 <= sizes[0] <= cap_out  # frame 0: unspecified bytes, inside its slot
        assert out[2 * cap_out:] == b"\x5A" * 256
        assert fresh.downscale(good, w, h, qs, denom, qd) == want  # the context still works
    finally:
        fresh.close()


def test_device_batch_of_three(codec, oracle):
    import myyuv_hip
    import torch

    w, h, qs, qd, denom = 832, 384, (90, 50, 20), (20, 60, 100), 4
    pays = [R.tiled_stream(w, h, qs)[0], R.tiled_stream(w, h, qs, 0, 0)[0], R.tiled_stream(w, h, qs, 100, 40)[0]]
    assert len(set(pays)) == 3
    cap_out = myyuv_hip.payload_bound(w // denom, h // denom)
    stream = torch.cuda.current_stream().cuda_stream
    cap, d_pay, d_sizes, d_out, d_osz = batch_buffers(pays, cap_out, pad=64)
    assert cap != cap_out
    codec.downscale_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 3, w, h, qs, denom, qd, d_out.data_ptr(),
                           cap_out, d_osz.data_ptr(), stream)
    assert codec.sync_status(stream) == (0, -1)
    out = bytes(d_out.cpu().numpy())
    sizes = d_osz.cpu().tolist()
    for f in range(3):
        assert out[f * cap_out:f * cap_out + sizes[f]] == D.cached(pays[f], w, h, qs, denom, qd), f
    assert out[3 * cap_out:] == b"\x5A" * 256  # nothing past the last frame
    # a bad chunk in frame 2: the batch-global SOURCE block index
    nblk, szs = luma_sizes(pays[2])
    k = next(k for k in range(300, nblk) if szs[k] >= 12)
    off = 20 + nblk + sum(szs[:k])
    p2 = bytearray(pays[2])
    p2[off:off + szs[k]] = malformed._bits_run_out(bytes(p2[off:off + szs[k]]), szs[k])
    cap, d_pay, d_sizes, d_out, d_osz = batch_buffers([pays[0], pays[1], bytes(p2)], cap_out, pad=64)
    codec.downscale_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 3, w, h, qs, denom, qd, d_out.data_ptr(),
                           cap_out, d_osz.data_ptr(), stream)
    assert codec.sync_status(stream) == (10, 2 * sum(R.blocks(w, h)) + k)
    out = bytes(d_out.cpu().numpy())
    sizes = d_osz.cpu().tolist()
    for f in range(2):  # the frames before it are whole
        assert out[f * cap_out:f * cap_out + sizes[f]] == D.cached(pays[f], w, h, qs, denom, qd), f
    # a frame larger than cap_out: MYYUV_E_CAPACITY, nothing past cap_out
    small = (len(D.cached(pays[0], w, h, qs, denom, qd)) // 2) & ~3
    cap, d_pay, d_sizes, d_out, d_osz = batch_buffers(pays[:1], small)
    codec.downscale_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, 1, w, h, qs, denom, qd, d_out.data_ptr(),
                           small, d_osz.data_ptr(), stream)
    assert codec.sync_status(stream) == (myyuv_hip.E_CAPACITY, -1)
    assert bytes(d_out.cpu().numpy())[small:] == b"\x5A" * 256
    # alignment, stride and overlap rules
    cap, d_pay, d_sizes, d_out, d_osz = batch_buffers(pays, cap_out, pad=64)
    p, s, o, z = d_pay.data_ptr(), d_sizes.data_ptr(), d_out.data_ptr(), d_osz.data_ptr()
    for args in ((p + 1, s, cap, 3, w, h, qs, denom, qd, o, cap_out, z),
                 (p, s, cap, 3, w, h, qs, denom, qd, o + 2, cap_out, z),
                 (p, s, cap + 2, 3, w, h, qs, denom, qd, o, cap_out, z),
                 (p, s, cap, 3, w, h, qs, denom, qd, o, cap_out + 1, z),
                 (p, s, cap, 3, w, h, qs, denom, qd, p + cap, cap_out, z),
                 (p, s, cap, 0, w, h, qs, denom, qd, o, cap_out, z),
                 (p, s, cap, 3, w, h, qs, 3, qd, o, cap_out, z)):
        assert error_of(codec.downscale_device, *args, stream)[0] == myyuv_hip.E_ARG
    assert codec.sync_status(stream) == (0, -1)
    check(codec, pays[0], w, h, qs, denom, qd)


# ------------------------------------------------------------- table caches
def test_interleaved_with_ordinary_calls(codec, oracle):
    """An ordinary compress / decompress at other qualities right after a
    downscale on the same context gives its usual bytes, and the other way
    round: the downscaler's tables have a buffer and a cache of their own."""
    w, h, qs, qd = 416, 192, (90, 50, 20), (20, 60, 100)
    pay, raw = R.tiled_stream(w, h, qs)
    other = (70, 70, 70)
    pay2, raw2 = R.tiled_stream(w, h, other)
    assert codec.compress(raw, w, h, other) == oracle.compress(raw, w, h, other)
    check(codec, pay, w, h, qs, 2, qd)
    assert codec.decompress(pay2, w, h, other) == raw2
    assert codec.compress(raw, w, h, other) == oracle.compress(raw, w, h, other)
    check(codec, pay, w, h, qs, 2, qd)
    assert codec.compress(raw2, w, h, qs) == oracle.compress(raw2, w, h, qs)
    check(codec, pay2, w, h, other, 2, qs)  # new tables for the downscaler; the compress tables stay
    assert codec.decompress(pay, w, h, qs) == raw
    # the definition, through the codec's own two calls
    small = codec.decompress_scaled(pay, w, h, qs, 2)
    assert codec.compress(small, w // 2, h // 2, qd) == D.cached(pay, w, h, qs, 2, qd)


def test_default_destination_quality_is_the_sources(codec, oracle):
    w, h, qs = 416, 192, (90, 50, 20)
    pay, _ = R.tiled_stream(w, h, qs)
    assert codec.downscale(pay, w, h, qs, 2) == D.cached(pay, w, h, qs, 2, qs)


# -------------------------------------------------------------- kernel stats
def test_kernel_stats_name_the_downscale_kernel(codec):
    w, h = 416, 192
    pay, _ = R.tiled_stream(w, h, Q50)
    codec.profile(True, ["downscale", "decode_scaled", "fdct_quant", "fdct_fix", "huff_decode", "huff_encode"])
    try:
        for denom in (2, 2):
            codec.downscale(pay, w, h, Q50, denom, Q50)
        stats = codec.kernel_stats()
    finally:
        codec.profile(False)
    assert stats["downscale"][1] == 2 and stats["downscale"][0] > 0
    assert stats["huff_encode"][1] == 2
    for k in ("decode_scaled", "fdct_quant", "fdct_fix", "huff_decode"):  # one launch replaces them
        assert stats[k][1] == 0, k

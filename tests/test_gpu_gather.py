"""Crop and join on the GPU (include/myyuv_hip.h, "Crop and join"): every byte
is compared with the numpy restatement (gatherref), which never calls the code
under test; the meaning of the result with the oracle's compressor and
decoder.  Output buffers are filled with a canary first: the bytes past the
result, and the guard bands around the device outputs, must keep it."""
import os
import struct
import subprocess

import numpy as np
import pytest

import gatherref as G
import malformed
import regionref as R
import streamcases
import synth
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
C90 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-90.myyuv")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
CANARY = 0x5A
GUARD = 256


def error_of(fn, *args):
    import myyuv_hip

    try:
        fn(*args)
    except myyuv_hip.CodecError as e:
        return e.code, e.bad_block
    return 0, None


def check_crop(codec, pay, w, h, region, want=None):
    """The host-buffer crop into a canary-filled buffer: gatherref's bytes,
    and nothing after them."""
    want = G.crop_stream(pay, w, h, region) if want is None else want
    src = np.frombuffer(pay, np.uint8).copy()
    out = np.full(len(want) + 64, CANARY, np.uint8)
    n = codec.crop_into(src, w, h, region, out)
    assert n == len(want)
    assert out[:n].tobytes() == want, first_diff(out[:n].tobytes(), want)
    assert (out[n:] == CANARY).all()
    return want


def check_join(codec, pays, cols, rows, tw, th, want=None):
    want = G.join_stream(pays, cols, rows, tw, th) if want is None else want
    out = np.full(len(want) + 64, CANARY, np.uint8)
    n = codec.join_into(pays, cols, rows, tw, th, out)
    assert n == len(want)
    assert out[:n].tobytes() == want, first_diff(out[:n].tobytes(), want)
    assert (out[n:] == CANARY).all()
    return want


def first_diff(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return f"first difference at byte {k} of {len(a)} / {len(b)}"


def device_slots(pays):
    import torch

    cap = (max(len(p) for p in pays) + 3) & ~3
    buf = np.random.default_rng(len(pays)).integers(1, 256, len(pays) * cap, dtype=np.uint8)
    for f, p in enumerate(pays):
        buf[f * cap:f * cap + len(p)] = np.frombuffer(p, np.uint8)
    d_pay = torch.from_numpy(buf).cuda()
    d_sizes = torch.tensor([len(p) for p in pays], dtype=torch.int32, device="cuda")
    return cap, d_pay, d_sizes


def device_crop(codec, pays, w, h, region, cap_out):
    """crop_device of the batch between two guard bands; returns (code, block,
    [frame bytes], sizes)."""
    import torch

    n = len(pays)
    cap, d_pay, d_sizes = device_slots(pays)
    d_out = torch.full((GUARD + n * cap_out + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    d_osz = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    codec.crop_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, n, w, h, region, d_out.data_ptr() + GUARD, cap_out,
                      d_osz.data_ptr(), stream)
    code, blk = codec.sync_status(stream)
    out = bytes(d_out.cpu().numpy())
    assert out[:GUARD] == bytes([CANARY]) * GUARD and out[GUARD + n * cap_out:] == bytes([CANARY]) * GUARD
    body = out[GUARD:GUARD + n * cap_out]
    return code, blk, [body[f * cap_out:(f + 1) * cap_out] for f in range(n)], d_osz.cpu().tolist()


def check_device_crop(codec, pays, w, h, region, wants):
    cap_out = (max(len(x) for x in wants) + 3 & ~3) + 8
    code, blk, frames, sizes = device_crop(codec, pays, w, h, region, cap_out)
    assert (code, blk) == (0, -1)
    for f, want in enumerate(wants):
        assert sizes[f] == len(want), f
        assert frames[f][:sizes[f]] == want, (f, first_diff(frames[f][:sizes[f]], want))
        assert frames[f][sizes[f]:] == bytes([CANARY]) * (cap_out - sizes[f]), f


# ------------------------------------------------------------ 1. every position
def test_every_position_of_a_48x48_frame(codec, oracle):
    q = (50, 50, 50)
    pay, _ = R.tiled_stream(48, 48, q)
    f = R.chef()
    raw = synth.tiled_frame(f.data, f.width, f.height, 48, 48, 400, 300).tobytes()  # (the frame it compressed)
    assert oracle.compress(raw, 48, 48, q) == pay
    for ry in (0, 16, 32):
        for rx in (0, 16, 32):
            rg = (rx, ry, 16, 16)
            got = check_crop(codec, pay, 48, 48, rg)
            assert got == oracle.compress(R.crop(raw, 48, 48, rg), 16, 16, q), rg
            assert [n for (_, _, _, _, n) in G.crop_runs(48, 48, rg)] == [2, 2, 1, 1]


# ------------------------------------------------------------ 2. alignment sweep
TOTALS = (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17)


def split(total, n):
    """`total` bytes over n chunk sizes, each 0..255."""
    base = total // n
    out = [base] * n
    out[0] += total - base * n
    assert max(out) <= 255
    return out


def sweep_frame(w, h, region, sa, da, total, seed):
    """A synthetic w x h stream whose SECOND luma run of `region` (its second
    block row) holds `total` bytes, starts at source offset = sa mod 4 and at
    destination offset = da mod 4.  (The first run of a rectangle always
    starts at destination offset 0 mod 4: 20 header and 4k size bytes.)"""
    rx, ry, rw, rh = region
    bw, n = w // 8, rw // 8
    sizes = G.random_sizes(w, h, seed)
    s = sizes[0].astype(np.int64)
    j1, j2 = (ry // 8) * bw + rx // 8, (ry // 8 + 1) * bw + rx // 8
    spos = 12 + 8 + len(s)  # the luma content's position in the source
    dpos = 12 + 8 + (rw // 8) * (rh // 8)
    s[j2:j2 + n] = split(total, n)
    first = split(((da - dpos) % 4) + 4 * (seed % 3), n)  # the first run's bytes place the second in the output
    s[j1:j1 + n] = first
    s[0] = (sa - spos - int(s[1:j2].sum())) % 4 + 4 * (seed % 5)
    sizes[0] = s.astype(np.uint8)
    pay = G.synthetic(w, h, sizes, seed)
    assert (spos + int(s[:j2].sum())) % 4 == sa and (dpos + sum(first)) % 4 == da
    return pay


def sweep(codec, w, h, region, totals):
    pays, wants = [], []
    for total in totals:
        for sa in range(4):
            for da in range(4):
                pay = sweep_frame(w, h, region, sa, da, total, 16 * total + 4 * sa + da)
                pays.append(pay)
                wants.append(check_crop(codec, pay, w, h, region))
    check_device_crop(codec, pays, w, h, region, wants)  # one batch, guard bands around d_out


def test_alignment_sweep_short_runs(codec):
    sweep(codec, 64, 32, (16, 0, 32, 32), TOTALS)


def test_alignment_sweep_longest_run(codec):
    # 66 luma blocks per row, the rectangle's rows are single runs of 64 blocks of 255 bytes
    sweep(codec, 528, 16, (16, 0, 512, 16), (64 * 255,))


# ------------------------------------------------------------ 3. runs and boundaries
BIG_W, BIG_H = 1104, 528


@pytest.fixture(scope="module")
def big_streams():
    pay, _ = R.tiled_stream(BIG_W, BIG_H, (50, 50, 50))
    syn = G.synthetic(BIG_W, BIG_H, G.random_sizes(BIG_W, BIG_H, 77), 78)
    wants = {}
    for name, p in (("chef", pay), ("synthetic", syn)):
        for rg in ((16, 0, 1056, 512), (32, 16, 1056, 512)):
            wants[name, rg] = (p, G.crop_stream(p, BIG_W, BIG_H, rg))
    return wants


@pytest.mark.parametrize("name", ["chef", "synthetic"])
@pytest.mark.parametrize("rg", [(16, 0, 1056, 512), (32, 16, 1056, 512)])
def test_runs_straddle_groups_and_scan_tiles(codec, big_streams, name, rg):
    assert G.plane_counts(BIG_W, BIG_H)[0] == 9108 and G.plane_counts(rg[2], rg[3])[0] == 8448
    runs = G.crop_runs(BIG_W, BIG_H, rg)
    assert [n for (p, _, _, _, n) in runs if p == 0][:3] == [64, 64, 4]
    assert [n for (p, _, _, _, n) in runs if p == 1][:2] == [64, 2]
    pay, want = big_streams[name, rg]
    check_crop(codec, pay, BIG_W, BIG_H, rg, want)


# ------------------------------------------------------------ 4. long and short runs
def test_long_runs_of_q100_noise(codec, oracle):
    q = (100, 100, 100)
    pay, _ = R.noise_stream(1040, 32)
    raw = synth.noise_frame(1040, 32).tobytes()  # (the frame noise_stream compressed)
    sizes = G.parse(pay, 1040, 32)[0][0]
    assert sizes.min() >= 100  # about 9 KB per run of 64
    for rg in ((0, 0, 1040, 32), (16, 16, 1024, 16), (496, 0, 32, 32)):
        got = check_crop(codec, pay, 1040, 32, rg)
        assert got == oracle.compress(R.crop(raw, 1040, 32, rg), rg[2], rg[3], q)
    assert check_crop(codec, pay, 1040, 32, (0, 0, 1040, 32)) == pay


def test_short_runs_of_a_flat_frame(codec, oracle):
    q = (50, 50, 50)
    w, h = 1040, 32
    raw = bytes([128]) * (w * h * 3 // 2)
    pay = oracle.compress(raw, w, h, q)
    assert set(G.parse(pay, w, h)[0][0].tolist()) == {7}
    for rg in ((0, 0, w, h), (16, 0, 1024, 32), (1024, 16, 16, 16)):
        assert check_crop(codec, pay, w, h, rg) == oracle.compress(bytes([128]) * (rg[2] * rg[3] * 3 // 2), rg[2],
                                                                   rg[3], q)


def test_all_zero_sizes_inside_the_rectangle(codec):
    w, h, rg = 208, 96, (32, 16, 144, 48)
    sizes = G.random_sizes(w, h, 5)
    for p, (bw, bh) in enumerate(G.plane_dims(w, h)):
        d = 8 if p == 0 else 16
        grid = sizes[p].reshape(bh, bw)
        grid[rg[1] // d:(rg[1] + rg[3]) // d, rg[0] // d:(rg[0] + rg[2]) // d] = 0
    pay = G.synthetic(w, h, sizes, 6)
    want = check_crop(codec, pay, w, h, rg)
    assert struct.unpack_from("<I", want, 16)[0] == 0  # content_size 0, written verbatim
    assert len(want) == 36 + sum(G.plane_counts(rg[2], rg[3]))


# ------------------------------------------------------------ 5. meaning
@pytest.mark.parametrize("q", [(50, 50, 50), (90, 50, 20)])
def test_crop_is_the_compressed_crop(codec, oracle, q):
    w, h = 256, 192
    pay, full = R.tiled_stream(w, h, q)
    f = R.chef()
    raw = synth.tiled_frame(f.data, f.width, f.height, w, h, 400, 300).tobytes()
    for rg in ((16, 32, 96, 64), (0, 0, 256, 192), (240, 176, 16, 16), (64, 0, 128, 192)):
        got = check_crop(codec, pay, w, h, rg)
        assert got == oracle.compress(R.crop(raw, w, h, rg), rg[2], rg[3], q), rg
        assert codec.decompress(got, rg[2], rg[3], q) == R.crop(full, w, h, rg), rg


def test_whole_frame_crop_of_the_golden_file_is_its_payload(codec, golden):
    f = golden("chef-with-trumpet-DCT-50.myyuv")
    assert codec.crop(f.data, f.width, f.height, (0, 0, f.width, f.height)) == bytes(f.data)
    assert codec.join([f.data], 1, 1, f.width, f.height) == bytes(f.data)


# ------------------------------------------------------------ 6. join
def oracle_tiles(oracle, cols, rows, tw, th, q, noise_at=None):
    f = R.chef()
    pays, raws = [], []
    for t in range(cols * rows):
        if t == noise_at:
            raw = synth.noise_frame(tw, th).tobytes()
        else:
            raw = synth.tiled_frame(f.data, f.width, f.height, tw, th, 64 * t + 16, 48 * t).tobytes()
        raws.append(raw)
        pays.append(oracle.compress(raw, tw, th, q))
    return pays, raws


@pytest.mark.parametrize("cols,rows,tw,th,noise_at", [(1, 1, 48, 32, None), (3, 2, 48, 32, 4), (2, 2, 1040, 16, 1),
                                                      (1, 3, 16, 16, None), (3, 1, 16, 16, 2)])
def test_join_equals_the_compressed_assembly_and_crops_back(codec, oracle, cols, rows, tw, th, noise_at):
    q = (90, 50, 20)
    pays, raws = oracle_tiles(oracle, cols, rows, tw, th, q, noise_at)
    if cols * rows > 1:
        assert len(set(pays)) == cols * rows
    joined = check_join(codec, pays, cols, rows, tw, th)
    assert joined == oracle.compress(G.assemble(raws, cols, rows, tw, th), cols * tw, rows * th, q)
    if cols * rows == 1:
        assert joined == pays[0]
    for t in range(cols * rows):
        assert check_crop(codec, joined, cols * tw, rows * th, G.tile_rect(t, cols, tw, th), pays[t]) == pays[t]


def test_join_of_synthetic_tiles_and_its_device_form(codec):
    import torch

    cols, rows, tw, th = 2, 2, 1040, 16
    pays = [G.synthetic(tw, th, G.random_sizes(tw, th, 30 + t), 40 + t) for t in range(4)]
    assert [n for (p, _, _, _, n) in G.join_runs(cols, rows, tw, th) if p == 0][:6] == [64, 64, 2] * 2
    want = check_join(codec, pays, cols, rows, tw, th)
    cap, d_pay, d_sizes = device_slots(pays)
    cap_out = (len(want) + 3 & ~3) + 8
    d_out = torch.full((GUARD + cap_out + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    d_osz = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    codec.join_device(d_pay.data_ptr(), d_sizes.data_ptr(), cap, cols, rows, tw, th, d_out.data_ptr() + GUARD, cap_out,
                      d_osz.data_ptr(), stream)
    assert codec.sync_status(stream) == (0, -1)
    out = bytes(d_out.cpu().numpy())
    assert d_osz.cpu().tolist() == [len(want)]
    assert out[GUARD:GUARD + len(want)] == want
    assert out[:GUARD] == bytes([CANARY]) * GUARD
    assert out[GUARD + len(want):] == bytes([CANARY]) * (cap_out - len(want) + GUARD)
    # the rules: alignment, the tiles' stride, overlap, the grid
    p, s, o, z = d_pay.data_ptr(), d_sizes.data_ptr(), d_out.data_ptr() + GUARD, d_osz.data_ptr()
    import myyuv_hip

    for args in ((p + 1, s, cap, cols, rows, tw, th, o, cap_out, z), (p, s, cap, cols, rows, tw, th, o + 2, cap_out, z),
                 (p, s, cap + 2, cols, rows, tw, th, o, cap_out, z), (p, s, cap, cols, rows, tw, th, p + cap, cap_out, z),
                 (p, s, cap, 0, rows, tw, th, o, cap_out, z), (p, s, cap, cols, rows, tw + 8, th, o, cap_out, z),
                 (p, s, cap, cols, rows, tw, 0x10000000, o, cap_out, z), (p, s, cap, 0x10000, 0x10000, 16, 16, o, cap_out, z)):
        assert error_of(codec.join_device, *args, stream)[0] in (myyuv_hip.E_ARG, myyuv_hip.E_WIDTH,
                                                                 myyuv_hip.E_HEIGHT), args[2:7]
    assert codec.sync_status(stream) == (0, -1)


# ------------------------------------------------------------ 7. errors
@pytest.fixture(scope="module")
def cases(oracle):
    return streamcases.cases(oracle)


def test_header_cases_give_decompress_s_code_and_block(codec, cases):
    hdr = [c for c in cases if c.expect[0] and not c.faults]
    assert len(hdr) >= 10
    for c in hdr:
        assert error_of(codec.crop, c.payload, c.w, c.h, (0, 0, 16, 16)) == c.expect, c.name
        assert error_of(codec.crop, c.payload, c.w, c.h, (0, 0, 16, 16)) == \
            error_of(codec.decompress, c.payload, c.w, c.h, c.q), c.name
    # join: tile 1 of 2 reports its first block, tile 0 no block
    good = next(c for c in cases if c.kind == "accept" and (c.w, c.h) == (16, 16)).payload
    for c in (c for c in hdr if (c.w, c.h) == (16, 16)):
        assert error_of(codec.join, [good, c.payload], 2, 1, 16, 16) == (c.expect[0], 6), c.name
        assert error_of(codec.join, [good, c.payload], 1, 2, 16, 16) == (c.expect[0], 6), c.name
        assert error_of(codec.join, [c.payload, good], 2, 1, 16, 16) == (c.expect[0], -1), c.name
        assert error_of(codec.join, [c.payload, c.payload], 2, 1, 16, 16) == (c.expect[0], -1), c.name


def test_malformed_chunks_are_carried_over_verbatim(codec, cases):
    import myyuv_hip

    chunk_codes = (myyuv_hip.E_BAD_CODE, myyuv_hip.E_UNKNOWN_SYMBOL, myyuv_hip.E_BAD_CHUNK)
    bad = [c for c in cases if c.faults and all(f.code in chunk_codes for f in c.faults)]
    assert len(bad) >= 10
    for c in bad[:40]:
        assert error_of(codec.decompress, c.payload, c.w, c.h, c.q)[0] == c.expect[0]
        rg = (0, 0, c.w, c.h)
        got = check_crop(codec, c.payload, c.w, c.h, rg)
        assert error_of(codec.decompress, got, c.w, c.h, c.q)[0] == c.expect[0], c.name  # still there


def test_content_overrun_inside_the_rectangle_only(codec, cases):
    import myyuv_hip

    over = [c for c in cases if c.branch == "decode_group: rel+s > content_size"]
    assert len(over) >= 6
    hit = miss = 0
    for c in over:
        f = c.faults[0]
        ny, nc, _ = R.blocks(c.w, c.h)
        rects = [(0, 0, c.w, c.h), (0, 0, 16, 16), (c.w - 16, c.h - 16, 16, 16)]
        g = min(f.detect)
        p = 0 if g < ny else (1 if g < ny + nc else 2)
        rects.append(R.block_rect(c.w, c.h, p, g - (0, ny, ny + nc)[p]))
        for rg in rects:
            want = c.region_expect(c.w, c.h, rg, R.contains_block)
            got = error_of(codec.crop, c.payload, c.w, c.h, rg)
            assert got == want, (c.name, rg, got, want)
            if want[0]:
                assert want[0] == myyuv_hip.E_PLANE_CONTENT
                hit += 1
            else:
                check_crop(codec, c.payload, c.w, c.h, rg)
                miss += 1
    assert hit and miss


def test_large_content_overrun_is_a_content_error_not_a_capacity_error(codec):
    """Every size byte 255 over a little declared content: the selected sizes
    sum to far more than the source stream is long, more than any buffer
    sized from the source holds.  That is still MYYUV_E_PLANE_CONTENT with the
    plane's first block (check 4 comes before check 5), and a rectangle of
    blocks that end inside the content is cut as ever."""
    import myyuv_hip

    tiny = G.overrun_stream(16, 16, (1, 1, 1), 21)
    assert error_of(codec.crop, tiny, 16, 16, (0, 0, 16, 16)) == (myyuv_hip.E_PLANE_CONTENT, -1)
    assert error_of(codec.join, [tiny, tiny], 2, 1, 16, 16) == (myyuv_hip.E_PLANE_CONTENT, -1)
    good16 = G.synthetic(16, 16, G.random_sizes(16, 16, 23), 24)
    assert error_of(codec.join, [good16, tiny], 1, 2, 16, 16) == (myyuv_hip.E_PLANE_CONTENT, 6)
    huge = np.empty(1 << 20, np.uint8)  # a caller's buffer that would hold even the overrun's total
    assert error_of(codec.crop_into, np.frombuffer(tiny, np.uint8).copy(), 16, 16, (0, 0, 16, 16), huge) == \
        (myyuv_hip.E_PLANE_CONTENT, -1)
    for content, first in (((255 * 10, 255, 255), -1), ((255 * 32, 255, 255), 32)):
        big = G.overrun_stream(64, 32, content, 22)
        assert 255 * sum(G.plane_counts(64, 32)) > len(big)  # more content selected than the stream has bytes
        assert error_of(codec.crop, big, 64, 32, (0, 0, 64, 32)) == (myyuv_hip.E_PLANE_CONTENT, first)
        assert error_of(codec.crop, big, 64, 32, (16, 0, 48, 32)) == (myyuv_hip.E_PLANE_CONTENT, first)
        check_crop(codec, big, 64, 32, (0, 0, 16, 16))  # blocks 0, 1, 8, 9 and chroma block 0: inside the content
    check_join(codec, [good16, good16], 2, 1, 16, 16)  # the context still works


def test_rectangle_and_grid_errors_come_last(codec):
    import myyuv_hip

    q = (50, 50, 50)
    w, h = 208, 96
    pay, _ = R.tiled_stream(w, h, q)
    for rg in ((8, 0, 16, 16), (0, 0, 0, 16), (0, 0, 16, 0), (0, 0, 24, 16), (208, 0, 16, 16), (0, 96, 16, 16),
               (0xFFFFFFF0, 0, 32, 16), (16, 0, 208, 16), (0, 0, 16, 112)):
        assert error_of(codec.crop, pay, w, h, rg) == (myyuv_hip.E_ARG, -1), rg
    bad_rg = (8, 0, 16, 16)
    for args, code in (((pay[:8], w, h, bad_rg), myyuv_hip.E_DCTYUV_SIZE), ((pay, 204, h, bad_rg), myyuv_hip.E_WIDTH),
                       ((pay, w, 100, bad_rg), myyuv_hip.E_HEIGHT)):
        assert error_of(codec.crop, *args)[0] == code, args[1:]
    t, _ = R.tiled_stream(16, 16, q)
    # (a tile that is not a multiple of 16 fails the % 8 check of its chroma planes first)
    for cols, rows, tw, th, code in ((1, 1, 24, 16, myyuv_hip.E_WIDTH), (1, 1, 16, 40, myyuv_hip.E_HEIGHT),
                                     (1, 1, 20, 16, myyuv_hip.E_WIDTH), (1, 1, 16, 20, myyuv_hip.E_HEIGHT),
                                     (1, 1, 0x10000000, 16, myyuv_hip.E_ARG),     # a tile the compressor refuses
                                     (0x1000, 1, 0x100000, 16, myyuv_hip.E_ARG),  # cols * tile_w wraps 32 bits
                                     (1, 0x1000, 16, 0x100000, myyuv_hip.E_ARG),  # rows * tile_h wraps
                                     (2, 1, 0x8000000, 16, myyuv_hip.E_ARG)):     # an output the compressor refuses
        assert error_of(codec.join, [t] * (cols * rows), cols, rows, tw, th) == (code, -1), (cols, rows, tw, th)
    # the header first (tile 1's first block: 3 x 2 + 2 x (1 x 1) blocks per 24 x 16 tile)
    assert error_of(codec.join, [t, t[:8]], 2, 1, 24, 16) == (myyuv_hip.E_DCTYUV_SIZE, 8)
    assert error_of(codec.join, [t[:8]], 1, 1, 24, 16)[0] == myyuv_hip.E_DCTYUV_SIZE  # the header first
    src = np.frombuffer(pay, np.uint8).copy()  # overlap of payload and out
    assert error_of(codec.crop_into, src, w, h, (0, 0, 16, 16), src[: len(src)]) == (myyuv_hip.E_ARG, -1)
    check_crop(codec, pay, w, h, (16, 16, 32, 32))  # the context still works


# ------------------------------------------------------------ 8. capacity
def test_capacity(codec):
    import myyuv_hip

    q = (90, 90, 90)
    w, h, rg = 208, 96, (16, 16, 160, 64)
    pay, _ = R.tiled_stream(w, h, q)
    want = G.crop_stream(pay, w, h, rg)
    src = np.frombuffer(pay, np.uint8).copy()
    short = np.full(len(want) - 1, CANARY, np.uint8)
    with pytest.raises(myyuv_hip.CodecError) as e:
        codec.crop_into(src, w, h, rg, short)
    assert (e.value.code, e.value.need) == (myyuv_hip.E_CAPACITY, len(want))
    assert (short == CANARY).all()
    exact = np.full(len(want), CANARY, np.uint8)
    assert codec.crop_into(src, w, h, rg, exact) == len(want) and exact.tobytes() == want
    tiles = [G.crop_stream(pay, w, h, (16 * t, 0, 16, 16)) for t in range(4)]
    jw = G.join_stream(tiles, 2, 2, 16, 16)
    short = np.full(len(jw) - 1, CANARY, np.uint8)
    with pytest.raises(myyuv_hip.CodecError) as e:
        codec.join_into(tiles, 2, 2, 16, 16, short)
    assert (e.value.code, e.value.need) == (myyuv_hip.E_CAPACITY, len(jw)) and (short == CANARY).all()
    # the device form: inside cap_out, reported through sync_status, the size still written
    cap_out = (len(want) - 1) & ~3
    code, blk, frames, sizes = device_crop(codec, [pay], w, h, rg, cap_out)
    assert (code, blk) == (myyuv_hip.E_CAPACITY, -1) and sizes == [len(want)]
    assert frames[0] == bytes([CANARY]) * cap_out
    check_crop(codec, pay, w, h, rg, want)


# ------------------------------------------------------------ 9. device batch
def test_device_batch_of_two(codec):
    import myyuv_hip
    import torch

    q = (50, 50, 50)
    w, h, rg = 208, 96, (32, 16, 128, 64)
    pays = [R.tiled_stream(w, h, q)[0], R.tiled_stream(w, h, (90, 90, 90), 0, 0)[0]]
    assert len(pays[0]) != len(pays[1])
    wants = [G.crop_stream(p, w, h, rg) for p in pays]
    check_device_crop(codec, pays, w, h, rg, wants)
    # the rules
    cap, d_pay, d_sizes = device_slots(pays)
    cap_out = 4096
    d_out = torch.full((2 * cap_out,), CANARY, dtype=torch.uint8, device="cuda")
    d_osz = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    p, s, o, z = d_pay.data_ptr(), d_sizes.data_ptr(), d_out.data_ptr(), d_osz.data_ptr()
    for args in ((p + 1, s, cap, 2, w, h, rg, o, cap_out, z), (p, s, cap, 2, w, h, rg, o + 2, cap_out, z),
                 (p, s, cap + 2, 2, w, h, rg, o, cap_out, z), (p, s, cap, 2, w, h, rg, o, cap_out + 1, z),
                 (p, s, cap, 2, w, h, rg, p + cap, cap_out, z), (p, s, cap, 0, w, h, rg, o, cap_out, z),
                 (p, s, cap, 2, w, h, (8, 0, 16, 16), o, cap_out, z)):
        assert error_of(codec.crop_device, *args, stream)[0] == myyuv_hip.E_ARG
    assert codec.sync_status(stream) == (0, -1)
    assert (d_out.cpu().numpy() == CANARY).all()


def test_bad_header_in_frame_0_leaves_frame_1_whole():
    """On a fresh context (its workspace holds whatever the allocator returned)."""
    import myyuv_hip

    q = (50, 50, 50)
    w, h, rg = 208, 96, (32, 16, 128, 64)
    good, _ = R.tiled_stream(w, h, q)
    bad = dict((n, p) for n, p, _ in malformed.cases(good))["truncated"]
    want = G.crop_stream(good, w, h, rg)
    cap_out = (len(want) + 3 & ~3) + 8
    fresh = myyuv_hip.Codec(0)
    try:
        code, blk, frames, sizes = device_crop(fresh, [bad, good], w, h, rg, cap_out)
        assert (code, blk) == error_of(fresh.decompress, bad, w, h, q)
        assert code == myyuv_hip.E_DCTYUV_SIZE
        assert sizes[1] == len(want) and frames[1][:sizes[1]] == want
        assert frames[1][sizes[1]:] == bytes([CANARY]) * (cap_out - sizes[1])
        assert 0 <= sizes[0] <= cap_out
        code, blk, frames, sizes = device_crop(fresh, [good, bad], w, h, rg, cap_out)
        assert (code, blk) == (myyuv_hip.E_DCTYUV_SIZE, sum(R.blocks(w, h)))
        assert frames[0][:sizes[0]] == want
        assert fresh.crop(good, w, h, rg) == want  # the context still works
    finally:
        fresh.close()


# ------------------------------------------------------------ 10. kernel stats
def test_kernel_stats_name_the_gather_kernel(codec):
    q = (90, 90, 90)
    pay, _ = R.tiled_stream(208, 96, q)
    codec.profile(True, ["stream_gather", "scan_tiles", "huff_decode", "huff_encode", "stream_out", "decode_region"])
    try:
        codec.crop(pay, 208, 96, (16, 16, 64, 32))
        stats = codec.kernel_stats()
    finally:
        codec.profile(False)
    assert stats["stream_gather"][1] == 1 and stats["stream_gather"][0] > 0
    assert stats["scan_tiles"][1] == 4  # two scans, the size table, the headers
    for k in ("huff_decode", "huff_encode", "stream_out", "decode_region"):  # nothing is decoded or encoded
        assert stats[k][1] == 0, k


# ------------------------------------------------------------ 11. CLI
def cli(*args):
    return subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True)


def test_cli_crop_and_join(codec, tmp_path, golden):
    import myyuv_file

    f = golden("chef-with-trumpet-DCT-50.myyuv")
    rg = (32, 16, 128, 64)
    assert rg[0] + rg[2] <= f.width and rg[1] + rg[3] <= f.height
    crop, a, b = tmp_path / "crop.myyuv", tmp_path / "a.myyuv", tmp_path / "b.myyuv"
    r = cli(C50, "-crop", *rg, "-o", crop)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    assert r.stdout.splitlines()[0].startswith("YUV DCT crop (32 16 128 64) : ")
    got = myyuv_file.YUVFile.load(str(crop))
    assert (got.width, got.height, tuple(got.params)) == (128, 64, tuple(f.params))
    assert bytes(got.data) == G.crop_stream(f.data, f.width, f.height, rg)
    assert cli(crop, "-decompress", "-o", a).returncode == 0
    assert cli(C50, "-decompress", "-crop", *rg, "-o", b).returncode == 0
    assert a.read_bytes() == b.read_bytes()
    # four quarters of the rectangle, joined again
    parts = []
    for t in range(4):
        p = tmp_path / f"t{t}.myyuv"
        assert cli(C50, "-crop", rg[0] + 64 * (t % 2), rg[1] + 32 * (t // 2), 64, 32, "-o", p).returncode == 0
        parts.append(p)
    joined = tmp_path / "joined.myyuv"
    r = cli("-join", 2, 2, "-o", joined, *parts)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    assert r.stdout.splitlines()[0].startswith("YUV DCT join (2 2) : ")
    assert joined.read_bytes() == crop.read_bytes()
    # refusals
    out = tmp_path / "no.myyuv"
    r = cli(RAW, "-crop", *rg, "-o", out)
    assert r.returncode == 1 and r.stdout.startswith("Nothing to crop, image is not compressed")
    r = cli("-join", 2, 2, "-o", out, *parts[:3])
    assert r.returncode == 1 and r.stdout.startswith("Invalid arguments amount. 4 tiles are required, 3 given")
    other = tmp_path / "q90.myyuv"
    assert cli(C90, "-crop", rg[0], rg[1], 64, 32, "-o", other).returncode == 0
    r = cli("-join", 2, 1, "-o", out, parts[0], other)
    assert r.returncode != 0 and "tiles differ in compression params" in r.stderr
    r = cli("-join", 2, 1, "-o", out, parts[0], crop)
    assert r.returncode != 0 and "tiles differ in size" in r.stderr
    r = cli(C50, "-crop", 8, 0, 16, 16, "-o", out)
    assert r.returncode != 0 and "Invalid argument" in r.stderr
    assert not out.exists()

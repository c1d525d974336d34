"""Crop and join, the parts that need no GPU: the numpy restatement
(gatherref) against the oracle's compressor on cropped and assembled pixels;
the run map and the host gather of csrc/stream_gather.h (the map the kernels
walk) compiled for the host (tools/stream_gather_host.cpp) against gatherref,
also built with the address and undefined-behaviour sanitizers; the argument
errors of the C ABI and the CLI that come before any device is touched."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import gatherref as G
import regionref as R
import synth
from conftest import GOLDEN, PKG, ROOT

SRC = os.path.join(ROOT, "tools", "stream_gather_host.cpp")
CLI = os.path.join(PKG, "myyuv_cli")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
# luma blocks (wide, high) of the run-map shapes: one block, one run, a few
# runs per row, rows of 64 + 64 + 4 (chroma 64 + 2) and of four full runs + 4
MAP_SHAPES = ((1, 1), (2, 2), (26, 12), (132, 4), (260, 2))
JOIN_TILE_WIDTHS = (1, 2, 64, 65, 130)  # blocks of the chroma planes (luma: twice as many)


def build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-O2", "-std=c++17", *flags, "-I", os.path.join(PKG, "csrc"), SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("gather"), "stream_gather_host")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("gather_san"), "stream_gather_host_san", "-g",
                 "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(exe, stdin):
    r = subprocess.run([exe], input=stdin, capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-2000:])
    return r.stdout


def read_runs(buf, pos):
    (n,) = struct.unpack_from("<I", buf, pos)
    a = np.frombuffer(buf, np.uint32, 5 * n, pos + 4).reshape(n, 5)
    return [tuple(int(v) for v in row) for row in a], pos + 4 + 20 * n


def read_result(buf, pos):
    code, bad, size = struct.unpack_from("<iqI", buf, pos)
    pos += 16
    out = None
    if code == 0:
        out = buf[pos:pos + size]
        pos += size
    return (code, bad, size, out), pos


def crop_record(pay, w, h, region, cap=None):
    cap = len(pay) + 36 if cap is None else cap
    return struct.pack("<8I", 3, w, h, *region, cap) + struct.pack("<I", len(pay)) + pay


def join_record(pays, cols, rows, tw, th, cap=None):
    cap = sum(len(p) for p in pays) + 36 if cap is None else cap
    return struct.pack("<6I", 4, cols, rows, tw, th, cap) + b"".join(struct.pack("<I", len(p)) + p for p in pays)


# ---- the definition means what the issue says --------------------------------
@pytest.fixture(scope="module")
def noise_tile(oracle):
    q = (90, 50, 20)
    raw = synth.noise_frame(48, 32).tobytes()
    return oracle.compress(raw, 48, 32, q), raw


def join_case(oracle, noise_tile):
    """3 x 2 tiles of 48 x 32 at q(90, 50, 20): tile 4 noise, the others
    different windows of the chef frame.  (payloads, raw frames)."""
    q = (90, 50, 20)
    f = R.chef()
    pays, raws = [], []
    for t in range(6):
        if t == 4:
            pays.append(noise_tile[0]), raws.append(noise_tile[1])
            continue
        raw = synth.tiled_frame(f.data, f.width, f.height, 48, 32, 64 * t + 16, 48 * t).tobytes()
        pays.append(oracle.compress(raw, 48, 32, q)), raws.append(raw)
    return pays, raws, q


@pytest.mark.parametrize("w,h,q,region", [(256, 192, (50, 50, 50), (16, 32, 96, 64)),
                                          (1056, 528, (90, 75, 30), (1024, 16, 32, 496))])
def test_crop_equals_compress_of_the_cropped_pixels(oracle, w, h, q, region):
    f = R.chef()
    raw = synth.tiled_frame(f.data, f.width, f.height, w, h, 400, 300).tobytes()
    pay = oracle.compress(raw, w, h, q)
    assert G.crop_stream(pay, w, h, region) == oracle.compress(R.crop(raw, w, h, region), region[2], region[3], q)


def test_whole_frame_crop_and_1x1_join_are_the_identity(oracle):
    q = (100, 100, 100)
    raw = synth.noise_frame(128, 128).tobytes()
    pay = oracle.compress(raw, 128, 128, q)
    assert G.crop_stream(pay, 128, 128, (0, 0, 128, 128)) == pay
    assert G.join_stream([pay], 1, 1, 128, 128) == pay
    assert G.build(G.parse(pay, 128, 128)) == pay


def test_join_equals_compress_of_the_assembled_pixels_and_crops_back(oracle, noise_tile):
    pays, raws, q = join_case(oracle, noise_tile)
    assert len({len(p) for p in pays}) > 1
    joined = G.join_stream(pays, 3, 2, 48, 32)
    assert joined == oracle.compress(G.assemble(raws, 3, 2, 48, 32), 144, 64, q)
    for t in range(6):
        assert G.crop_stream(joined, 144, 64, G.tile_rect(t, 3, 48, 32)) == pays[t], t


# ---- csrc/stream_gather.h on the host -----------------------------------------
@pytest.fixture(scope="module")
def map_inputs():
    recs, want = [], []
    for bw, bh in MAP_SHAPES:
        w, h = 8 * bw if bw % 2 == 0 else 16 * bw, 8 * bh if bh % 2 == 0 else 16 * bh
        W, H = w + 48, h + 32
        for region in ((0, 0, w, h), (16, 32, w, h), (48, 0, w, h)):
            recs.append(struct.pack("<7I", 1, W, H, *region))
            want.append(G.crop_runs(W, H, region))
        recs.append(struct.pack("<7I", 1, w, h, 0, 0, w, h))
        want.append(G.crop_runs(w, h, (0, 0, w, h)))
    for cb in JOIN_TILE_WIDTHS:
        for cols, rows, th in ((1, 1, 16), (3, 2, 32), (2, 3, 16)):
            recs.append(struct.pack("<5I", 2, cols, rows, 16 * cb, th))
            want.append(G.join_runs(cols, rows, 16 * cb, th))
    return b"".join(recs), want


def test_run_map_equals_the_restatement(harness, map_inputs):
    recs, want = map_inputs
    buf, pos = run(harness, recs), 0
    for k, w in enumerate(want):
        got, pos = read_runs(buf, pos)
        assert got == w, (k, got[:3], w[:3])
    assert pos == len(buf)
    # the shapes split as intended
    counts = [n for (p, _, _, _, n) in G.crop_runs(1104, 528, (16, 0, 1056, 32)) if p == 0]
    assert counts[:3] == [64, 64, 4]
    assert [n for (p, _, _, _, n) in G.join_runs(2, 1, 1040, 16) if p == 0][:6] == [64, 64, 2] * 2
    for runs in want:  # every output block once, in order, per plane
        for p in range(3):
            nxt = 0
            for (pp, dst, _, _, n) in runs:
                if pp == p:
                    assert dst == nxt and 1 <= n <= 64
                    nxt += n


@pytest.fixture(scope="module")
def gather_inputs(oracle):
    """(records, wanted (code, bad, size, bytes)) on synthetic streams whose
    size bytes include 0 and 255, and on one oracle stream."""
    recs, want = [], []

    def crop(pay, w, h, region, cap=None, expect=None):
        recs.append(crop_record(pay, w, h, region, cap))
        ref = G.crop_stream(pay, w, h, region)
        want.append(expect(ref) if expect else (0, -1, len(ref), ref))

    for seed, (w, h) in enumerate(((16, 16), (64, 32), (1104, 32), (208, 96))):
        sizes = G.random_sizes(w, h, seed)
        for s in sizes:
            s[0], s[-1] = 255, 0
            s[len(s) // 2] = 255
        pay = G.synthetic(w, h, sizes, 100 + seed)
        crop(pay, w, h, (0, 0, w, h))
        crop(pay, w, h, (0, 0, 16, 16))
        crop(pay, w, h, (w - 16, h - 16, 16, 16))
        if w > 32:
            crop(pay, w, h, (16, 0, w - 32, h))
        need = len(G.crop_stream(pay, w, h, (0, 0, w, h)))
        crop(pay, w, h, (0, 0, w, h), cap=need - 1, expect=lambda ref: (5, -1, len(ref), None))
    pay, _ = R.tiled_stream(256, 192, (50, 50, 50))
    crop(pay, 256, 192, (16, 32, 96, 64))
    # a header fault, and content overruns: the last chunk of plane 0 / plane 1
    # ends one byte beyond the declared content (reported with the plane's
    # first block, -1 for block 0; outside the rectangle: not at all)
    good = G.synthetic(64, 32, G.random_sizes(64, 32, 9, 1, 9), 9)
    ps0, hc0 = struct.unpack_from("<I", good, 0)[0], struct.unpack_from("<I", good, 16)[0]
    for hpos, hc, first in ((16, hc0, -1), (12 + ps0 + 4, struct.unpack_from("<I", good, 12 + ps0 + 4)[0], 32)):
        over = bytearray(good)
        struct.pack_into("<I", over, hpos, hc - 1)
        crop(bytes(over), 64, 32, (0, 0, 16, 16), expect=lambda ref: (0, -1, len(ref), ref))
        recs.append(crop_record(bytes(over), 64, 32, (48, 16, 16, 16)))
        want.append((9, first, None, None))
    recs.append(crop_record(good[:-1], 64, 32, (0, 0, 16, 16)))
    want.append((6, -1, None, None))
    # large overruns: every size byte 255, a little content (the selected sizes
    # sum to far more than the stream is long)
    tiny = G.overrun_stream(16, 16, (1, 1, 1), 21)
    recs.append(crop_record(tiny, 16, 16, (0, 0, 16, 16)))
    want.append((9, -1, None, None))
    for content, first in (((255 * 10, 255, 255), -1), ((255 * 32, 255, 255), 32)):
        big = G.overrun_stream(64, 32, content, 22)
        assert 255 * sum(G.plane_counts(64, 32)) > len(big)  # more content selected than the stream has bytes
        recs.append(crop_record(big, 64, 32, (0, 0, 64, 32)))
        want.append((9, first, None, None))
        crop(big, 64, 32, (0, 0, 16, 16))  # outside the overrun: blocks 0, 1, 8, 9 and chroma block 0
    recs.append(join_record([tiny, tiny], 2, 1, 16, 16))
    want.append((9, -1, None, None))
    good16 = G.synthetic(16, 16, G.random_sizes(16, 16, 23), 24)
    recs.append(join_record([good16, tiny], 1, 2, 16, 16))
    want.append((9, 6, None, None))
    # joins
    for k, (cols, rows, tw, th) in enumerate(((1, 1, 16, 16), (3, 2, 48, 32), (2, 2, 1040, 16), (1, 3, 16, 16),
                                              (3, 1, 16, 16))):
        pays = [G.synthetic(tw, th, G.random_sizes(tw, th, 50 * k + t), 7 * k + t) for t in range(cols * rows)]
        recs.append(join_record(pays, cols, rows, tw, th))
        ref = G.join_stream(pays, cols, rows, tw, th)
        want.append((0, -1, len(ref), ref))
        if cols * rows > 1:  # a header fault in tile 1: its first block
            bad = list(pays)
            bad[1] = bad[1][:-1]
            recs.append(join_record(bad, cols, rows, tw, th))
            want.append((6, sum(G.plane_counts(tw, th)), None, None))
    return b"".join(recs), want


def check_results(buf, want):
    pos = 0
    for k, (code, bad, size, out) in enumerate(want):
        got, pos = read_result(buf, pos)
        assert got[0] == code and got[1] == bad, (k, got[:3], (code, bad))
        if size is not None:
            assert got[2] == size, (k, got[2], size)
        if code == 0:
            assert got[3] == out, k
    assert pos == len(buf)


def test_host_gather_equals_the_restatement(harness, gather_inputs):
    recs, want = gather_inputs
    check_results(run(harness, recs), want)


def test_sanitized_build_is_clean_and_identical(harness, sanitized, map_inputs, gather_inputs):
    for recs in (map_inputs[0], gather_inputs[0]):
        r = subprocess.run([sanitized], input=recs, capture_output=True)
        assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr.decode(errors="replace")[-2000:])
        assert r.stdout == run(harness, recs)


def test_bad_records_are_refused(harness):
    for rec in (struct.pack("<I", 9), struct.pack("<7I", 1, 64, 32, 8, 0, 16, 16), struct.pack("<7I", 1, 64, 32, 0, 0, 80, 16),
                struct.pack("<7I", 1, 64, 32, 0, 0, 0, 16), struct.pack("<5I", 2, 0, 1, 16, 16),
                struct.pack("<5I", 2, 1, 1, 24, 16)):
        assert subprocess.run([harness], input=rec, capture_output=True).returncode == 2


# ---- argument errors that need no device -------------------------------------
def test_handle_and_pointer_errors_need_no_device():
    import myyuv_hip

    L = myyuv_hip.load()
    pay = np.zeros(64, np.uint8)
    out = np.zeros(64, np.uint8)
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    size = ctypes.c_uint32(9)
    bad = ctypes.c_int64(7)
    assert L.myyuv_gpu_dct_crop(None, u8(pay), 64, 16, 16, 0, 0, 16, 16, u8(out), 64, ctypes.byref(size),
                                ctypes.byref(bad)) == myyuv_hip.E_ARG
    assert bad.value == -1 and size.value == 9
    bad.value = 7
    ptrs = (ctypes.c_void_p * 1)(pay.ctypes.data)
    sizes = (ctypes.c_uint32 * 1)(64)
    assert L.myyuv_gpu_dct_join(None, ptrs, sizes, 1, 1, 16, 16, u8(out), 64, ctypes.byref(size),
                                ctypes.byref(bad)) == myyuv_hip.E_ARG
    assert bad.value == -1 and size.value == 9
    assert L.myyuv_gpu_dct_crop_device(None, 256, 512, 64, 1, 16, 16, 0, 0, 16, 16, 1024, 64, 2048,
                                       None) == myyuv_hip.E_ARG
    assert L.myyuv_gpu_dct_join_device(None, 256, 512, 64, 1, 1, 16, 16, 1024, 64, 2048, None) == myyuv_hip.E_ARG
    assert not (out != 0).any()
    # the new id lies past the fixed-length list of myyuv_hip_kernel_stats, which keeps its length
    assert myyuv_hip.KERNELS_ALL.index("stream_gather") == myyuv_hip.K_GATHER == 17
    assert myyuv_hip.KERNELS_ALL[:len(myyuv_hip.KERNELS)] == myyuv_hip.KERNELS and myyuv_hip.K_TOTAL == 18
    # and the sized call checks its arguments before any device is touched
    ms, n = (ctypes.c_double * 18)(), (ctypes.c_int64 * 18)()
    assert L.myyuv_hip_kernel_stats_n(None, 18, ms, n) == myyuv_hip.E_ARG
    for name in ("myyuv_gpu_dct_crop", "myyuv_gpu_dct_crop_device", "myyuv_gpu_dct_join", "myyuv_gpu_dct_join_device"):
        assert name in myyuv_hip.EXPORTS and getattr(L, name)


def test_header_defines_the_calls():
    import re

    src = open(os.path.join(ROOT, "include", "myyuv_hip.h")).read()
    assert re.search(r"^#define MYYUV_K_GATHER 17\b", src, re.M)
    assert re.search(r"^#define MYYUV_K_COUNT 17\b", src, re.M) and re.search(r"^#define MYYUV_K_TOTAL 18\b", src, re.M)
    assert re.search(r"^int myyuv_hip_kernel_stats_n\(", src, re.M)
    for name in ("myyuv_gpu_dct_crop", "myyuv_gpu_dct_crop_device", "myyuv_gpu_dct_join", "myyuv_gpu_dct_join_device"):
        assert re.search(r"^int %s\(" % name, src, re.M), name


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def test_cli_crop_and_join_argument_errors(tmp_path):
    out = str(tmp_path / "x.myyuv")
    r = cli(RAW, "-crop", "0", "0", "16", "16", "-o", out)
    assert r.returncode == 1, r.stdout
    assert r.stdout.splitlines()[0] == \
        "Nothing to crop, image is not compressed (-crop keeps DCT chunks; use -decompress -crop)"
    for tail in (["0", "0", "16"], ["0", "0", "16", "x", "-o", out], ["0", "0", "16", "-16", "-o", out], []):
        r = cli(C50, "-crop", *tail)
        assert r.returncode == 1 and "Usage" in r.stdout, (tail, r.stdout)
        assert r.stdout.splitlines()[0] == "Invalid argument, -crop must be followed by four numbers `X Y W H`"
    for tail in ([], ["-o"], ["-o", out, "extra"], ["out.myyuv"]):
        r = cli(C50, "-crop", "0", "0", "16", "16", *tail)
        assert r.returncode == 1 and "Usage" in r.stdout, (tail, r.stdout)
        assert r.stdout.splitlines()[0] == "Invalid argument, last arguments must be `-o /path/to/new_image.myyuv`"
    # the grid, the tile count, uncompressed tiles
    for tail in (["0", "1", "-o", out, C50], ["x", "1", "-o", out, C50], ["1"]):
        r = cli("-join", *tail)
        assert r.returncode == 1 and "Usage" in r.stdout, (tail, r.stdout)
        assert r.stdout.splitlines()[0] == "Invalid argument, -join must be followed by two numbers `COLS ROWS`"
    r = cli("-join", "2", "1", "-o", out, C50)
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "Invalid arguments amount. 2 tiles are required, 1 given"
    r = cli("-join", "1", "1", out, C50, C50)
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "Invalid arguments. Expected -o OUT.myyuv followed by the tiles"
    r = cli("-join", "1", "1", "-o", out, RAW)
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "Nothing to join, a tile is not compressed (-join keeps DCT chunks)"
    assert not os.path.exists(out)
    usage = cli(C50, "-crop").stdout
    assert "myyuv_cli IMAGE.myyuv -crop X Y W H -o OUT.myyuv" in usage
    assert "myyuv_cli -join COLS ROWS -o OUT.myyuv TILE.myyuv..." in usage

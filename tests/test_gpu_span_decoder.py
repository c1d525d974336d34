"""The span decoder (k_decode_span, csrc/k_huff_decode.hip): a wave owns 256
consecutive blocks of a plane, finishes the blocks whose 7-byte chunk is the
one-symbol closed form (codec_common.hpp single_chunk_words) without decoding
them, and decodes the others, the "real" ones, in passes of 64 from a list.

Every stream here is built in the coefficient domain (coefgen, streamcases'
Layout) and decoded by a context with MYYUV_DECODER=span and by one with
MYYUV_DECODER=group (k_decode_idct); the expected frame or (code, bad block)
is the oracle's (oracle.decompress_ex), and for the hand-made chunks also
written down by construction (coefgen.compose of the blocks they must decode
to).  Nothing is taken from the code under test.
"""
import os

import numpy as np
import pytest

import coefgen
from streamcases import Layout, Plane, _junk, _pad, bad_chunks

pytestmark = pytest.mark.gpu

SPAN = 256  # codec_common.hpp kDecSpan
Q50 = (50, 50, 50)
# (frame, luma blocks, chroma blocks): around the group and span edges
GEOMETRIES = ((16, 16, 4, 1), (64, 64, 64, 16), (128, 128, 256, 64), (80, 208, 260, 65), (48, 688, 516, 129))


def _codec_with_decoder(name):
    import myyuv_hip

    old = os.environ.get("MYYUV_DECODER")
    os.environ["MYYUV_DECODER"] = name
    try:
        return myyuv_hip.Codec(0)
    finally:
        if old is None:
            del os.environ["MYYUV_DECODER"]
        else:
            os.environ["MYYUV_DECODER"] = old


@pytest.fixture(scope="module")
def decoders():
    d = {name: _codec_with_decoder(name) for name in ("span", "group")}
    yield d
    for c in d.values():
        c.close()


@pytest.fixture(scope="module")
def chunks(oracle):
    return coefgen.Chunks(oracle.huff_encode_block)


@pytest.fixture(scope="module")
def pools(oracle):
    """(single, busy): 96 one-symbol blocks (the DC alone, DC 0 and both
    extremes among them) and 160 others: short messages, in-range noise, and
    a block of every K2 sort key (long messages and large tables included)."""
    rng = np.random.default_rng(4242)
    single = np.zeros((96, 64), np.int16)
    single[:, 0] = rng.integers(-1024, 1024, 96)
    single[:3, 0] = (0, -1024, 1023)
    short = np.zeros((48, 64), np.int16)
    for b in short:
        msz = int(rng.integers(2, 9))
        b[:msz] = rng.integers(-40, 41, msz)
        b[msz - 1] = b[msz - 1] or 5
    noise = coefgen.in_range_blocks(64, oracle.qtable(50, 0), rng)
    for b in noise:
        if not b[1:].any():
            b[7] = 1
    busy = np.concatenate([short, noise, coefgen.mixed_pool(seed=4343, per_key=4)])
    busy = busy[[i for i, b in enumerate(busy) if b[1:].any()]]
    return single, busy


def layout_of(w, h, plane_blocks, chunks):
    return Layout(w, h, [Plane(b, [chunks.one(z) for z in b]) for b in plane_blocks])


def mixed_planes(w, h, pools, rng, p_single=0.5):
    single, busy = pools
    out = []
    for n in coefgen.plane_counts(w, h):
        pick_single = rng.random(n) < p_single
        out.append(np.where(pick_single[:, None], single[rng.integers(0, len(single), n)],
                            busy[rng.integers(0, len(busy), n)]))
    return out


def outcome(codec, payload, w, h, q):
    import myyuv_hip

    try:
        return 0, -1, codec.decompress(payload, w, h, q)
    except myyuv_hip.CodecError as e:
        return e.code, e.bad_block, None


def check(decoders, oracle, payload, w, h, q, expect=None, frame=None):
    """Both decoders against the oracle; `expect` / `frame`: what the stream
    must give by construction (the oracle is held to it too)."""
    code, bad, want = oracle.decompress_ex(payload, w, h, q)
    if expect is not None:
        assert (code, bad) == expect, ("oracle", code, bad)
    if frame is not None:
        assert want == frame, "the oracle against the construction"
    for name, c in decoders.items():
        gcode, gbad, got = outcome(c, payload, w, h, q)
        assert (gcode, gbad) == (code, bad), (name, gcode, gbad, code, bad)
        if code == 0:
            assert got == want, name
    return code, bad, want


# ---- plane sizes around the span and group edges ----------------------------
@pytest.mark.parametrize("w,h,ny,nc", GEOMETRIES, ids=[f"{g[0]}x{g[1]}" for g in GEOMETRIES])
def test_plane_sizes(decoders, oracle, chunks, pools, w, h, ny, nc):
    assert coefgen.plane_counts(w, h) == (ny, nc, nc)
    rng = np.random.default_rng(w * 1000 + h)
    for p_single in (0.5, 0.0, 1.0):
        lay = layout_of(w, h, mixed_planes(w, h, pools, rng, p_single), chunks)
        code, _, _ = check(decoders, oracle, lay.payload(), w, h, (50, 60, 70))
        assert code == 0


def closed_form(v):
    key = v & 0x7FF
    return bytes([1, 0, 3, 0, key & 0xFF, key >> 8, 0])


def is_closed_form(chunk):
    return len(chunk) == 7 and chunk == closed_form(chunk[4] | chunk[5] << 8)


# ---- exactly N real chunks in a span ------------------------------------------
EDGE_SPOTS = (0, SPAN - 1, 63, 64, 127, 128, 191, 192)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129, 256])
def test_real_chunk_counts(decoders, oracle, chunks, pools, n):
    """80x208: the luma plane is a full span and one of 4 blocks.  A flat
    frame with exactly n busy blocks in the full span, at its first and last
    block and on both sides of every group boundary first."""
    w, h = 80, 208
    single, busy = pools
    rng = np.random.default_rng(100 + n)
    planes = [single[rng.integers(0, len(single), k)] for k in coefgen.plane_counts(w, h)]
    order = list(EDGE_SPOTS) + [int(i) for i in rng.permutation(SPAN) if i not in EDGE_SPOTS]
    for i in order[:n]:
        planes[0][i] = busy[rng.integers(0, len(busy))]
    lay = layout_of(w, h, planes, chunks)
    real = [not is_closed_form(c) for c in lay.planes[0].chunks]
    assert sum(real[:SPAN]) == n and not any(real[SPAN:])
    code, _, _ = check(decoders, oracle, lay.payload(), w, h, Q50)
    assert code == 0


def test_all_busy_noise(decoders, oracle, chunks):
    w, h = 80, 208
    rng = np.random.default_rng(77)
    planes = [coefgen.in_range_blocks(k, oracle.qtable(50, p != 0), rng)
              for p, k in enumerate(coefgen.plane_counts(w, h))]
    for pl in planes:
        pl[:, 5] |= 1  # (none DC-only)
    code, _, _ = check(decoders, oracle, layout_of(w, h, planes, chunks).payload(), w, h, Q50)
    assert code == 0


# ---- 7-byte chunks that are not the closed form --------------------------------
def seven_byte_variants():
    """name -> (chunk, zig-zag block or None, code): chunks of 7 bytes that
    differ from the closed form of v = -37 in one respect each."""
    v = -37
    key = v & 0x7FF
    lo, hi = key & 0xFF, key >> 8
    out = {}
    for k in range(2, 9):  # one code "0" of length 1, sent k times
        blk = np.zeros(64, np.int16)
        blk[:k] = v
        out[f"message_of_{k}"] = (bytes([k, 0, 3, 0, lo, hi, 0]), blk, 0)
    dc = np.zeros(64, np.int16)
    dc[0] = v
    out["junk_in_value_padding"] = (bytes([1, 0, 3, 0, lo, hi | 0xA8, 0]), dc, 0)
    out["junk_in_value_padding_all"] = (bytes([1, 0, 3, 0, lo, hi | 0xF8, 0]), dc, 0)
    out["junk_in_code_byte"] = (bytes([1, 0, 3, 0, lo, hi, 0xFE]), dc, 0)
    out["junk_in_code_byte_one_bit"] = (bytes([1, 0, 3, 0, lo, hi, 0x80]), dc, 0)
    out["tb0_nbits0"] = (bytes([0, 0, 0, 0xAB, 0xCD, 0xEF, 0x01]), np.zeros(64, np.int16), 0)
    out["nbits9"] = (bytes([9, 0, 3, 0, lo, hi, 0]), None, 12)   # 3 + 3 + 2 bytes > 7
    out["tb4"] = (bytes([1, 0, 4, 0, lo, hi, 0]), None, 12)      # 3 + 4 + 1 bytes > 7
    for name, (ch, _, _) in out.items():
        assert len(ch) == 7 and ch != closed_form(v), name
    return out


VARIANTS = seven_byte_variants()
# (plane, block): a span's first and last block, both sides of a group and of
# a span boundary, the 4-block last span, the chroma planes
SPOTS_80x208 = ((0, 0), (0, 63), (0, 64), (0, 255), (0, 256), (0, 259), (1, 0), (1, 64), (2, 33))


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_seven_byte_chunks_that_are_not_the_closed_form(decoders, oracle, chunks, pools, name):
    w, h = 80, 208
    single, _ = pools
    chunk, blk, code = VARIANTS[name]
    rng = np.random.default_rng(5)
    planes = [single[rng.integers(0, len(single), k)] for k in coefgen.plane_counts(w, h)]
    lay = layout_of(w, h, planes, chunks)
    assert all(len(c) == 7 for p in lay.planes for c in p.chunks)
    assert lay.planes[0].chunks[1] == closed_form(int(planes[0][1][0]))
    spots = SPOTS_80x208 if code == 0 else ((0, 100), (1, 5))
    for p, k in spots:
        lay.set(p, k, chunk, blk)
    if code == 0:
        frame = coefgen.compose(lay.blocks(), w, h, Q50, oracle)
        check(decoders, oracle, lay.payload(), w, h, Q50, expect=(0, -1), frame=frame)
    else:
        check(decoders, oracle, lay.payload(), w, h, Q50, expect=(code, 100))


def test_all_seven_byte_variants_in_one_span(decoders, oracle, chunks, pools):
    """Every accepted variant next to true closed forms and busy blocks."""
    w, h = 128, 128
    single, busy = pools
    rng = np.random.default_rng(6)
    planes = [single[rng.integers(0, len(single), k)] for k in coefgen.plane_counts(w, h)]
    planes[0][::5] = busy[rng.integers(0, len(busy), len(planes[0][::5]))]
    lay = layout_of(w, h, planes, chunks)
    ok = [v for _, v in sorted(VARIANTS.items()) if v[2] == 0]
    for i, (chunk, blk, _) in enumerate(ok * 3):
        lay.set(0, 1 + 6 * i + i % 4, chunk, blk)
    frame = coefgen.compose(lay.blocks(), w, h, Q50, oracle)
    check(decoders, oracle, lay.payload(), w, h, Q50, expect=(0, -1), frame=frame)


# ---- truncation -----------------------------------------------------------------
def test_truncation(decoders, oracle, chunks, pools):
    """A flat frame (closed forms only) with bytes after plane 2: the stream
    cut just after its last chunk decodes, cut inside that chunk it fails its
    header's total (6); a declared content that ends inside a closed-form
    chunk is the plane-content error (9) at the plane's first block."""
    w, h = 64, 64
    single, _ = pools
    rng = np.random.default_rng(8)
    planes = [single[rng.integers(0, len(single), k)] for k in coefgen.plane_counts(w, h)]
    lay = layout_of(w, h, planes, chunks)
    whole = lay.payload()
    lay.trailing = _junk(29, 9)
    long = lay.payload()
    code, _, frame = check(decoders, oracle, long, w, h, Q50, expect=(0, -1))
    check(decoders, oracle, long[:len(whole)], w, h, Q50, expect=(0, -1), frame=frame)
    check(decoders, oracle, long[:len(whole) + 1], w, h, Q50, expect=(0, -1), frame=frame)
    for cut in (1, 3, 6, 7, 8):
        check(decoders, oracle, long[:len(whole) - cut], w, h, Q50, expect=(6, -1))
    for p, first in ((0, -1), (1, 64), (2, 80)):
        for short in (1, 4, 7, 8):
            lie = layout_of(w, h, planes, chunks)
            lie.planes[p].hc = 7 * len(planes[p]) - short
            check(decoders, oracle, lie.payload(), w, h, Q50, expect=(9, first))
    check(decoders, oracle, whole, w, h, Q50, expect=(0, -1), frame=frame)  # the contexts afterwards


# ---- long chunks: a pass needs several staging rounds ----------------------------
def test_span_of_255_byte_chunks(decoders, oracle, chunks, pools):
    """128x128: the luma plane is one span of 256 chunks of 255 B (the list's
    largest offset, 255 * 255), the chroma planes a group each with closed
    forms between long chunks."""
    w, h = 128, 128
    single, busy = pools
    rng = np.random.default_rng(10)
    planes = [busy[rng.integers(0, len(busy), 256)], single[rng.integers(0, len(single), 64)],
              busy[rng.integers(0, len(busy), 64)]]
    planes[2][::3] = single[:22]
    lay = layout_of(w, h, planes, chunks)
    for p in (0, 1, 2):
        for k, c in enumerate(lay.planes[p].chunks):
            if p == 0 or (p == 1 and k % 2) or (p == 2 and len(c) != 7):
                lay.set(p, k, _pad(c, 255, 20000 + 300 * p + k))
    assert all(len(c) == 255 for c in lay.planes[0].chunks)
    frame = coefgen.compose(lay.blocks(), w, h, Q50, oracle)
    check(decoders, oracle, lay.payload(), w, h, Q50, expect=(0, -1), frame=frame)


# ---- error order -------------------------------------------------------------------
@pytest.mark.parametrize("spots", [((70, "bits_out_len3"), (200, "size2")), ((200, "nomatch_8left"), (3, "nbits513")),
                                   ((255, "size1"), (64, "bits_out_len8"))],
                         ids=["passes_1_3", "passes_3_0", "passes_3_1"])
def test_two_bad_chunks_in_different_passes(decoders, oracle, chunks, pools, spots):
    """An all-busy span (four passes) with two bad chunks: the lowest block's
    code is reported, whichever pass finds it."""
    w, h = 128, 128
    single, busy = pools
    rng = np.random.default_rng(11)
    planes = [busy[rng.integers(0, len(busy), 256)], single[rng.integers(0, len(single), 64)],
              single[rng.integers(0, len(single), 64)]]
    lay = layout_of(w, h, planes, chunks)
    bad = bad_chunks()
    for k, name in spots:
        lay.set(0, k, bad[name][0])
    k_low, name_low = min(spots)
    check(decoders, oracle, lay.payload(), w, h, Q50, expect=(bad[name_low][1], k_low))
    # ... and with closed forms between them (the bad chunks in passes 0 and 1 of 2)
    planes[0][1::2] = single[rng.integers(0, len(single), 128)]
    lay = layout_of(w, h, planes, chunks)
    for k, name in spots:
        lay.set(0, k & ~1, bad[name][0])
    check(decoders, oracle, lay.payload(), w, h, Q50, expect=(bad[name_low][1], k_low & ~1))


# ---- context reuse --------------------------------------------------------------------
def test_batch_of_three_different_frames(decoders, oracle, chunks, pools):
    w, h = 80, 208
    rng = np.random.default_rng(12)
    pays = [layout_of(w, h, mixed_planes(w, h, pools, rng, ps), chunks).payload() for ps in (0.5, 0.9, 0.1)]
    want = [oracle.decompress(p, w, h, Q50) for p in pays]
    assert len(set(want)) == 3
    for name, c in decoders.items():
        assert list(c.decompress_frames(pays, w, h, Q50)) == want, name


def test_large_small_large_on_one_context(decoders, oracle, chunks, pools):
    """A frame of many spans, a frame of 4 + 1 + 1 blocks, the first again: a
    list or a stage left over from the other frame must not be read."""
    rng = np.random.default_rng(13)
    big = layout_of(512, 512, mixed_planes(512, 512, pools, rng, 0.5), chunks).payload()
    small = layout_of(16, 16, mixed_planes(16, 16, pools, rng, 0.5), chunks).payload()
    flat = layout_of(16, 16, mixed_planes(16, 16, pools, rng, 1.0), chunks).payload()
    wb, ws, wf = (oracle.decompress(big, 512, 512, Q50), oracle.decompress(small, 16, 16, Q50),
                  oracle.decompress(flat, 16, 16, Q50))
    for name, c in decoders.items():
        for _ in range(2):
            assert c.decompress(big, 512, 512, Q50) == wb, name
            assert c.decompress(small, 16, 16, Q50) == ws, name
            assert c.decompress(flat, 16, 16, Q50) == wf, name


# ---- random sweep -----------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_random_sweep(decoders, oracle, chunks, pools, seed):
    rng = np.random.default_rng(9000 + seed)
    w, h = (16 * int(rng.integers(1, 33)) for _ in range(2))
    q = tuple(int(x) for x in rng.integers(10, 101, 3))
    lay = layout_of(w, h, mixed_planes(w, h, pools, rng, float(rng.choice([0.2, 0.5, 0.8, 0.97]))), chunks)
    code, _, _ = check(decoders, oracle, lay.payload(), w, h, q)
    assert code == 0

"""Single-class blocks (msz <= 1: the DC alone, or all zero) bypass K2's runs
and the stage: k_huff_encode stores a marker (kSrcSingle | the DC's low 11
bits, codec_common.hpp) at classification and k_stream_out forms the 7-byte
chunk from it.  Whole payloads byte for byte against the oracle, and the round
trip against the oracle's decode, on both kernel arrangements: frames of
single blocks alone (no K2 run at all), single / non-single blocks at every
position K4 treats specially (a plane's first and last block, a tile's last
block and the next tile's first, the neighbours of an overflow block), a
context that alternates frames with and without single blocks, and one batch
large enough for K2's 8-tile windows."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLAT, LOW, NOISE = 0, 1, 2
SINGLE_CHUNK = 7  # codec_common.hpp kSingleChunk


def chunk_tables(payload):
    """Per plane: the u8 chunk sizes and the chunks (the DCTYUV layout: u32
    plane_size[3]; per plane u32 nblocks, u32 content_size, u8 size[nblocks],
    the chunks back to back)."""
    planes, pos = [], 12
    for p in range(3):
        nb, content = struct.unpack_from("<II", payload, pos)
        sizes = np.frombuffer(payload, np.uint8, nb, pos + 8)
        at = pos + 8 + nb
        offs = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
        assert offs[-1] == content
        planes.append((sizes, [payload[at + offs[i]: at + offs[i + 1]] for i in range(nb)]))
        assert struct.unpack_from("<I", payload, 4 * p)[0] == 8 + nb + content
        pos = at + content
    assert pos == len(payload)
    return planes


def plane_pixels(kinds, bw, rng):
    """A plane of 8x8 blocks, row-major, of the given kinds: FLAT one pixel
    value (DC alone), LOW a two-level step (a few low-frequency
    coefficients), NOISE uniform random pixels."""
    bh = len(kinds) // bw
    assert bh * bw == len(kinds)
    blocks = np.empty((len(kinds), 8, 8), np.uint8)
    flat = rng.integers(0, 256, len(kinds))
    for i, k in enumerate(kinds):
        if k == FLAT:
            blocks[i] = flat[i]
        elif k == LOW:
            a, b = (40, 215) if i & 1 else (200, 30)
            blocks[i] = a
            if i & 2:
                blocks[i, :, 3 + (i >> 2) % 3:] = b
            else:
                blocks[i, 2 + (i >> 2) % 4:, :] = b
        else:
            blocks[i] = rng.integers(0, 256, (8, 8))
    return blocks.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def frame_of(kinds3, w, h, seed):
    rng = np.random.default_rng(seed)
    planes = [plane_pixels(kinds3[0], w // 8, rng), plane_pixels(kinds3[1], w // 16, rng),
              plane_pixels(kinds3[2], w // 16, rng)]
    return b"".join(p.tobytes() for p in planes)


def check_kinds(oracle, payload, kinds3, overflow):
    """The frame came out as intended: every FLAT block a 7-byte chunk, no
    other block one; with `overflow`, every NOISE block more than 8 distinct
    symbols (K2's overflow list) in a chunk past K4's register path (64
    source bytes)."""
    for (sizes, chunks), kinds in zip(chunk_tables(payload), kinds3):
        kinds = np.asarray(kinds)
        assert len(sizes) == len(kinds)
        assert (sizes[kinds == FLAT] == SINGLE_CHUNK).all()
        assert (sizes[kinds != FLAT] > SINGLE_CHUNK).all()
        if overflow:
            for i in np.nonzero(kinds == NOISE)[0]:
                c = oracle.huff_decode_block(chunks[i])
                assert len(set(c.tolist())) > 8 and sizes[i] > 64, i


def roundtrip(codec, oracle, frame, w, h, q):
    exp = oracle.compress(frame, w, h, q)
    assert codec.compress(frame, w, h, q) == exp
    assert codec.decompress(exp, w, h, q) == oracle.decompress(exp, w, h, q)
    return exp


def batch_payloads(codec, frames, w, h, q):
    import torch
    import myyuv_hip
    n = len(frames)
    cap = (myyuv_hip.payload_bound(w, h) + 3) & ~3
    d_in = torch.frombuffer(bytearray(b"".join(frames)), dtype=torch.uint8).cuda()
    d_pay = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    codec.reserve_batch(w, h, n)
    codec.compress_batch_device(d_in.data_ptr(), n, w, h, q, d_pay.data_ptr(), cap, d_sizes.data_ptr(), stream)
    rc, bad = codec.sync_status(stream)
    assert rc == 0, (rc, bad)
    return d_pay, d_sizes.cpu().numpy(), cap


FLAT_VALUES = (0, 1, 127, 128, 129, 255)
Q50 = (50, 50, 50)


def test_all_single_frames(codec, oracle):
    """16x16 flat frames: 4 + 1 + 1 blocks, every plane one tile, every block
    single: K2's windows have no run and must still publish their totals.
    At least one of the values quantises to a zero DC (msz = 0, the all-zero
    block's chunk)."""
    w = h = 16
    frames = [bytes([v]) * (w * h * 3 // 2) for v in FLAT_VALUES]
    zero_dc = 0
    exps = []
    for fr in frames:
        exp = roundtrip(codec, oracle, fr, w, h, Q50)
        for sizes, chunks in chunk_tables(exp):
            assert (sizes == SINGLE_CHUNK).all()
            zero_dc += sum(not oracle.huff_decode_block(c).any() for c in chunks)
        exps.append(exp)
    assert zero_dc > 0
    for part in (slice(0, 3), slice(3, 6)):
        d_pay, sizes, cap = batch_payloads(codec, frames[part], w, h, Q50)
        pay = d_pay.cpu().numpy()
        for i, exp in enumerate(exps[part]):
            assert bytes(pay[i * cap: i * cap + int(sizes[i])]) == exp, i


# 144 x 272: luma 18 x 34 = 612 blocks = tiles of 256 / 256 / 100, chroma 153 each
EW, EH = 144, 272
OVF_AT = (100, 300)  # luma overflow blocks whose neighbours are pinned (their tiles' inner blocks)


def edge_kinds(n, pinned_kind, seed, ovf_at=()):
    """Block kinds of a plane of n blocks: a seeded mix, with the positions K4
    treats specially (the plane's first and last block, each tile's block 255
    and the next tile's block 0, the neighbours of the blocks `ovf_at`) all of
    `pinned_kind`, and the `ovf_at` blocks NOISE."""
    rng = np.random.default_rng(seed)
    kinds = rng.choice([FLAT, FLAT, LOW, NOISE], n)
    pins = {0, n - 1}
    for t in range(256, n, 256):
        pins |= {t - 1, t}
    for j in ovf_at:
        pins |= {j - 1, j + 1}
    for i in pins:
        kinds[i] = pinned_kind
    for j in ovf_at:
        kinds[j] = NOISE
    return kinds


@pytest.mark.parametrize("q", [(50, 50, 50), (100, 100, 100)])
@pytest.mark.parametrize("pinned", [FLAT, LOW], ids=["edges_single", "edges_not_single"])
def test_tile_plane_and_neighbour_edges(codec, oracle, q, pinned):
    kinds3 = [edge_kinds(612, pinned, 1, OVF_AT), edge_kinds(153, pinned, 2, (70,)),
              edge_kinds(153, pinned, 3, (80,))]
    frame = frame_of(kinds3, EW, EH, 4)
    exp = roundtrip(codec, oracle, frame, EW, EH, q)
    check_kinds(oracle, exp, kinds3, overflow=q[0] == 100)
    # the batch path: the other pinning as the neighbouring frame
    other = [edge_kinds(612, FLAT + LOW - pinned, 1, OVF_AT), edge_kinds(153, FLAT + LOW - pinned, 2, (70,)),
             edge_kinds(153, FLAT + LOW - pinned, 3, (80,))]
    frames = [frame, frame_of(other, EW, EH, 4), frame]
    d_pay, sizes, cap = batch_payloads(codec, frames, EW, EH, q)
    pay = d_pay.cpu().numpy()
    for i, fr in enumerate(frames):
        assert bytes(pay[i * cap: i * cap + int(sizes[i])]) == oracle.compress(fr, EW, EH, q), i


def test_stale_stage(codec, oracle):
    """One context: a frame without a single block, an all-single frame of the
    same geometry, the first again.  K4 must not read the stage for a marked
    block, and K2 must leave no totals behind."""
    busy3 = [np.where(np.arange(n) % 3 == 0, NOISE, LOW) for n in (612, 153, 153)]
    flat3 = [np.full(n, FLAT) for n in (612, 153, 153)]
    busy, flat = frame_of(busy3, EW, EH, 5), frame_of(flat3, EW, EH, 6)
    e_busy, e_flat = oracle.compress(busy, EW, EH, Q50), oracle.compress(flat, EW, EH, Q50)
    check_kinds(oracle, e_busy, busy3, overflow=False)
    check_kinds(oracle, e_flat, flat3, overflow=False)
    for fr, exp in ((busy, e_busy), (flat, e_flat), (busy, e_busy), (flat, e_flat)):
        assert codec.compress(fr, EW, EH, Q50) == exp


@pytest.fixture(scope="module")
def big_frame(oracle):
    """A 2048x2048 frame built like the edge frames, its oracle stream and
    decode (once for both arrangements)."""
    w = h = 2048
    kinds3 = [edge_kinds(65536, FLAT, 7, (1000, 40000)), edge_kinds(16384, LOW, 8, (500,)),
              edge_kinds(16384, FLAT, 9, (9000,))]
    frame = frame_of(kinds3, w, h, 10)
    exp = oracle.compress(frame, w, h, Q50)
    check_kinds(oracle, exp, kinds3, overflow=False)
    return frame, exp, oracle.decompress(exp, w, h, Q50)


def test_eight_tile_windows(codec, big_frame):
    """One batch whose tile count reaches kWinBigTiles (16,384): 44 copies of
    a 2048x2048 frame (384 tiles each) take k_huff_encode<8>; the same frame
    in a 2-frame batch takes <4>.  Compared on the device."""
    import torch
    import myyuv_hip
    w = h = 2048
    n = 44
    assert myyuv_hip.batch_tiles(w, h) == 384 and n * 384 >= 16384 > 2 * 384
    frame, exp, dec = big_frame
    d_exp = torch.frombuffer(bytearray(exp), dtype=torch.uint8).cuda()
    for nf in (n, 2):
        d_pay, sizes, cap = batch_payloads(codec, [frame] * nf, w, h, Q50)
        assert (sizes == len(exp)).all()
        for i in range(nf):
            assert torch.equal(d_pay[i * cap: i * cap + len(exp)], d_exp), (nf, i)
    assert codec.decompress(exp, w, h, Q50) == dec

"""What crop and join must return, stated with numpy straight from the
definition in include/myyuv_hip.h ("Crop and join"): streams are parsed into
per-plane size tables and chunk lists, the chunks are picked by block index
and a stream is built again.  Nothing here calls the code under test."""
import struct

import numpy as np


def plane_dims(w, h):
    """(blocks per row, block rows) of the planes Y, U, V of a w x h frame."""
    return (w // 8, h // 8), (w // 16, h // 16), (w // 16, h // 16)


def plane_counts(w, h):
    return tuple(bw * bh for bw, bh in plane_dims(w, h))


def parse(payload, w, h):
    """[(sizes uint8[blocks], [chunk bytes, ...])] per plane: the plane's first
    `blocks` size bytes and the chunks they place inside its content."""
    pay = bytes(payload)
    ps = struct.unpack_from("<3I", pay, 0)
    off, out = 12, []
    for p, n in enumerate(plane_counts(w, h)):
        hn, hc = struct.unpack_from("<2I", pay, off)
        assert hn >= n
        sizes = np.frombuffer(pay, np.uint8, n, off + 8).copy()
        content = pay[off + 8 + hn: off + 8 + hn + hc]
        ends = np.cumsum(sizes.astype(np.int64))
        starts = ends - sizes
        out.append((sizes, [content[int(a):int(b)] for a, b in zip(starts, ends)]))
        off += ps[p]
    return out


def build(planes):
    """The DCTYUV stream of [(sizes, chunks)] per plane, as DCTYUV::dump lays it
    out: plane_size = 8 + nblocks + content_size, no slack."""
    bodies = []
    for sizes, chunks in planes:
        content = b"".join(chunks)
        sizes = np.asarray(sizes, np.uint8)
        bodies.append(struct.pack("<2I", len(sizes), len(content)) + sizes.tobytes() + content)
    return struct.pack("<3I", *(len(b) for b in bodies)) + b"".join(bodies)


def crop_stream(payload, w, h, region):
    """The stream of the rw x rh frame: block (by', bx') of plane p is the
    source plane's block (ry/d + by') * bw + rx/d + bx', size byte and chunk."""
    rx, ry, rw, rh = region
    assert all(v % 16 == 0 for v in region) and rw > 0 and rh > 0 and rx + rw <= w and ry + rh <= h
    src = parse(payload, w, h)
    out = []
    for p, ((bw, _), (sizes, chunks)) in enumerate(zip(plane_dims(w, h), src)):
        d = 8 if p == 0 else 16
        idx = [(ry // d + by) * bw + rx // d + bx for by in range(rh // d) for bx in range(rw // d)]
        out.append((sizes[idx], [chunks[k] for k in idx]))
    return build(out)


def join_stream(payloads, cols, rows, tw, th):
    """The stream of the (cols*tw) x (rows*th) frame: block (by', bx') of plane
    p is block (by' mod bh_t) * bw_t + bx' mod bw_t of tile (by' div bh_t) *
    cols + bx' div bw_t."""
    assert len(payloads) == cols * rows and cols >= 1 and rows >= 1 and tw % 16 == 0 and th % 16 == 0
    tiles = [parse(p, tw, th) for p in payloads]
    out = []
    for p, (bwt, bht) in enumerate(plane_dims(tw, th)):
        sizes, chunks = [], []
        for by in range(bht * rows):
            for bx in range(bwt * cols):
                t = (by // bht) * cols + bx // bwt
                k = (by % bht) * bwt + bx % bwt
                sizes.append(tiles[t][p][0][k])
                chunks.append(tiles[t][p][1][k])
        out.append((np.asarray(sizes, np.uint8), chunks))
    return build(out)


def tile_rect(t, cols, tw, th):
    return ((t % cols) * tw, (t // cols) * th, tw, th)


def synthetic(w, h, sizes_per_plane, seed):
    """A stream with the given size bytes (0..255 each, one sequence per plane)
    and random content bytes: legal input, because the gather never parses a
    chunk.  At least one size per plane must be non-zero (content_size 0 is a
    header error)."""
    rng = np.random.default_rng(seed)
    planes = []
    for n, sizes in zip(plane_counts(w, h), sizes_per_plane):
        sizes = np.asarray(sizes, np.uint8)
        assert sizes.shape == (n,) and sizes.any()
        planes.append((sizes, [rng.integers(0, 256, int(s), dtype=np.uint8).tobytes() for s in sizes]))
    return build(planes)


def overrun_stream(w, h, content_bytes, seed):
    """A stream whose every size byte is 255 and whose plane p declares (and
    holds) only content_bytes[p] bytes of content: the headers pass, the size
    tables overrun the content by far more than the stream is long.  Blocks
    that end inside the content are whole chunks of random bytes."""
    rng = np.random.default_rng(seed)
    planes = []
    for n, nbytes in zip(plane_counts(w, h), content_bytes):
        assert 1 <= nbytes <= 255 * n
        planes.append((np.full(n, 255, np.uint8), [rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()]))
    return build(planes)


def random_sizes(w, h, seed, lo=0, hi=256):
    rng = np.random.default_rng(seed)
    out = []
    for n in plane_counts(w, h):
        s = rng.integers(lo, hi, n).astype(np.uint8)
        if not s.any():
            s[-1] = 1
        out.append(s)
    return out


def assemble(frames, cols, rows, tw, th):
    """The IYUV frame (bytes) of cols x rows IYUV tiles of tw x th."""
    planes = [[], [], []]
    for f in frames:
        a = np.frombuffer(bytes(f), np.uint8)
        planes[0].append(a[: tw * th].reshape(th, tw))
        planes[1].append(a[tw * th: tw * th * 5 // 4].reshape(th // 2, tw // 2))
        planes[2].append(a[tw * th * 5 // 4:].reshape(th // 2, tw // 2))
    return b"".join(np.block([[pl[r * cols + c] for c in range(cols)] for r in range(rows)]).tobytes()
                    for pl in planes)


# ---- the run map (csrc/stream_gather.h), restated -----------------------------
def runs(cols, rows, sbw, bx, by, tbw, tbh):
    """[(plane, dst first block, stream, src first block, count)] in run order
    for per-plane lists sbw, bx, by, tbw, tbh: every output row splits at the
    pieces' borders, each piece row every 64 blocks."""
    out = []
    for p in range(3):
        for row in range(tbh[p] * rows):
            ty, ly = divmod(row, tbh[p])
            for tx in range(cols):
                for lx in range(0, tbw[p], 64):
                    out.append((p, row * tbw[p] * cols + tx * tbw[p] + lx, ty * cols + tx,
                                (by[p] + ly) * sbw[p] + bx[p] + lx, min(64, tbw[p] - lx)))
    return out


def crop_runs(w, h, region):
    rx, ry, rw, rh = region
    d = (8, 16, 16)
    return runs(1, 1, [w // k for k in d], [rx // k for k in d], [ry // k for k in d], [rw // k for k in d],
                [rh // k for k in d])


def join_runs(cols, rows, tw, th):
    d = (8, 16, 16)
    return runs(cols, rows, [tw // k for k in d], [0] * 3, [0] * 3, [tw // k for k in d], [th // k for k in d])

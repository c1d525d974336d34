"""Every crafted stream of tests/streamcases.py on every decode path of the
GPU, in both kernel arrangements (the `codec` fixture): the outcome is the
case's own by-construction expectation, which tests/test_stream_cases.py
pins to the oracle (oracle.decompress_ex) and to the reference.

Bounds (why these hostile streams cannot make a kernel read or write outside
an allocation) are argued per family in streamcases' docstring; here every
device buffer is allocated to the `cap` that is passed (never smaller), the
bytes of a slot after the stream hold a non-zero pattern, and the outputs of
the device calls sit between 4 KiB sentinels that are checked.
"""
import numpy as np
import pytest

import colorref
import coefgen
import regionref
import scaleref
import streamcases

pytestmark = pytest.mark.gpu

NAMES = streamcases.names()
GUARD = 4096
SENTINEL = 0xC3


@pytest.fixture(scope="module")
def by_name(oracle):
    return {c.name: c for c in streamcases.cases(oracle)}


_FRAMES = {}


def frame_of(c, oracle):
    """The case's (repaired) decode, computed once per distinct block set."""
    key = (c.w, c.h, b"".join(np.ascontiguousarray(b).tobytes() for b in c.blocks))
    if key not in _FRAMES:
        _FRAMES[key] = c.frame(oracle)
    return _FRAMES[key]


def outcome(call):
    """(code, bad_block, result) of a host-buffer call."""
    import myyuv_hip

    try:
        return 0, None, call()
    except myyuv_hip.CodecError as e:
        return e.code, e.bad_block, None


def cap_for(*payloads):
    return max(64, (max(len(p) for p in payloads) + 3 & ~3) + 64)


def slots(payloads, cap, seed):
    """Device slots of `cap` bytes each: the stream, then a seeded non-zero
    pattern up to the slot's end."""
    import torch

    buf = np.random.default_rng(seed).integers(1, 256, len(payloads) * cap, dtype=np.uint8)
    for f, p in enumerate(payloads):
        assert len(p) <= cap
        buf[f * cap: f * cap + len(p)] = np.frombuffer(bytes(p), np.uint8)
    return torch.from_numpy(buf).cuda()


class Guarded:
    """`n` output bytes on the device between two 4 KiB sentinels."""

    def __init__(self, n):
        import torch

        self.n = n
        self.t = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return self.t.data_ptr() + GUARD

    def check(self):
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == SENTINEL).all(), "bytes written in front of the output"
        assert (a[GUARD + self.n:] == SENTINEL).all(), "bytes written after the output"
        return a[GUARD:GUARD + self.n].tobytes()


def device_decode(codec, payloads, w, h, q, seed, sizes=None, cap=None):
    """decompress_device (one stream) or decompress_batch_device; returns
    (code, bad_block, frames bytes), the sentinels checked."""
    import torch

    n = len(payloads)
    cap = cap or cap_for(*payloads)
    d_in = slots(payloads, cap, seed)
    d_sz = torch.tensor(sizes or [len(p) for p in payloads], dtype=torch.int32, device="cuda")
    out = Guarded(n * w * h * 3 // 2)
    stream = torch.cuda.current_stream().cuda_stream
    if n == 1:
        codec.decompress_device(d_in.data_ptr(), d_sz.data_ptr(), cap, w, h, q, out.ptr(), stream)
    else:
        codec.decompress_batch_device(d_in.data_ptr(), d_sz.data_ptr(), cap, n, w, h, q, out.ptr(), stream)
    rc, bad = codec.sync_status(stream)
    return rc, (bad if rc else None), out.check()


def test_case_names_are_the_generators(oracle):
    assert set(NAMES) == {c.name for c in streamcases.build(oracle)} and len(NAMES) == len(set(NAMES))


@pytest.mark.parametrize("name", NAMES)
def test_full_decode(codec, oracle, by_name, name):
    """decompress, decompress_to_bmp and decompress_device (guard bands, two
    patterns after the stream); after a rejected stream the context decodes a
    valid one."""
    c = by_name[name]
    want = frame_of(c, oracle)
    code, bad, got = outcome(lambda: codec.decompress(c.payload, c.w, c.h, c.q))
    assert (code, bad) == c.expect, (c.branch, code, bad)
    if c.kind == "accept":
        assert got == want, c.branch
    code, bad, got = outcome(lambda: codec.decompress_to_bmp(c.payload, c.w, -c.h, c.q, 32, colorref.LINEAR))
    assert (code, bad) == c.expect, ("to_bmp", c.branch, code, bad)
    if c.kind == "accept":
        assert got == colorref.to_bmp(want, c.w, -c.h, 32, colorref.LINEAR), c.branch
    for seed in (1, 2) if c.kind != "accept" else (1,):
        code, bad, got = device_decode(codec, [c.payload], c.w, c.h, c.q, seed)
        assert (code, bad) == c.expect, ("device", seed, c.branch, code, bad)
        if c.kind == "accept":
            assert got == want, c.branch
    if c.kind != "accept":
        assert codec.decompress(c.repaired, c.w, c.h, c.q) == want, "the context after an error"
        code, bad, got = device_decode(codec, [c.repaired], c.w, c.h, c.q, 3)
        assert (code, bad, got) == (0, None, want), "the context after an error (device)"


_SCALED = {}


def scaled_frame(c, oracle, denom):
    """scaleref's transform of the case's own blocks (the accepted streams'
    size tables are not what scaleref.parse_planes expects), computed once
    per distinct block set and scale."""
    key = (c.w, c.h, denom, b"".join(np.ascontiguousarray(b).tobytes() for b in c.blocks))
    if key not in _SCALED:
        _SCALED[key] = _scaled_frame(c, oracle, denom)
    return _SCALED[key]


def _scaled_frame(c, oracle, denom):
    N = 8 // denom
    out = []
    for p, blocks in enumerate(c.blocks):
        pw, ph = (c.w, c.h) if p == 0 else (c.w // 2, c.h // 2)
        bw, bh = pw // 8, ph // 8
        px = scaleref.scaled_blocks(coefgen.natural(blocks), oracle.qtable(c.q[p], p != 0), N)
        out.append(px.reshape(bh, bw, N, N).transpose(0, 2, 1, 3).reshape(bh * N, bw * N).tobytes())
    return b"".join(out)


@pytest.mark.parametrize("name", NAMES)
def test_scaled_decode(codec, oracle, by_name, name):
    c = by_name[name]
    for denom in scaleref.DENOMS:
        code, bad, got = outcome(lambda: codec.decompress_scaled(c.payload, c.w, c.h, c.q, denom))
        assert (code, bad) == c.expect, (denom, c.branch, code, bad)
        if c.kind == "accept":
            assert got == scaled_frame(c, oracle, denom), (denom, c.branch)
    if c.kind != "accept":
        assert codec.decompress_scaled(c.repaired, c.w, c.h, c.q, 2) == scaled_frame(c, oracle, 2)


def rects(c):
    """Candidate rectangles: around every detecting block of the first
    fault, a few fixed ones, the whole frame."""
    out = [(0, 0, c.w, c.h)]
    ny, nc, _ = regionref.blocks(c.w, c.h)
    for f in c.faults:
        for g in (min(f.detect), max(f.detect)):
            p = 0 if g < ny else (1 if g < ny + nc else 2)
            out.append(regionref.block_rect(c.w, c.h, p, g - (0, ny, ny + nc)[p]))
    if c.w >= 64 and c.h >= 64:
        out += [(0, 0, 16, 16), (c.w - 48, c.h - 32, 48, 32), (64, 32, 80, 48), (16, 16, c.w - 16, 16)]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_region_decode(codec, oracle, by_name, name):
    """A rectangle that contains a faulty block reports the full frame's code
    and index; one that does not decodes to the crop of the repaired stream's
    frame; header faults fail every rectangle."""
    c = by_name[name]
    want = frame_of(c, oracle)
    hit = miss = 0
    for r in rects(c):
        exp = c.region_expect(c.w, c.h, r, regionref.contains_block)
        code, bad, got = outcome(lambda: codec.decompress_region(c.payload, c.w, c.h, c.q, r))
        assert (code, bad) == exp, (r, c.branch, code, bad)
        if exp[0] == 0:
            assert got == regionref.crop(want, c.w, c.h, r), (r, c.branch)
            miss += 1
        else:
            hit += 1
    if c.kind != "accept":
        assert hit >= 1
        whole_plane = any(len(f.detect) >= regionref.blocks(c.w, c.h)[1] for f in c.faults)
        if c.faults and c.w >= 64 and not whole_plane:
            assert miss >= 1, "no rectangle avoids the fault"


def pick(by_name, *names):
    """The cases of these names; a name ending in '*' is a prefix (the first
    case in the generator's order that starts with it)."""
    out = []
    for n in names:
        out.append(by_name[n] if not n.endswith("*") else
                   next(c for k, c in by_name.items() if k.startswith(n[:-1])))
    return out


def batch_mixes(by_name):
    """(streams, expected) of three-frame batches of one geometry:
    [valid, fault at block k, fault at a lower block j] -> 1 * nblk + k."""
    out = []
    for a, b in (("chunk_bits_out_len3_p1k63", "chunk_size2_p0k0"),
                 ("chunk_bits_out_len3_p2k30", "overrun_p1_mid_208"),
                 ("overrun_p2_last_208", "chunk_size2_p0k63"),
                 ("overrun_p0_mid_208", "chunk_size2_p0k0"),
                 ("chunk_bits_out_len3_p0k3_16", "chunk_size2_p0k0_16")):
        ca, cb = pick(by_name, a, b)
        assert ca.nblk == cb.nblk and ca.expect[1] > cb.expect[1] or ca.expect[0] == 9
        k = ca.expect[1] if ca.expect[1] >= 0 else 0  # (a plane-0 overrun of frame 1: that frame's block 0)
        out.append(([ca.repaired, ca.payload, cb.payload], ca, (ca.expect[0], ca.nblk + k)))
    return out


def test_batch_reports_the_lowest_frame_and_block(codec, oracle, by_name):
    for streams, c, exp in batch_mixes(by_name):
        code, bad, _ = device_decode(codec, streams, c.w, c.h, c.q, 5)
        assert (code, bad) == exp, ("device", c.name)
        code, bad, _ = outcome(lambda: codec.decompress_frames(streams, c.w, c.h, c.q))
        assert (code, bad) == exp, ("host", c.name)
        # the context afterwards
        code, bad, got = device_decode(codec, [c.repaired] * 3, c.w, c.h, c.q, 6)
        assert (code, bad, got) == (0, None, frame_of(c, oracle) * 3)


def test_batch_header_fault_in_frame_2(codec, oracle, by_name):
    """On the device every header fault of frame 2 reports 2 * nblk.  The
    host batch checks the headers on the host first (-1), except the chunk
    count against the geometry, which only the device knows (2 * nblk)."""
    for name in ("hdr_size12_208", "hdr_cut1_16", "hdr_ps_is_8_p1*", "hdr_hn_is_0_p1*", "hdr_hc_is_0_p2*",
                 "hdr_ps_minus_1_p2*", "hdr_hn_short_by_1_p0*", "hdr_hn_short_by_1_p1*", "hdr_hn_short_by_1_p2*",
                 "hdr_ps_ffffffff_p0*", "hdr_hn_ffffffff_p2*", "hdr_hc_ffffffff_p0*",
                 "precedence_hn2_chunk0_208"):
        c, = pick(by_name, name)
        streams = [c.repaired, c.repaired, c.payload]
        code, bad, _ = device_decode(codec, streams, c.w, c.h, c.q, 7)
        assert (code, bad) == (c.expect[0], 2 * c.nblk), ("device", name)
        code, bad, _ = outcome(lambda: codec.decompress_frames(streams, c.w, c.h, c.q))
        on_device = c.branch in ("parse_stream: hn < blocks", "order: header fault against chunk fault")
        assert (code, bad) == (c.expect[0], 2 * c.nblk if on_device else -1), ("host", name)


def test_batch_of_accepted_streams(codec, oracle, by_name):
    for names in (("odd_all_16", "padded_16", "odd_extremes_16"),
                  ("two_rounds_208", "odd_table80_split_p*", "odd_len7_x64_p*"),
                  ("slack_208", "odd_kraft_wrap_p*", "odd_table66_regular_p*")):
        cs = pick(by_name, *names)
        want = b"".join(frame_of(c, oracle) for c in cs)
        assert len({frame_of(c, oracle) for c in cs}) == 3 and len({c.payload for c in cs}) == 3
        streams = [c.payload for c in cs]
        code, bad, got = device_decode(codec, streams, cs[0].w, cs[0].h, cs[0].q, 8)
        assert (code, bad) == (0, None) and got == want, names
        got = codec.decompress_frames(streams, cs[0].w, cs[0].h, cs[0].q)
        assert b"".join(got) == want, names


@pytest.mark.parametrize("name", ["padded_208", "group_255x64_256", "odd_all_16"])
def test_size_word_is_clamped_to_cap(codec, oracle, by_name, name):
    """A valid stream whose size word is larger than cap decodes as the
    stream cut at cap does in the oracle (here: cap a few bytes short of the
    stream, so the cut stream fails its header's total; and cap = the
    stream's size rounded up, so it decodes)."""
    c = by_name[name]
    n = len(c.payload)
    for cap in (n + 3 & ~3, (n & ~3) - 4):
        cut = c.payload[:cap]
        exp_code, exp_bad, exp_frame = oracle.decompress_ex(cut, c.w, c.h, c.q)
        code, bad, got = device_decode(codec, [cut], c.w, c.h, c.q, 9, sizes=[n + 1000], cap=cap)
        assert (code, bad if code else -1) == (exp_code, exp_bad), (cap, n)
        if exp_code == 0:
            assert got == exp_frame
    assert exp_code == 6

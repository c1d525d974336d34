"""tests/streamcases.py against the CPU decoders (no GPU): the expectation each
case carries was written down from how the stream was built; here the oracle
(oracle.decompress_ex) must agree with every one, and the reference's own
library with the accepted and the defined ones.  The GPU side of the same
list is tests/test_gpu_stream_cases.py."""
import os
import re
import struct

import pytest

import coefgen
import streamcases
from conftest import ROOT
from oracle import ref


@pytest.fixture(scope="module")
def cases(oracle):
    return streamcases.cases(oracle)


@pytest.fixture(scope="module")
def chunks(oracle):
    return coefgen.Chunks(oracle.huff_encode_block)


@pytest.fixture(scope="module")
def ref_ready():
    if not ref.available("serial"):
        pytest.skip("oracle/_ref not built (`make -C oracle ref`)")


def header_messages():
    """code -> the reference's message, from the comments of include/myyuv_hip.h."""
    text = open(os.path.join(ROOT, "include", "myyuv_hip.h")).read()
    out = {}
    for m in re.finditer(r'#define MYYUV_E_\w+ (\d+)\s*/\* [\w.:,]+ "([^"]+)"', text):
        out[int(m.group(1))] = m.group(2)
    return out


def test_expectation_equals_oracle(oracle, cases):
    for c in cases:
        code, bad, frame = oracle.decompress_ex(c.payload, c.w, c.h, c.q)
        if c.kind == "accept":
            assert (code, frame is not None) == (0, True), c.name
            assert c.expect == (0, None), c.name
        else:
            assert c.expect[0] != 0 and c.repaired is not None, c.name
            assert (code, bad) == c.expect, (c.name, c.branch)
        # `decompress` keeps its behaviour: the code as an exception
        if code:
            with pytest.raises(RuntimeError) as e:
                oracle.decompress(c.payload, c.w, c.h, c.q)
            assert e.value.args[0] == code, c.name


def test_repaired_streams_decode(oracle, cases):
    seen = {}
    for c in cases:
        if c.kind == "accept":
            continue
        if c.repaired not in seen:
            code, bad, frame = oracle.decompress_ex(c.repaired, c.w, c.h, c.q)
            assert (code, bad) == (0, -1), c.name
            seen[c.repaired] = frame
        assert seen[c.repaired] == c.frame(oracle), c.name
        assert c.repaired != c.payload, c.name


def test_accepted_streams_decode_to_their_blocks(oracle, cases, chunks):
    for c in cases:
        if c.kind != "accept":
            continue
        assert c.payload != c.plain(chunks), c.name
        assert oracle.decompress(c.payload, c.w, c.h, c.q) == c.frame(oracle), (c.name, c.branch)
        assert oracle.decompress(c.plain(chunks), c.w, c.h, c.q) == c.frame(oracle), c.name


def test_region_expectations_are_consistent(cases):
    """A whole-frame region meets what the full decode meets."""
    import regionref

    for c in cases:
        got = c.region_expect(c.w, c.h, (0, 0, c.w, c.h), regionref.contains_block)
        assert got == c.expect, c.name


def test_reference_decodes_accepted(oracle, cases, ref_ready):
    for c in cases:
        if c.kind == "accept":
            assert ref.decompress(c.payload, c.w, c.h, c.q, variant="serial") == \
                oracle.decompress(c.payload, c.w, c.h, c.q), (c.name, c.branch)


def test_reference_raises_the_mapped_message(cases, ref_ready):
    msgs = header_messages()
    assert set(msgs) >= {6, 7, 8, 9, 10, 11}
    n = 0
    for c in cases:
        if c.kind != "defined":
            continue
        with pytest.raises(ref.RefError) as e:
            ref.decompress(c.payload, c.w, c.h, c.q, variant="serial")
        assert str(e.value) == msgs[c.expect[0]], (c.name, c.branch)
        n += 1
    assert n >= 20


def test_manifest(cases):
    branches = (
        "parse_stream: size <= 12",
        "parse_stream: 12+ps0+ps1+ps2 > size",
        "parse_stream: ps <= 8",
        "parse_stream: hn == 0",
        "parse_stream: hc == 0",
        "parse_stream: 8+hn+hc > ps",
        "parse_stream: hn < blocks",
        "parse_stream: 64-bit sums",
        "parse_table: s < 3",
        "parse_table: nbits > 512",
        "parse_table: 3+tb+ceil(nbits/8) > s",
        "parse_table: group overruns tb",
        "parse_table: more than 64 entries of one length",
        "decode: bits run out at code length 2..8",
        "decode: no match, >= 8 bits left (11) / fewer (10)",
        "decode: Kraft-oversubscribed table, uint8 first wraps",
        "decode_general_to: empty length / cd < first (neg)",
        "decode_group: rel+s > content_size",
        "order: lowest block of two bad chunks",
        "order: content overrun against chunk errors",
        "order: header fault against chunk fault",
        "accept: trailing bytes after plane 2",
        "accept: slack at a plane's end",
        "accept: hn > blocks",
        "accept: content_size > sum of sizes",
        "accept: chunks longer than their message, junk after the bits",
        "accept: 64 chunks of 255 B in one group",
        "accept: chunk 00 00 00",
        "accept: 64 symbols exactly / with bits left over",
        "accept: unused and duplicate table entries",
        "accept: values -1024 and 1023",
        "accept: 3+tb = 20 / 21",
        "accept: table of more than 64 entries",
        "accept: 64 entries of one length",
    )
    assert tuple(streamcases.BRANCHES) == branches
    targeted = {}
    for c in cases:
        targeted.setdefault(c.branch, []).append(c.name)
    assert set(targeted) == set(branches)
    for c in cases:
        assert c.kind in ("accept", "defined", "strict"), c.name
        assert not hasattr(c, "skip") and not hasattr(c, "xfail") and not hasattr(c, "marks"), c.name
        assert (c.w, c.h) in ((16, 16), (208, 96), (256, 192)), c.name
    # every plane, lane 0, lane 63, mid-group, first and last group carry a chunk fault
    spots = {(f.bad_block) for c in cases if (c.w, c.h) == (208, 96) for f in c.faults if f.code != 9}
    for g in (0, 63, 100, 311, 312, 375, 389, 454, 420):
        assert g in spots, g
    # "one short of the plane's blocks" is never the hn == 0 check, and every plane has one
    short = [c for c in cases if c.branch == "parse_stream: hn < blocks"]
    assert len(short) == 3
    for c in short + [c for c in cases if c.branch == "order: header fault against chunk fault"]:
        ps = struct.unpack_from("<III", c.payload, 0)
        hn = [struct.unpack_from("<I", c.payload, 12 + sum(ps[:p]))[0] for p in range(3)]
        want = coefgen.plane_counts(c.w, c.h)
        assert all(h > 0 for h in hn) and sum(h == n - 1 for h, n in zip(hn, want)) == 1, c.name
    # the bits run out before every length 2..8
    for L in range(2, 9):
        assert any(f"bits_out_len{L}_" in c.name for c in cases), L
    # both tables of more than 64 entries, in both small geometries
    for n in ("table80_split", "table66_regular"):
        assert sum(n in c.name for c in cases) >= 2, n

"""Requantise, the parts that need no GPU: the coefficient arithmetic of
csrc/requant.h (the code k_requant runs) compiled for the host
(tools/requant_host.cpp) against the numpy restatement (requantref) of the
definition in include/myyuv_hip.h, for every table-entry pair the tested
quality pairs produce; the restatement's own properties the GPU tests rely on
(identity, .5 ties, all-zero blocks, the clamp); the argument errors of the
CLI and the C ABI that come before any device is touched."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import regionref as R
import requantref as Q
import scaleref as S
from conftest import GOLDEN, PKG, ROOT

SRC = os.path.join(ROOT, "tools", "requant_host.cpp")
CLI = os.path.join(PKG, "myyuv_cli")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
QUALITIES = (1, 5, 20, 50, 70, 90, 100)
AW, AH = 208, 96
Z = np.arange(-1024, 1024, dtype=np.int16)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("requant") / "requant_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), SRC, "-o", exe],
                   check=True)
    return exe


def run(exe, qs, qd):
    qs, qd = np.ascontiguousarray(qs, np.float32), np.ascontiguousarray(qd, np.float32)
    r = subprocess.run([exe], input=struct.pack("<I", len(qs)) + qs.tobytes() + qd.tobytes(), capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-2000:])
    assert len(r.stdout) == len(qs) * 2048 * 2
    return np.frombuffer(r.stdout, np.int16).reshape(len(qs), 2048)


@pytest.fixture(scope="module")
def pairs(oracle):
    """Every distinct (Qs[i], Qd[i]) of the quality pairs over QUALITIES^2, luma and chroma."""
    seen = set()
    for chroma in (0, 1):
        t = {q: oracle.qtable(q, chroma) for q in QUALITIES}
        for a in QUALITIES:
            for b in QUALITIES:
                seen.update(zip(t[a].tolist(), t[b].tolist()))
    out = np.array(sorted(seen), np.float32)
    assert out.min() == 1 and out.max() == 255 and (out == np.round(out)).all()
    return out


def test_round_half_away():
    x = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999997, -0.49999997, 1022.5, -1023.5, 0.0, 8388607.5],
                 np.float32)
    assert Q.round_half_away(x).tolist() == [1, -1, 2, -2, 3, -3, 0, 0, 1023, -1024, 0, 8388608]


def test_shared_header_equals_numpy(harness, pairs):
    """All 2,048 values of z for every pair; the pairs reach both ends of the
    clamp, the identity and a few thousand exact .5 ties."""
    assert len(pairs) > 1000
    got = run(harness, pairs[:, 0], pairs[:, 1])
    t = Q.quotients(Z[None, :], pairs[:, :1], pairs[:, 1:])
    want = Q.requant(Z[None, :], pairs[:, :1], pairs[:, 1:])
    assert want.shape == got.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(pairs[i].tolist(), int(Z[j]), int(got[i, j]), int(want[i, j])) for i, j in bad[:4]]
    assert want.min() == -1024 and want.max() == 1023
    assert (Q.round_half_away(t) > 1023).any() and (Q.round_half_away(t) < -1024).any()  # the clamp works
    assert np.count_nonzero(Q.is_tie(t)) > 1000
    same = pairs[:, 0] == pairs[:, 1]
    assert same.sum() >= 50 and (got[same] == Z[None, :]).all()  # Qd == Qs: z' == z
    # the product is exact and below 2^24
    prod = Z[None, :].astype(np.float64) * pairs[:, :1].astype(np.float64)
    assert np.abs(prod).max() < 2 ** 24
    assert (Z[None, :].astype(np.float32) * pairs[:, :1] == prod).all()


def test_shared_header_equals_numpy_for_every_table_entry(harness):
    """The whole domain: Q tables hold integers 1..255, so 255 x 255 pairs
    times 2,048 values is every input the kernel's arithmetic can meet."""
    v = np.arange(1, 256, dtype=np.float32)
    qs, qd = np.repeat(v, 255), np.tile(v, 255)
    for k in range(0, len(qs), 8192):
        a, b = qs[k:k + 8192], qd[k:k + 8192]
        got = run(harness, a, b)
        want = Q.requant(Z[None, :], a[:, None], b[:, None])
        bad = np.argwhere(got != want)
        assert len(bad) == 0, [(float(a[i]), float(b[i]), int(Z[j]), int(got[i, j]), int(want[i, j]))
                               for i, j in bad[:4]]


def test_divide_is_not_a_reciprocal_multiply(pairs):
    """The definition's divide differs from z * Qs * fl(1 / Qd) after rounding
    for some of these values, so a kernel using the reciprocal would be seen."""
    t = Q.quotients(Z[None, :], pairs[:, :1], pairs[:, 1:])
    prod = Z[None, :].astype(np.float32) * pairs[:, :1]
    alt = prod * (np.float32(1) / pairs[:, 1:])
    assert alt.dtype == np.float32
    assert (Q.round_half_away(alt) != Q.round_half_away(t)).any()


# ---- the reference's own properties (they keep the GPU inputs honest) -------
def chunks_of(payload):
    out = []
    for sizes, content in S.parse_planes(payload):
        pos = 0
        for s in sizes:
            out.append(content[pos:pos + s])
            pos += s
    return out


@pytest.mark.parametrize("q", [(90, 90, 90), (50, 50, 50), (90, 50, 20)])
def test_identity_returns_the_source_bytes(oracle, q):
    pay, _ = R.tiled_stream(AW, AH, q)
    assert Q.cached(pay, q, q) == pay
    assert len(chunks_of(pay)) == 468


def test_q90_to_q50_has_ties(oracle):
    qs, qd = (90, 90, 90), (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, qs)
    planes = Q.requant_planes(pay, qs, qd)
    ties = sum(int(np.count_nonzero(Q.is_tie(t))) for _, t in planes)
    assert ties > 100
    out = Q.cached(pay, qs, qd)
    assert out != pay and len(out) < len(pay)
    # the result is a stream the oracle decodes, and not the recompressed bytes
    assert len(oracle.decompress(out, AW, AH, qd)) == AW * AH * 3 // 2
    assert out != oracle.compress(oracle.decompress(pay, AW, AH, qs), AW, AH, qd)


def test_q100_to_q1_has_all_zero_blocks(oracle):
    qs, qd = (100, 100, 100), (1, 1, 1)
    pay, _ = R.tiled_stream(AW, AH, qs)
    planes = Q.requant_planes(pay, qs, qd)
    src = S.coefficients(pay)
    zero = sum(int(np.count_nonzero(~nat.any(axis=1))) for nat, _ in planes)
    zero_src = sum(int(np.count_nonzero(~nat.any(axis=1))) for nat in src)
    assert zero > 50 and zero_src < 10  # requantising made most of them
    assert len(chunks_of(Q.cached(pay, qs, qd))) == 468


def test_q1_to_q100_grows_the_coefficients(oracle):
    """The other direction: a few small coefficients become large ones (the
    clamp itself is reached by coefgen's extreme streams, not by this frame)."""
    qs, qd = (1, 1, 1), (100, 100, 100)
    pay, _ = R.tiled_stream(AW, AH, qs)
    planes = Q.requant_planes(pay, qs, qd)
    src = S.coefficients(pay)
    assert all(nat.min() >= -1024 and nat.max() <= 1023 for nat, _ in planes)
    assert max(int(np.abs(nat).max()) for nat, _ in planes) > 20 * max(int(np.abs(nat).max()) for nat in src)
    assert Q.cached(pay, qs, qd) != pay


def test_extreme_streams_reach_the_clamp(oracle):
    import coefgen

    sh = coefgen.shared(oracle)
    s = sh.by_name["extreme_q1"]
    planes = Q.requant_planes(sh.payload(s.name), s.q, (100, 100, 100))
    assert any((Q.round_half_away(t) > 1023).any() for _, t in planes)
    assert any((Q.round_half_away(t) < -1024).any() for _, t in planes)
    assert all(nat.min() == -1024 and nat.max() == 1023 for nat, _ in planes)


# ---- argument errors that need no device -----------------------------------
def test_handle_and_pointer_errors_need_no_device():
    import myyuv_hip

    L = myyuv_hip.load()
    pay = np.zeros(64, np.uint8)
    out = np.zeros(64, np.uint8)
    qa = np.array([50, 50, 50], np.uint8)
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    size = ctypes.c_uint32(9)
    bad = ctypes.c_int64(7)
    assert L.myyuv_gpu_dct_requantize(None, u8(pay), 64, 16, 16, u8(qa), u8(qa), u8(out), 64, ctypes.byref(size),
                                      ctypes.byref(bad)) == myyuv_hip.E_ARG
    assert bad.value == -1 and size.value == 9
    assert L.myyuv_gpu_dct_requantize_device(None, 256, 512, 64, 1, 16, 16, u8(qa), u8(qa), 1024, 64, 2048,
                                             None) == myyuv_hip.E_ARG
    assert not (out != 0).any()
    assert "requant" in myyuv_hip.KERNELS and myyuv_hip.KERNELS.index("requant") == myyuv_hip.K_REQUANT == 15


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def test_cli_requantize_argument_errors(tmp_path):
    out = str(tmp_path / "x.myyuv")
    # an uncompressed input has no coefficients
    r = cli(RAW, "-requantize", "50", "-o", out)
    assert r.returncode == 1, r.stdout
    assert r.stdout.splitlines()[0] == \
        "Nothing to requantize, image is not compressed (-requantize needs DCT coefficients)"
    # no output file
    for tail in ([], ["50"], ["50", "-o"], ["50", "-o", out, "extra"]):
        r = cli(C50, "-requantize", *tail)
        assert r.returncode == 1 and "Usage" in r.stdout, (tail, r.stdout)
        assert r.stdout.splitlines()[0] == "Invalid argument, last arguments must be `-o /path/to/new_image.myyuv`"
    # the qualities, parsed as -compress DCT's (the exception propagates, as in the reference CLI)
    for params, msg in ((["0"], "must range between [1..100]"), (["101"], "must range between [1..100]"),
                        (["50", "50", "50", "50"], "Too many compression parameters"),
                        ([], "Too few compression parameters")):
        r = cli(C50, "-requantize", *params, "-o", out)
        assert r.returncode != 0 and msg in r.stderr, (params, r.returncode, r.stderr)
    assert not os.path.exists(out)
    assert "-requantize Q [Q [Q]] -o OUT.myyuv" in cli(C50, "-requantize").stdout

"""Transform, the parts that need no GPU: the in-block arithmetic and the
block-index map of csrc/coef_xform.h (the code k_coef_xform runs) compiled for
the host (tools/coef_xform_host.cpp) against the numpy restatement (xformref)
of the definition in include/myyuv_hip.h, for all eight operations; the same
program built with the address and undefined-behaviour sanitizers; the
restatement's own properties the GPU tests rely on; the argument errors of the
CLI and the C ABI that come before any device is touched."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import regionref as R
import scaleref as S
import xformref as X
from conftest import GOLDEN, PKG, ROOT

SRC = os.path.join(ROOT, "tools", "coef_xform_host.cpp")
CLI = os.path.join(PKG, "myyuv_cli")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
QUALITIES = (1, 20, 50, 90, 100)
SHAPES = ((1, 1), (2, 2), (26, 12), (12, 26), (260, 4), (4, 260))
AW, AH = 208, 96


def build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *flags, "-I", os.path.join(PKG, "csrc"), SRC,
                    "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("coef_xform"), "coef_xform_host")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("coef_xform_san"), "coef_xform_host_san", "-g",
                 "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def blocks_record(op, qs, qd, z):
    z = np.ascontiguousarray(z, np.int16).reshape(-1, 64)
    return (struct.pack("<III", 1, op, len(z)) + np.ascontiguousarray(qs, np.float32).tobytes() +
            np.ascontiguousarray(qd, np.float32).tobytes() + z.tobytes())


def map_record(op, bw, bh):
    return struct.pack("<IIII", 2, op, bw, bh)


def run(exe, stdin):
    r = subprocess.run([exe], input=stdin, capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-2000:])
    return r.stdout


def one_hot_blocks():
    """Every position x every value of +-1, 1023, -1024: 256 blocks."""
    out = np.zeros((64 * 4, 64), np.int16)
    for n in range(64):
        for k, v in enumerate((1, -1, 1023, -1024)):
            out[4 * n + k, n] = v
    return out


def dense_blocks(n=96, seed=11):
    rng = np.random.default_rng(seed)
    z = rng.integers(-1024, 1024, (n, 64)).astype(np.int16)
    z[: n // 3] = rng.integers(-40, 41, (n // 3, 64))  # small ones: the .5 ties of a rescale
    z[0], z[1] = -1024, 1023
    return z


@pytest.fixture(scope="module")
def block_inputs(oracle):
    """(records, wanted output) for every operation x table pair x (one-hot, dense)."""
    z = np.concatenate([one_hot_blocks(), dense_blocks()])
    recs, want = [], []
    for chroma in (0, 1):
        t = {q: np.asarray(oracle.qtable(q, chroma), np.float32) for q in QUALITIES}
        for a in QUALITIES:
            for b in QUALITIES:
                for op in X.OPS:
                    recs.append(blocks_record(op, t[a], t[b], z))
                    want.append(X.xform_blocks(z, op, t[a], t[b]))
    return b"".join(recs), np.concatenate(want)


@pytest.fixture(scope="module")
def map_inputs():
    recs = b"".join(map_record(op, bw, bh) for op in X.OPS for bw, bh in SHAPES)
    want = np.concatenate([X.block_map(op, bw, bh) for op in X.OPS for bw, bh in SHAPES]).astype(np.uint32)
    return recs, want


def test_pixel_mover_equals_numpy():
    assert X.check_mover()
    # and on an IYUV frame: every plane moved, the planes in order
    w, h = 32, 16
    f = np.arange(w * h * 3 // 2, dtype=np.uint32).astype(np.uint8)
    y = f[:w * h].reshape(h, w)
    got = np.frombuffer(X.move_iyuv(f.tobytes(), w, h, X.NAMES["rot90"]), np.uint8)
    assert np.array_equal(got[:w * h].reshape(w, h), np.rot90(y, -1))
    assert X.out_size(w, h, 5) == (h, w) and X.out_size(w, h, 3) == (w, h)


def test_blocks_equal_numpy(harness, block_inputs):
    recs, want = block_inputs
    got = np.frombuffer(run(harness, recs), np.int16).reshape(-1, 64)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in bad[:4]]
    assert want.min() == -1024 and want.max() == 1023


def test_block_map_equals_numpy(harness, map_inputs):
    recs, want = map_inputs
    got = np.frombuffer(run(harness, recs), np.uint32)
    assert np.array_equal(got, want)
    pos = 0
    for op in X.OPS:
        for bw, bh in SHAPES:  # a bijection of the plane's blocks
            assert sorted(got[pos:pos + bw * bh].tolist()) == list(range(bw * bh)), (op, bw, bh)
            pos += bw * bh


def test_sanitized_build_is_clean_and_identical(harness, sanitized, block_inputs, map_inputs):
    for recs in (block_inputs[0], map_inputs[0]):
        r = subprocess.run([sanitized], input=recs, capture_output=True)
        assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr.decode(errors="replace")[-2000:])
        assert r.stdout == run(harness, recs)


def test_bad_records_are_refused(harness):
    for rec in (struct.pack("<II", 1, 8), struct.pack("<II", 3, 0), struct.pack("<IIII", 2, 0, 0, 4)):
        assert subprocess.run([harness], input=rec, capture_output=True).returncode == 2


# ---- the restatement's own properties ---------------------------------------
def test_negation_clamp_is_reached_only_by_minus_1024(oracle):
    t = np.asarray(oracle.qtable(50, 0), np.float32)
    z = one_hot_blocks()
    out = X.xform_blocks(z, X.NAMES["flip_h"], t, t).reshape(-1, 8, 8)
    src = z.reshape(-1, 8, 8)
    assert np.array_equal(out[:, :, 0::2], src[:, :, 0::2])
    odd_src, odd_out = src[:, :, 1::2], out[:, :, 1::2]
    assert np.array_equal(odd_out[odd_src != -1024], -odd_src[odd_src != -1024])
    assert (odd_out[odd_src == -1024] == 1023).all() and (odd_src == -1024).sum() == 32


@pytest.mark.parametrize("q", [(1, 1, 1), (50, 50, 50), (90, 90, 90), (100, 100, 100), (90, 50, 20)])
def test_mirrors_are_involutions_and_move_the_oracles_pixels(oracle, q):
    """On the tiled chef window: applied twice the source bytes come back, and
    the oracle's decode of the result is the moved decode of the source."""
    pay, raw = R.tiled_stream(AW, AH, q)
    for name in ("flip_h", "flip_v", "rot180"):
        op = X.NAMES[name]
        once = X.cached(pay, AW, AH, q, op, q)
        assert once != pay
        assert X.cached(once, AW, AH, q, op, q) == pay, name
        assert oracle.decompress(once, AW, AH, q) == X.move_iyuv(raw, AW, AH, op), name


@pytest.mark.parametrize("q", [(1, 1, 1), (100, 100, 100)])
def test_swaps_are_exact_where_the_luma_table_is_symmetric(oracle, q):
    t = np.asarray(oracle.qtable(q[0], 0), np.float32).reshape(8, 8)
    assert np.array_equal(t, t.T)
    c = np.asarray(oracle.qtable(50, 1), np.float32).reshape(8, 8)
    assert np.array_equal(c, c.T)  # chroma: at every quality
    pay, raw = R.tiled_stream(AW, AH, q)
    r90 = X.cached(pay, AW, AH, q, X.NAMES["rot90"], q)
    assert X.cached(r90, AH, AW, q, X.NAMES["rot270"], q) == pay
    tr = X.cached(pay, AW, AH, q, X.NAMES["transpose"], q)
    assert X.cached(tr, AH, AW, q, X.NAMES["transpose"], q) == pay
    for name in ("transpose", "rot90", "rot270", "transverse"):
        op = X.NAMES[name]
        out = X.cached(pay, AW, AH, q, op, q)
        assert oracle.decompress(out, AH, AW, q) == X.move_iyuv(raw, AW, AH, op), name


def test_swap_at_an_asymmetric_luma_table_rescales_luma_only(oracle):
    q = (50, 50, 50)
    t = np.asarray(oracle.qtable(50, 0), np.float32).reshape(8, 8)
    assert not np.array_equal(t, t.T)
    pay, _ = R.tiled_stream(AW, AH, q)
    src = S.coefficients(pay)
    out = X.xform_planes(src, AW, AH, X.NAMES["transpose"], q, q)
    for p in (1, 2):  # chroma: the transposed coefficients, exactly
        bw, bh = X.plane_shapes(AW, AH)[p]
        want = src[p].reshape(bh, bw, 8, 8).transpose(1, 0, 3, 2).reshape(-1, 64)
        assert np.array_equal(out[p], want)
    bw, bh = X.plane_shapes(AW, AH)[0]
    assert not np.array_equal(out[0], src[0].reshape(bh, bw, 8, 8).transpose(1, 0, 3, 2).reshape(-1, 64))


def test_op_none_is_requantise(oracle):
    import requantref as Q

    qs, qd = (90, 90, 90), (50, 50, 50)
    pay, _ = R.tiled_stream(AW, AH, qs)
    assert X.cached(pay, AW, AH, qs, 0, qd) == Q.cached(pay, qs, qd)


def test_extreme_streams_reach_the_negation_clamp(oracle):
    import coefgen

    sh = coefgen.shared(oracle)
    s = sh.by_name["extreme_q100"]
    src = S.coefficients(sh.payload(s.name))
    out = X.xform_planes(src, s.w, s.h, X.NAMES["rot180"], s.q, s.q)
    assert any((a == -1024).sum() > (b == -1024).sum() for a, b in zip(src, out))  # some became 1023


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
    assert L.myyuv_gpu_dct_transform(None, u8(pay), 64, 16, 16, u8(qa), 1, u8(qa), u8(out), 64, ctypes.byref(size),
                                     ctypes.byref(bad)) == myyuv_hip.E_ARG
    assert bad.value == -1 and size.value == 9
    assert L.myyuv_gpu_dct_transform_device(None, 256, 512, 64, 1, 16, 16, u8(qa), 1, u8(qa), 1024, 64, 2048,
                                            None) == myyuv_hip.E_ARG
    assert not (out != 0).any()
    assert myyuv_hip.KERNELS.index("coef_xform") == myyuv_hip.K_COEF_XF == 16 and len(myyuv_hip.KERNELS) == 17
    assert myyuv_hip.XF_NAMES == X.NAMES
    assert [myyuv_hip.XF_NONE, myyuv_hip.XF_FLIP_H, myyuv_hip.XF_FLIP_V, myyuv_hip.XF_ROT180, myyuv_hip.XF_TRANSPOSE,
            myyuv_hip.XF_ROT90, myyuv_hip.XF_ROT270, myyuv_hip.XF_TRANSVERSE] == list(range(8))
    assert [myyuv_hip.xf_swaps(op) for op in range(8)] == [False] * 4 + [True] * 4


def test_header_names_the_operations():
    import re

    src = open(os.path.join(ROOT, "include", "myyuv_hip.h")).read()
    ids = {m.group(1).lower(): int(m.group(2))
           for m in re.finditer(r"^#define MYYUV_XF_([A-Z0-9_]+)\s+(\d+)", src, re.M)}
    assert ids == X.NAMES
    assert re.search(r"^#define MYYUV_XF_SWAPS\(op\) \(\(op\) & 4\)", src, re.M)


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def test_cli_transform_argument_errors(tmp_path):
    out = str(tmp_path / "x.myyuv")
    # an uncompressed input has no coefficients
    r = cli(RAW, "-transform", "rot90", "-o", out)
    assert r.returncode == 1, r.stdout
    assert r.stdout.splitlines()[0] == \
        "Nothing to transform, image is not compressed (-transform needs DCT coefficients)"
    # the operation
    for tail in ([], ["rot45", "-o", out], ["none", "-o", out], ["-o", out]):
        r = cli(C50, "-transform", *tail)
        assert r.returncode == 1 and "Usage" in r.stdout, (tail, r.stdout)
        assert r.stdout.splitlines()[0] == \
            "Invalid argument, -transform takes flip_h, flip_v, rot180, transpose, transverse, rot90 or rot270"
    # no output file, or qualities without -q
    for tail in ([], ["-o"], ["-o", out, "extra"], ["50", "-o", out], ["-q", "50"], ["-q", "50", "-o"]):
        r = cli(C50, "-transform", "flip_h", *tail)
        assert r.returncode == 1 and "Usage" in r.stdout, (tail, r.stdout)
        assert r.stdout.splitlines()[0] == "Invalid argument, last arguments must be `-o /path/to/new_image.myyuv`"
    # the qualities, parsed as -compress DCT's (the exception propagates, as in the reference CLI)
    for params, msg in ((["0"], "must range between [1..100]"), (["101"], "must range between [1..100]"),
                        (["50", "50", "50", "50"], "Too many compression parameters"),
                        ([], "Too few compression parameters")):
        r = cli(C50, "-transform", "rot180", "-q", *params, "-o", out)
        assert r.returncode != 0 and msg in r.stderr, (params, r.returncode, r.stderr)
    assert not os.path.exists(out)
    assert ("-transform flip_h|flip_v|rot180|transpose|transverse|rot90|rot270 [-q Q [Q [Q]]] -o OUT.myyuv"
            in cli(C50, "-transform").stdout)

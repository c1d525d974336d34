"""Compare, the parts that need no GPU: the block arithmetic of csrc/metric.h
(the code k_decode_compare and k_frame_compare run) compiled for the host
(tools/metric_host.cpp) against the exact-integer restatement (metricref) of
the definition in include/myyuv_hip.h; the same program under ASan + UBSan; the
64-bit claim of the definition; a hand-written 16x16 pair with its expected
integers; the two host conversions; the argument errors of the C ABI and the
CLI's -compare argument errors and refusals."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import metricref as M
from conftest import GOLDEN, PKG, ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "tools", "metric_host.cpp")
INC = ["-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include")]
CLI = os.path.join(PKG, "myyuv_cli")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
OUT = np.dtype([("sse", "<u4"), ("max", "<u4"), ("ssim", "<i4"), ("zero", "<u4"), ("num", "<i8"), ("den", "<u8")])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("metric") / "metric_host")
    subprocess.run([HIPCC, "-O2", "-std=c++17", *INC, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same program with AddressSanitizer + UndefinedBehaviorSanitizer on
    the host (the flags of tests/test_scaled_host.py harness_san); a stand-alone
    binary, never loaded into Python."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("metricsan") / "metric_host_san")
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-fno-gpu-sanitize"]
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17"] + san +
                   ["-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *INC, SRC, "-o", exe], check=True)
    return exe


def run_blocks(exe, x, y, env=None):
    x = np.ascontiguousarray(x, np.uint8).reshape(-1, 64)
    y = np.ascontiguousarray(y, np.uint8).reshape(-1, 64)
    assert x.shape == y.shape
    r = subprocess.run([exe], input=struct.pack("<II", 0, len(x)) + x.tobytes() + y.tobytes(), capture_output=True,
                       env=env)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return np.frombuffer(r.stdout, OUT), r.stderr


def run_sums(exe, s, env=None):
    s = np.ascontiguousarray(s, "<u4").reshape(-1, 5)
    r = subprocess.run([exe], input=struct.pack("<II", 1, len(s)) + s.tobytes(), capture_output=True, env=env)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return np.frombuffer(r.stdout, OUT), r.stderr


def quotient_steps(num, den):
    """The device's quotient (metric.h ssim_quotient) on Python ints: one
    compare-subtract for the integer part, 24 shift-subtract steps, the floor
    of a negative quotient.  Returns (quotient, the widest intermediate)."""
    neg, r, q = num < 0, abs(num), 0
    if r >= den:
        r, q = r - den, 1
    widest = r
    for _ in range(24):
        r, q = r << 1, q << 1
        widest = max(widest, r)
        if r >= den:
            r, q = r - den, q | 1
    return (-q - (1 if r else 0)) if neg else q, widest


def ones_block(k, shift=0):
    """k samples of 255 (from position `shift`, wrapping), the rest 0."""
    b = np.zeros(64, np.uint8)
    b[(np.arange(k) + shift) % 64] = 255
    return b


def stripe():
    return np.tile(np.array([0, 255], np.uint8), 32)


@pytest.fixture(scope="module")
def inputs():
    """{name: (x, y)}: uint8 blocks [n, 64]."""
    rng = np.random.default_rng(2424)
    noise = rng.integers(0, 256, (512, 64), dtype=np.uint8)
    other = rng.integers(0, 256, (512, 64), dtype=np.uint8)
    near = np.clip(noise.astype(np.int16) + rng.integers(-3, 4, noise.shape), 0, 255).astype(np.uint8)
    flat = np.repeat(np.arange(256, dtype=np.uint8), 64).reshape(256, 64)
    st = np.stack([stripe(), 255 - stripe(), np.repeat(np.array([0, 255], np.uint8), 32)])
    # the largest denominators: k samples of 255 on both sides, B1 B2 ~ k^3 (64 - k), largest at k = 48;
    # every overlap of the two patterns, so the numerators and remainders vary
    heavy_x = np.stack([ones_block(k) for k in range(40, 57) for _ in range(64)])
    heavy_y = np.stack([ones_block(k, s) for k in range(40, 57) for s in range(64)])
    return {"random": (noise, other), "near": (noise, near), "identical": (noise, noise),
            "inverse_noise": (noise, 255 - noise), "inverse_stripe": (st, 255 - st),
            "black_white": (np.zeros((1, 64), np.uint8), np.full((1, 64), 255, np.uint8)),
            "flat_one_apart": (flat[:-1], flat[1:]), "heavy": (heavy_x, heavy_y)}


def check(got, x, y):
    sse, mx, sx, sy, sxx, syy, sxy = M.sums(x, y)
    assert (got["sse"] == sse).all() and (got["max"] == mx).all()
    assert (got["zero"] == 0).all()
    widest_den = widest_rem = 0
    for k, t in enumerate(zip(sx, sy, sxx, syy, sxy)):
        a1, a2, b1, b2 = M.terms(*t)
        num, den = a1 * a2, b1 * b2
        assert int(got["num"][k]) == num and int(got["den"][k]) == den, k  # no 64-bit wrap on the way
        want = M.ssim_of_sums(*t)
        q, widest = quotient_steps(num, den)
        assert q == want and -M.ONE <= want <= M.ONE
        assert int(got["ssim"][k]) == want, (k, int(got["ssim"][k]), want)
        widest_den, widest_rem = max(widest_den, den), max(widest_rem, widest)
    return widest_den, widest_rem


def test_host_equals_metricref(harness, inputs):
    seen_negative = False
    for name, (x, y) in inputs.items():
        got, _ = run_blocks(harness, x, y)
        den, rem = check(got, x, y)
        assert den.bit_length() <= 56 and rem.bit_length() <= 57, name  # the definition's 64-bit claim
        if name == "identical":
            assert (got["ssim"] == M.ONE).all() and (got["sse"] == 0).all() and (got["max"] == 0).all()
        if name.startswith("inverse"):
            assert (got["ssim"] < 0).all(), name
            seen_negative = True
        if name == "black_white":
            assert got["sse"][0] == 64 * 255 * 255 and got["max"][0] == 255 and got["ssim"][0] == 1677
        if name == "flat_one_apart":
            assert (got["sse"] == 64).all() and (got["max"] == 1).all() and (got["ssim"] > 0).all()
        if name == "heavy":
            # 2 * 255^2 * 48^2 * 2 * 255^2 * 48 * 16 (+ the constants): 55 bits, as large as B1 B2 gets
            assert den.bit_length() == 55 and rem.bit_length() in (55, 56)
            k = 8 * 64  # k = 48, shift 0
            assert int(got["den"][k]) == (2 * 65025 * 48 * 48 + M.C1) * (2 * 65025 * 48 * 16 + M.C2)
    assert seen_negative


def test_floor_is_towards_minus_infinity(harness, inputs):
    """A negative quotient that is not exact goes one further down; the exact
    ones (and only those) do not."""
    x, y = inputs["inverse_noise"]
    got, _ = run_blocks(harness, x, y)
    inexact = 0
    for k in range(len(got)):
        num, den = int(got["num"][k]), int(got["den"][k])
        assert num < 0
        trunc = -((-num << 24) // den)
        exact = (-num << 24) % den == 0
        assert int(got["ssim"][k]) == (trunc if exact else trunc - 1)
        inexact += not exact
    assert inexact > 0
    # the same arithmetic from sums given directly: the stripe against its inverse
    got, _ = run_sums(harness, [[8160, 8160, 2080800, 2080800, 0]])
    a1, a2, b1, b2 = M.terms(8160, 8160, 2080800, 2080800, 0)
    assert int(got["ssim"][0]) == ((a1 * a2) << 24) // (b1 * b2) == -16716927


def test_sanitized_host_build_is_clean(harness, harness_san, inputs):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for name, (x, y) in inputs.items():
        want, _ = run_blocks(harness, x, y)
        got, err = run_blocks(harness_san, x, y, env=env)
        assert b"runtime error" not in err and b"AddressSanitizer" not in err, name
        assert got.tobytes() == want.tobytes(), name
    s = [[16320, 16320, 4161600, 4161600, 4161600], [0, 0, 0, 0, 0], [16320, 0, 4161600, 0, 0]]
    want, _ = run_sums(harness, s)
    got, err = run_sums(harness_san, s, env=env)
    assert b"runtime error" not in err and b"AddressSanitizer" not in err
    assert got.tobytes() == want.tobytes() and want["ssim"].tolist() == [M.ONE, M.ONE, 1677]


# A 16x16 pair, reference x against test y (Y: four blocks, U and V one each).
#   Y0  x = y = 100 everywhere: sse 0, max 0, ssim 2^24 = 16777216
#   Y1  x = 0, y = 255: sse 64 * 255^2 = 4161600, max 255; Sx = Sxx = Sxy = 0, Sy = 16320, Syy = 4161600:
#       A1 = C1, A2 = C2, B1 = 16320^2 + C1 = 266369034, B2 = 64 * 4161600 - 16320^2 + C2 = C2:
#       ssim = floor(26634 * 2^24 / 266369034) = floor(446844370944 / 266369034) = 1677
#   Y2  x = 100, y = 101: sse 64, max 1; Sx = 6400, Sy = 6464, Sxy = 646400, Sxx = 640000, Syy = 652864:
#       64 Sxy = Sx Sy and 64 (Sxx + Syy) = Sx^2 + Sy^2 (flat blocks), so A2 = B2 = C2,
#       A1 = 2 * 6400 * 6464 + C1 = 82765834, B1 = 6400^2 + 6464^2 + C1 = 82769930:
#       ssim = floor(82765834 * 2^24 / 82769930) = 16776385
#   Y3  x = columns 0, 255, 0, 255 ..., y = 255 - x: sse 4161600, max 255; Sx = Sy = 8160, Sxx = Syy = 2080800,
#       Sxy = 0: A1 = B1 = 2 * 8160^2 + C1, A2 = -2 * 8160^2 + C2 = -132931492,
#       B2 = 128 * 2080800 - 2 * 8160^2 + C2 = 133410908:
#       ssim = floor(-132931492 * 2^24 / 133410908) = -16716927 (16716926 and a remainder, one further down)
#   U   x = y = 0 .. 63: sse 0, max 0, ssim 2^24
#   V   x = 0 .. 63, y = x + 1: sse 64, max 1; Sx = 2016, Sy = 2080, Sxx = 85344, Syy = 89440, Sxy = 87360:
#       A1 = 8413194, A2 = 2 (5591040 - 4193280) + C2 = 3035228, B1 = 8417290,
#       B2 = 64 * 174784 - 4064256 - 4326400 + C2 = 3035228: ssim = floor(8413194 * 2^24 / 8417290) = 16769051
HAND_RECORDS = ((0 + 4161600 + 64 + 4161600, 16777216 + 1677 + 16776385 - 16716927, 4, 255),
                (0, 16777216, 1, 0), (64, 16769051, 1, 1))
HAND_MAP = [(0, 16777216), (4161600, 1677), (64, 16776385), (4161600, -16716927), (0, 16777216), (64, 16769051)]


def hand_pair():
    def frame(yb, u, v):
        y = np.zeros((16, 16), np.uint8)
        for k, b in enumerate(yb):
            y[8 * (k // 2):8 * (k // 2) + 8, 8 * (k % 2):8 * (k % 2) + 8] = np.asarray(b, np.uint8).reshape(8, 8)
        return y.tobytes() + np.asarray(u, np.uint8).tobytes() + np.asarray(v, np.uint8).tobytes()

    ramp = np.arange(64)
    x = frame([np.full(64, 100), np.zeros(64), np.full(64, 100), stripe()], ramp, ramp)
    y = frame([np.full(64, 100), np.full(64, 255), np.full(64, 101), 255 - stripe()], ramp, ramp + 1)
    return x, y


def test_hand_written_pair():
    x, y = hand_pair()
    recs, bmap = M.frame_metric(x, y, 16, 16)
    assert recs == HAND_RECORDS
    assert [(int(s), int(q)) for s, q in zip(bmap["sse"], bmap["ssim"])] == HAND_MAP
    assert M.frame_metric(y, x, 16, 16)[0] == HAND_RECORDS  # symmetric


def test_hand_written_pair_on_the_host_program(harness):
    x, y = hand_pair()
    bx = np.concatenate([M.plane_blocks(p) for p in M.planes(x, 16, 16)])
    by = np.concatenate([M.plane_blocks(p) for p in M.planes(y, 16, 16)])
    got, _ = run_blocks(harness, bx, by)
    assert [(int(s), int(q)) for s, q in zip(got["sse"], got["ssim"])] == HAND_MAP
    assert got["max"].tolist() == [0, 255, 1, 255, 0, 1]


def test_psnr_and_ssim_conversions():
    import myyuv_hip

    for sse, n in ((1, 1), (64, 64), (4161600, 64), (12345678, 992 * 736), (35 * 10 ** 9, 532480), (2 ** 40, 2 ** 33)):
        want = 10.0 * math.log10(255.0 ** 2 * n / sse)
        assert myyuv_hip.metric_psnr(sse, n) == pytest.approx(want, rel=1e-12, abs=1e-12), (sse, n)
        assert M.psnr(sse, n) == pytest.approx(want, rel=1e-12, abs=1e-12)
    assert myyuv_hip.metric_psnr(0, 64) == math.inf and M.psnr(0, 64) == math.inf
    for ss, nb in ((16777216, 1), (-16716927, 1), (3 * 16777216 - 5, 3), (-(2 ** 40), 2 ** 20), (0, 7)):
        assert myyuv_hip.metric_ssim(ss, nb) == pytest.approx(ss / (nb * 2.0 ** 24), rel=1e-12, abs=0.0)
        assert M.ssim(ss, nb) == pytest.approx(ss / (nb * 2.0 ** 24), rel=1e-12, abs=0.0)
    assert myyuv_hip.metric_ssim(5 * 16777216, 5) == 1.0


def test_argument_errors_need_no_device():
    """MYYUV_E_ARG for a null handle or pointer, or ref_frames not in {1,
    nframes}: *bad_block = -1 and a zeroed record, before anything touches a
    device."""
    import myyuv_hip

    L = myyuv_hip.load()
    pay = np.zeros(64, np.uint8)
    ref = np.zeros(16 * 16 * 3 // 2, np.uint8)
    qa = np.array([50, 50, 50], np.uint8)
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731

    def dirty():
        m = myyuv_hip.FrameMetric()
        ctypes.memset(ctypes.byref(m), 0x5A, ctypes.sizeof(m))
        return m

    assert ctypes.sizeof(myyuv_hip.FrameMetric) == 72 and myyuv_hip.BLOCK_METRIC.itemsize == 8
    m, bad = dirty(), ctypes.c_int64(7)
    assert L.myyuv_gpu_dct_compare(None, u8(pay), 64, 16, 16, u8(qa), u8(ref), ctypes.byref(m), None,
                                   ctypes.byref(bad)) == myyuv_hip.E_ARG
    assert bad.value == -1 and m.as_ints() == ((0, 0, 0, 0),) * 3
    m, bad = dirty(), ctypes.c_int64(7)
    assert L.myyuv_gpu_dct_compare(None, u8(pay), 64, 16, 16, u8(qa), None, ctypes.byref(m), None,
                                   ctypes.byref(bad)) == myyuv_hip.E_ARG
    assert bad.value == -1 and m.as_ints() == ((0, 0, 0, 0),) * 3
    m = dirty()
    assert L.myyuv_gpu_iyuv_compare(None, u8(ref), u8(ref), 16, 16, ctypes.byref(m), None) == myyuv_hip.E_ARG
    assert m.as_ints() == ((0, 0, 0, 0),) * 3
    # the device forms: a null handle; then, with a handle that is never used, ref_frames and null pointers
    assert L.myyuv_gpu_iyuv_compare_device(None, 256, 512, 1, 1, 16, 16, 1024, None, None) == myyuv_hip.E_ARG
    assert L.myyuv_gpu_dct_compare_device(None, 256, 512, 64, 1, 16, 16, u8(qa), 1024, 1, 2048, None,
                                          None) == myyuv_hip.E_ARG
    fake = ctypes.c_void_p(8)  # (not dereferenced: the argument checks come first)
    for nframes, ref_frames in ((3, 2), (3, 0), (2, 3), (1, 0), (0, 0)):
        assert L.myyuv_gpu_iyuv_compare_device(fake, 256, 512, nframes, ref_frames, 16, 16, 1024, None,
                                               None) == myyuv_hip.E_ARG, (nframes, ref_frames)
    for nframes, ref_frames in ((3, 2), (3, 0), (2, 3), (1, 0)):
        assert L.myyuv_gpu_dct_compare_device(fake, 256, 512, 64, nframes, 16, 16, u8(qa), 1024, ref_frames, 2048,
                                              None, None) == myyuv_hip.E_ARG, (nframes, ref_frames)
    assert L.myyuv_gpu_iyuv_compare_device(fake, None, 512, 1, 1, 16, 16, 1024, None, None) == myyuv_hip.E_ARG
    assert L.myyuv_gpu_iyuv_compare_device(fake, 256, 512, 1, 1, 16, 16, None, None, None) == myyuv_hip.E_ARG
    assert L.myyuv_gpu_dct_compare_device(fake, 256, 512, 64, 1, 16, 16, u8(qa), None, 1, 2048, None,
                                          None) == myyuv_hip.E_ARG
    assert L.myyuv_gpu_dct_compare_device(fake, 256, 512, 64, 1, 16, 16, u8(qa), 1028, 1, 2048, None,
                                          None) == myyuv_hip.E_ARG  # d_ref not 8-byte aligned
    for name in ("myyuv_gpu_iyuv_compare", "myyuv_gpu_iyuv_compare_device", "myyuv_gpu_dct_compare",
                 "myyuv_gpu_dct_compare_device", "myyuv_metric_psnr", "myyuv_metric_ssim"):
        assert name in myyuv_hip.EXPORTS and getattr(L, name)
    # the new kernel ids follow the frozen bounds
    assert myyuv_hip.KERNELS_ALL[myyuv_hip.K_COMPARE] == "decode_compare" and myyuv_hip.K_COMPARE == 18
    assert myyuv_hip.KERNELS_ALL[myyuv_hip.K_FRAME_CMP] == "frame_compare" and myyuv_hip.K_FRAME_CMP == 19
    assert myyuv_hip.KERNELS_ALL[myyuv_hip.K_METRIC_SUM] == "metric_reduce" and myyuv_hip.K_METRIC_SUM == 20
    assert myyuv_hip.K_END == 21 == len(myyuv_hip.KERNELS_ALL)


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def test_cli_compare_argument_errors(tmp_path):
    """A malformed -compare: one fixed first line, the usage, exit 1, no file;
    before the other image is read (no GPU is touched)."""
    out = str(tmp_path / "report.txt")
    first = "Invalid argument, -compare must be followed by an image and at most `-o /path/to/report.txt`"
    for src in (RAW, C50):
        for tail in ([], [C50, "-o"], [C50, out], [C50, "-o", out, "x"], [C50, "-x", out], [C50, C50, "-o", out]):
            r = cli(src, "-compare", *tail)
            assert r.returncode == 1 and "Usage" in r.stdout, (tail, r.stdout)
            assert r.stdout.splitlines()[0] == first, (tail, r.stdout)
            assert not os.path.exists(out)
    assert "-compare OTHER.myyuv [-o REPORT.txt]" in cli(RAW, "-compare").stdout


def test_cli_compare_refusals(tmp_path, golden):
    import myyuv_file

    out = str(tmp_path / "report.txt")
    f = golden("chef-with-trumpet.myyuv")
    small = tmp_path / "small.myyuv"
    small.write_bytes(myyuv_file.YUVFile(f.fourcc, 16, 16, myyuv_file.NONE, b"", bytes(384), f.unused).dumps())
    for src in (RAW, C50):
        for a, b in ((src, str(small)), (str(small), src)):
            r = cli(a, "-compare", b, "-o", out)
            assert r.returncode == 1, r.stdout
            assert r.stdout.splitlines()[0] == "Nothing to compare, the images differ in size or format"
            assert not os.path.exists(out)
        r = cli(src, "-compare", str(tmp_path / "missing.myyuv"), "-o", out)
        assert r.returncode == 1 and r.stdout.startswith("Error comparing: "), r.stdout
        assert not os.path.exists(out)

"""Scaled decode, the parts that need no GPU: the block arithmetic of
csrc/idct_scaled.h (the code k_decode_scaled runs) compiled for the host
(tools/idct_scaled_host.cpp, -ffp-contract=off) against the numpy restatement
(scaleref) of the definition in include/myyuv_hip.h; the same program under
ASan + UBSan; the header's N = 1 claim against the oracle's full decode; a
hand-written stream with its expected bytes; the CLI's -scale argument errors
and refusals."""
import os
import struct
import subprocess

import numpy as np
import pytest

import coefgen
import scaleref as S
from conftest import GOLDEN, PKG, ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "tools", "idct_scaled_host.cpp")
INC = ["-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include")]
CLI = os.path.join(PKG, "myyuv_cli")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
NS = (1, 2, 4)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("scaled") / "idct_scaled_host")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", *INC, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same program with AddressSanitizer + UndefinedBehaviorSanitizer on
    the host (the flags of tests/test_r8_host.py harness_san); a stand-alone
    binary, never loaded into Python."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("scaledsan") / "idct_scaled_host_san")
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-fno-gpu-sanitize"]
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + san +
                   ["-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *INC, SRC, "-o", exe], check=True)
    return exe


def payload_for(N, Q, nat):
    nat = np.ascontiguousarray(nat, np.int16).reshape(-1, 64)
    return struct.pack("<II", N, len(nat)) + np.ascontiguousarray(Q, np.float32).tobytes() + nat.tobytes()


def run(exe, N, Q, nat, env=None):
    r = subprocess.run([exe], input=payload_for(N, Q, nat), capture_output=True, env=env)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    n = len(np.asarray(nat).reshape(-1, 64))
    assert len(r.stdout) == n * N * N
    return np.frombuffer(r.stdout, np.uint8).reshape(n, N, N), r.stderr


@pytest.fixture(scope="module")
def qtables(oracle):
    return {"q50_luma": oracle.qtable(50, 0), "q90_luma": oracle.qtable(90, 0), "q100_luma": oracle.qtable(100, 0),
            "q50_chroma": oracle.qtable(50, 1), "ones": np.ones(64, np.float32), "q255": np.full(64, 255, np.float32)}


@pytest.fixture(scope="module")
def inputs(qtables):
    """{name: natural-order blocks [n, 64]}, the same for every Q table and N."""
    rng = np.random.default_rng(1414)
    ext = coefgen.extreme_blocks(64, rng)
    assert set(np.unique(ext)) <= {1023, -1024}
    return {"one_coefficient": coefgen.natural(coefgen.one_coefficient_blocks()),
            "extreme": coefgen.natural(ext),
            "extreme_pm1023": np.where(coefgen.natural(ext) > 0, 1023, -1023).astype(np.int16),
            "in_range": coefgen.natural(np.concatenate([coefgen.in_range_blocks(128, Q, rng)
                                                        for Q in qtables.values()])),
            "dc_sweep": coefgen.natural(coefgen.dc_blocks())}


def test_basis_literals_are_the_formula():
    for N in NS:
        assert S.BASIS[N].dtype == np.float32
        assert (S.BASIS[N] == S.basis_from_formula(N)).all(), N
    assert float(S.C_) == 0.3535533845424652


def test_round_half_away():
    x = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999997, -0.49999997, 126.5, -128.5, 0.0], np.float32)
    assert S.round_half_away(x).tolist() == [1, -1, 2, -2, 3, -3, 0, 0, 127, -129, 0]


@pytest.mark.parametrize("N", NS)
def test_host_equals_scaleref(harness, qtables, inputs, N):
    ties = 0
    for qn, Q in qtables.items():
        for name, nat in inputs.items():
            got, _ = run(harness, N, Q, nat)
            want = S.scaled_blocks(nat, Q, N)
            assert (got == want).all(), (qn, name, np.argwhere(got != want)[:4])
            if name == "one_coefficient":
                # the coefficient of block k is at zig-zag position k // 12: outside
                # the N x N corner the block is flat 128
                z = coefgen.ZZ[np.arange(len(nat)) // 12]
                outside = (z // 8 >= N) | (z % 8 >= N)
                assert outside.sum() == 12 * (64 - N * N)
                assert (got[outside] == 128).all()
                assert (got[~outside] != 128).any()
            if name.startswith("extreme") and qn == "q255":  # the clamp, both ends
                assert got.min() == 0 and got.max() == 255
            if name == "dc_sweep":  # the .5 ties: R = z Q / 8 exactly when it is representable
                r = nat[:, 0].astype(np.float64) * float(Q[0]) / 8.0
                ties += int(np.count_nonzero(np.abs(r - np.trunc(r)) == 0.5))
    assert ties > 1000


def test_sanitized_host_build_is_clean(harness, harness_san, qtables, inputs):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for N in NS:
        for qn, Q in qtables.items():
            for name, nat in inputs.items():
                want, _ = run(harness, N, Q, nat)
                got, err = run(harness_san, N, Q, nat, env=env)
                assert b"runtime error" not in err and b"AddressSanitizer" not in err, (N, qn, name)
                assert (got == want).all(), (N, qn, name)


@pytest.mark.parametrize("name", [f"dc_sweep_luma_q{q}" for q in (1, 25, 50, 88, 100)] +
                         ["dc_sweep_chroma_q50", "dc_sweep_chroma_q100"])
def test_eighth_of_dc_only_frame_is_the_full_decodes_pixel(oracle, name):
    """include/myyuv_hip.h: "A frame whose blocks are all DC-only therefore has
    a 1/8 decode equal to any one pixel of each block of its full decode."""
    sh = coefgen.shared(oracle)
    s = sh.by_name[name]
    pay, full = sh.decoded(name)
    got = S.decode_scaled(pay, s.w, s.h, s.q, 8)
    a = np.frombuffer(full, np.uint8)
    want, off = [], 0
    for p in range(3):
        pw, ph = (s.w, s.h) if p == 0 else (s.w // 2, s.h // 2)
        plane = a[off:off + pw * ph].reshape(ph, pw)
        assert (plane.reshape(ph // 8, 8, pw // 8, 8) == plane[::8, ::8][:, None, :, None]).all()  # flat blocks
        want.append(plane[::8, ::8].tobytes())
        off += pw * ph
    assert got == b"".join(want)


# A 16x16 frame at q50 (luma Q[0][0] = 16, Q[0][1] = 11, Q[1][0] = 12; chroma
# Q[0][0] = 17): zig-zag blocks, Y row-major then U, V.
#   Y0  DC 10:            every scale 128 + 10 * 16 / 8 = 148
#   Y1  DC -20:           128 - 40 = 88
#   Y2  DC 4, z[0][1] 8:  1/8 sees the DC only: 136; 1/4 and 1/2 a horizontal ramp
#   Y3  z[7][7] = 1023:   outside every corner: 128
#   U   DC 100:           128 + 100 * 17 / 8 = 340.5 -> 341, clamped to 255
#   V   DC -3, z[1][0] -5: 1/8: roundf(-6.375) = -6 -> 122; a vertical ramp
HAND = ([[10] + [0] * 63, [-20] + [0] * 63, [4, 8] + [0] * 62, [0] * 63 + [1023]],
        [[100] + [0] * 63], [[-3, 0, -5] + [0] * 61])
#   Y2 at 1/4: c c 64 +- c c 88 = 8 +- 11 -> 147, 125; at 1/2: 8 + c 88 {s, t, -t, -s} = 8 + {14.37, 5.95,
#   -5.95, -14.37} -> 150, 142, 130, 122.  V at 1/4 (chroma Q[1][0] = 18): -6.375 -+ 11.25 -> 110, 133; at
#   1/2: -6.375 - c 90 {s, t, -t, -s} -> 107, 116, 128, 136.
HAND_WANT = {
    8: [148, 88, 136, 128] + [255] + [122],
    4: [148, 148, 88, 88] * 2 + [147, 125, 128, 128] * 2 + [255] * 4 + [110, 110, 133, 133],
    2: [148, 148, 148, 148, 88, 88, 88, 88] * 4 + [150, 142, 130, 122, 128, 128, 128, 128] * 4 + [255] * 16 +
       [107] * 4 + [116] * 4 + [128] * 4 + [136] * 4,
}


def test_hand_written_stream(oracle):
    q = (50, 50, 50)
    pay = coefgen.build_payload(HAND, oracle)
    assert coefgen.compose(HAND, 16, 16, q, oracle) == oracle.decompress(pay, 16, 16, q)
    for denom, want in HAND_WANT.items():
        got = S.decode_scaled(pay, 16, 16, q, denom)
        assert got == bytes(want), (denom, list(got))


def test_handle_and_pointer_errors_need_no_device():
    """MYYUV_E_ARG for a null handle or pointer, *bad_block = -1, before
    anything touches a device."""
    import ctypes

    import myyuv_hip

    L = myyuv_hip.load()
    pay = np.zeros(64, np.uint8)
    out = np.zeros(64, np.uint8)
    qa = np.array([50, 50, 50], np.uint8)
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    bad = ctypes.c_int64(7)
    assert L.myyuv_gpu_dct_decompress_scaled(None, u8(pay), 64, 16, 16, u8(qa), 2, u8(out), ctypes.byref(bad)) == 1
    assert bad.value == -1
    bad = ctypes.c_int64(7)
    assert L.myyuv_gpu_dct_decompress_scaled_to_bmp(None, u8(pay), 64, 16, -16, u8(qa), 2, 32, 1, u8(out),
                                                    ctypes.byref(bad)) == 1
    assert bad.value == -1
    assert L.myyuv_gpu_dct_decompress_scaled_device(None, 256, 512, 64, 1, 16, 16, u8(qa), 2, 1024, None) == 1
    assert not (out != 0).any()


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def test_cli_scale_argument_errors(tmp_path):
    """A malformed -scale: one fixed first line, the usage, exit 1, no file;
    before the file's content matters (no GPU is touched)."""
    out = str(tmp_path / "x.out")
    first = "Invalid argument, -scale must be followed by `1/2`, `1/4` or `1/8`"
    bad = (["-scale"], ["-scale", "2"], ["-scale", "1/3"], ["-scale", "1/16"], ["-scale", "1/1"], ["-scale", "0.5"],
           ["-scale", "1/2x"], ["-scale", "-o"], ["-scale", ""])
    for src in (RAW, C50):
        for head in (["-decompress"], ["-to_bmp"], ["-to_bmp", "24", "-chroma", "nearest"]):
            for b in bad:
                args = [src, *head, *b] + ([] if b[-1] == "-o" else ["-o"]) + [out]
                r = cli(*args)
                assert r.returncode == 1 and "Usage" in r.stdout, (args, r.stdout)
                assert r.stdout.splitlines()[0] == first, (args, r.stdout)
                assert not os.path.exists(out)
    # the usage names the two forms
    r = cli(C50, "-decompress", "-scale", "1/3", "-o", out)
    assert "-decompress -scale 1/2|1/4|1/8 -o OUT.myyuv" in r.stdout
    assert "-to_bmp [24|32] [-chroma nearest|linear] -scale 1/2|1/4|1/8 -o OUT.bmp" in r.stdout


def test_cli_scale_refusals(tmp_path):
    out = str(tmp_path / "x.out")
    # an uncompressed input has no coefficients to scale from
    for head in (["-decompress"], ["-to_bmp"], ["-to_bmp", "24"]):
        r = cli(RAW, *head, "-scale", "1/2", "-o", out)
        assert r.returncode == 1, r.stdout
        assert r.stdout.splitlines()[0] == "Nothing to scale, image is not compressed (-scale needs DCT coefficients)"
        assert not os.path.exists(out)
    # -scale and -crop together, in either order
    crop = ["-crop", "0", "0", "16", "16"]
    for src in (RAW, C50):
        for head in (["-decompress"], ["-to_bmp"], ["-to_bmp", "32", "-chroma", "linear"]):
            for opts in (crop + ["-scale", "1/4"], ["-scale", "1/4"] + crop):
                r = cli(src, *head, *opts, "-o", out)
                assert r.returncode == 1 and "Usage" in r.stdout, (src, head, opts, r.stdout)
                assert r.stdout.splitlines()[0] == "Invalid arguments, -scale and -crop cannot be combined"
                assert not os.path.exists(out)

"""Downscale, the parts that need no GPU: the work map of csrc/downscale.h (the
code k_downscale runs) compiled for the host (tools/downscale_host.cpp) against
its numpy restatement (downscaleref.work_map), for every (geometry, denom) pair
of tests/test_gpu_downscale.py; every source block lands exactly once and every
output pixel is covered exactly once; the same program under ASan + UBSan; the
C ABI's pointer checks and the bindings' lists; the CLI's -downscale argument
errors and refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import downscaleref as D
from conftest import GOLDEN, PKG, ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "tools", "downscale_host.cpp")
INC = ["-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include")]
CLI = os.path.join(PKG, "myyuv_cli")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")

# (w, h, denom) of tests/test_gpu_downscale.py and tests/test_cli_downscale.py
GEOMETRIES = [(128, 128, 2), (128, 128, 4), (128, 128, 8), (416, 192, 2), (832, 384, 4), (1664, 768, 8),
              (2080, 64, 2), (2112, 64, 4), (2176, 128, 8), (1056, 512, 2), (416, 96, 2), (256, 128, 4),
              (960, 704, 2), (960, 704, 4)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("downscale") / "downscale_host")
    subprocess.run([HIPCC, "-O2", "-std=c++17", *INC, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same program with AddressSanitizer + UndefinedBehaviorSanitizer on
    the host (the flags of tests/test_scaled_host.py harness_san); a
    stand-alone binary, never loaded into Python."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("downscalesan") / "downscale_host_san")
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-fno-gpu-sanitize"]
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17"] + san +
                   ["-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *INC, SRC, "-o", exe], check=True)
    return exe


def run(exe, w, h, denom, env=None):
    r = subprocess.run([exe, str(w), str(h), str(denom)], capture_output=True, env=env)
    assert r.returncode == 0, (w, h, denom, r.returncode, r.stderr.decode(errors="replace")[-2000:])
    assert len(r.stdout) % 32 == 0
    return np.frombuffer(r.stdout, np.uint32).reshape(-1, 8), r.stderr


@pytest.mark.parametrize("w,h,denom", GEOMETRIES)
def test_host_map_equals_numpy_map(harness, w, h, denom):
    got, _ = run(harness, w, h, denom)
    want = D.work_map(w, h, denom)
    assert got.shape == want.shape
    assert (got == want).all(), np.argwhere(got != want)[:4]


@pytest.mark.parametrize("w,h,denom", GEOMETRIES)
def test_every_block_once_and_every_pixel_once(harness, w, h, denom):
    """From the host program's records alone: each source block of each plane
    appears once; the N x N cells, placed by the records' image bytes inside
    their output blocks, tile every output plane exactly."""
    got = run(harness, w, h, denom)[0].astype(np.int64)
    N = 8 // denom
    for p, (sbw, sbh, dbw, dbh) in enumerate(D.plane_blocks(w, h, denom)):
        m = got[got[:, 1] == p]
        assert len(m) == sbw * sbh
        assert (np.sort(m[:, 4]) == np.arange(sbw * sbh)).all()  # every source block, once
        assert m[:, 5].max() == dbw * dbh - 1
        cover = np.zeros((dbh * 8, dbw * 8), np.int32)
        off = m[:, 7] - 64 * m[:, 6]  # the first pixel inside its block's 8 x 8-byte image
        assert ((off >= 0) & (off < 64)).all()
        y0 = (m[:, 5] // dbw) * 8 + off // 8
        x0 = (m[:, 5] % dbw) * 8 + off % 8
        for i in range(N):
            for j in range(N):
                np.add.at(cover, (y0 + i, x0 + j), 1)
        assert (cover == 1).all(), (p, int((cover != 1).sum()))
        # a wave's lanes are one run of consecutive source blocks per run, at most 64
        key = m[:, 0] * 8 + m[:, 2]
        for kk in np.unique(key)[:: max(1, len(np.unique(key)) // 50)]:
            run_ = m[key == kk]
            assert len(run_) <= 64 and len(run_) % denom == 0
            assert (np.diff(run_[:, 4]) == 1).all() and (run_[:, 3] == np.arange(len(run_))).all()
            assert run_[0, 4] // sbw == run_[-1, 4] // sbw  # one source block row


def test_runs_of_the_smallest_frame():
    """128 x 128 at 1/8: a 16 x 16 output of 4 + 1 + 1 blocks; the luma wave's
    runs have 16 live lanes, the chroma waves' 8."""
    m = D.work_map(128, 128, 8).astype(np.int64)
    waves = np.unique(m[:, 0])
    assert len(waves) == 2 + 1 + 1
    for t in waves:
        mm = m[m[:, 0] == t]
        assert set(np.unique(mm[:, 2])) == set(range(8))
        assert len(mm) == 8 * (16 if mm[0, 1] == 0 else 8)


def test_sanitized_host_build_is_clean(harness, harness_san):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for w, h, denom in GEOMETRIES:
        want, _ = run(harness, w, h, denom)
        got, err = run(harness_san, w, h, denom, env=env)
        assert b"runtime error" not in err and b"AddressSanitizer" not in err, (w, h, denom)
        assert (got == want).all(), (w, h, denom)


def test_host_program_refuses_bad_arguments(harness):
    for args in (["208", "96", "2"], ["416", "192", "3"], ["416", "192"], ["0", "64", "2"]):
        assert subprocess.run([harness, *args], capture_output=True).returncode == 2, args


def test_handle_and_pointer_errors_need_no_device():
    """MYYUV_E_ARG for a null handle or pointer, *bad_block = -1, before
    anything touches a device."""
    import myyuv_hip

    L = myyuv_hip.load()
    pay = np.zeros(64, np.uint8)
    out = np.zeros(64, np.uint8)
    qa = np.array([50, 50, 50], np.uint8)
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    size = ctypes.c_uint32(7)
    bad = ctypes.c_int64(7)
    assert L.myyuv_gpu_dct_downscale(None, u8(pay), 64, 128, 128, u8(qa), 2, u8(qa), u8(out), 64, ctypes.byref(size),
                                     ctypes.byref(bad)) == myyuv_hip.E_ARG
    assert bad.value == -1
    assert L.myyuv_gpu_dct_downscale_device(None, 256, 512, 64, 1, 128, 128, u8(qa), 2, u8(qa), 1024, 64, 2048,
                                            None) == myyuv_hip.E_ARG
    assert not (out != 0).any()


def test_bindings_name_the_kernel_and_the_symbols():
    import myyuv_hip

    assert "myyuv_gpu_dct_downscale" in myyuv_hip.EXPORTS and "myyuv_gpu_dct_downscale_device" in myyuv_hip.EXPORTS
    assert myyuv_hip.KERNELS_FULL[myyuv_hip.K_DOWNSCALE] == "downscale" and myyuv_hip.K_DOWNSCALE == 23
    assert myyuv_hip.KERNELS_FULL[:myyuv_hip.K_LIMIT] == myyuv_hip.KERNELS_EVERY
    assert myyuv_hip.K_BOUND == 24 == len(myyuv_hip.KERNELS_FULL)
    for name in ("downscale", "downscale_into", "downscale_device"):
        assert callable(getattr(myyuv_hip.Codec, name))


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def test_cli_downscale_argument_errors(tmp_path):
    """A malformed -downscale: one fixed first line, the usage, exit 1, no
    file; before the file's content matters (no GPU is touched)."""
    out = str(tmp_path / "x.out")
    first = "Invalid argument, -downscale must be followed by `1/2`, `1/4` or `1/8`"
    bad = (["-downscale"], ["-downscale", "2"], ["-downscale", "1/3"], ["-downscale", "1/16"], ["-downscale", "1/1"],
           ["-downscale", "0.5"], ["-downscale", "1/2x"], ["-downscale", "-o"], ["-downscale", ""])
    for src in (RAW, C50):
        for b in bad:
            args = [src, *b] + ([] if b[-1] == "-o" else ["-o"]) + [out]
            r = cli(*args)
            assert r.returncode == 1 and "Usage" in r.stdout, (args, r.stdout)
            assert r.stdout.splitlines()[0] == first, (args, r.stdout)
            assert not os.path.exists(out)
    r = cli(C50, "-downscale", "1/3", "-o", out)
    assert "-downscale 1/2|1/4|1/8 [-q Q [Q [Q]]] -o OUT.myyuv" in r.stdout
    # a quality out of range, as -compress DCT's
    r = cli(C50, "-downscale", "1/2", "-q", "101", "-o", out)
    assert r.returncode != 0 and "must range between [1..100]" in r.stderr and not os.path.exists(out), r.stderr
    # qualities without -q, and anything after the output
    for tail in (["50", "-o", out], ["-q", "50", "-o", out, "x"], ["-q", "50"]):
        r = cli(C50, "-downscale", "1/2", *tail)
        assert r.returncode == 1 and "Usage" in r.stdout and not os.path.exists(out), (tail, r.stdout)
        assert r.stdout.splitlines()[0] == "Invalid argument, last arguments must be `-o /path/to/new_image.myyuv`"


def test_cli_downscale_refuses_an_uncompressed_input(tmp_path):
    out = str(tmp_path / "x.out")
    r = cli(RAW, "-downscale", "1/2", "-o", out)
    assert r.returncode == 1, r.stdout
    assert r.stdout.splitlines()[0] == "Nothing to downscale, image is not compressed (-downscale needs DCT coefficients)"
    assert not os.path.exists(out)

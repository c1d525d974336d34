"""Compress from BMP, the parts that need no GPU: the work map of
csrc/bmp_fdct.h (the code k_bmp_fdct runs) compiled for the host
(tools/bmp_fdct_host.cpp), which checks on arrays of the kernel's sizes that
every source byte is read exactly once and inside the pixel array, that every
sample lands where its block's picture has it, and that every block of every
plane is handed over exactly once; the same program under ASan + UBSan; the C
ABI's pointer checks, the bindings' lists and the CLI's usage and refusals."""
import ctypes
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "tools", "bmp_fdct_host.cpp")
INC = ["-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include")]
CLI = os.path.join(PKG, "myyuv_cli")
HEADER = os.path.join(ROOT, "include", "myyuv_hip.h")

# the frames of tests/test_gpu_bmp_compress.py, the bench frame, and widths around the strip width
GEOMETRIES = [(16, 16), (272, 32), (528, 16), (992, 736), (1056, 512), (4032, 3008), (256, 16), (240, 32), (512, 48)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("bmpfdct") / "bmp_fdct_host")
    subprocess.run([HIPCC, "-O2", "-std=c++17", *INC, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same program with AddressSanitizer + UndefinedBehaviorSanitizer on
    the host (the flags of tests/test_downscale_host.py harness_san); a
    stand-alone binary, never loaded into Python."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("bmpfdctsan") / "bmp_fdct_host_san")
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-fno-gpu-sanitize"]
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17"] + san +
                   ["-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *INC, SRC, "-o", exe], check=True)
    return exe


def run(exe, w, h, orient, bpp, env=None):
    r = subprocess.run([exe, str(w), str(h), str(orient), str(bpp)], capture_output=True, env=env)
    assert r.returncode == 0, (w, h, orient, bpp, r.returncode, r.stderr.decode(errors="replace")[-2000:])
    assert len(r.stdout) % 24 == 0
    return np.frombuffer(r.stdout, np.uint32).reshape(-1, 6).astype(np.int64), r.stderr


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_every_block_once_every_pixel_once(harness, w, h):
    """The program's own checks (exit 0: every source byte read once and in
    bounds, every sample in its block's picture, no stray image byte) for the
    three orientations and both depths, and from its records: every block of
    every plane is owned exactly once, by the strip that covers it, in a unit of
    its plane."""
    ny, nc = (w // 8) * (h // 8), (w // 16) * (h // 16)
    first = None
    for orient in (0, 1, 2):
        for bpp in (3, 4):
            m, _ = run(harness, w, h, orient, bpp)
            if first is None:
                first = m
            else:  # the block map does not depend on where the pixels come from
                assert (m == first).all(), (orient, bpp)
    m = first
    assert len(m) == ny + 2 * nc
    assert (np.sort(m[:, 5]) == np.arange(ny + 2 * nc)).all()  # every block of the frame, once
    spr = -(-w // 256)
    for p, (n, bw, bs) in enumerate(((ny, w // 8, 8), (nc, w // 16, 16), (nc, w // 16, 16))):
        mp = m[m[:, 2] == p]
        assert len(mp) == n and (np.sort(mp[:, 4]) == np.arange(n)).all()
        # the block's strip: 16 luma rows by 256 luma columns
        bx, by = mp[:, 4] % bw, mp[:, 4] // bw
        assert (mp[:, 0] == (by * bs // 16) * spr + bx * bs // 256).all()
        # slots: Y below 64, then 16 for U and 16 for V; a unit holds 16 consecutive slots of one plane
        lo, hi = ((0, 64), (64, 80), (80, 96))[p]
        assert (mp[:, 3] >= lo).all() and (mp[:, 3] < hi).all()
    nstrips = spr * (h // 16)
    assert set(m[:, 0]) == set(range(nstrips))
    for s in {0, nstrips - 1, spr - 1}:
        ms = m[m[:, 0] == s]
        for k in np.unique(ms[:, 1]):
            mk = ms[ms[:, 1] == k]
            assert len(mk) <= 16 and len(np.unique(mk[:, 2])) == 1
            assert (np.diff(mk[:, 3]) == 1).all() and mk[0, 3] % 16 == 0
        nmb = len(ms) // 6
        assert len(np.unique(ms[:, 1])) == -(-nmb // 4) + 2  # the fewest units


def test_units_of_the_smallest_frame(harness):
    """16 x 16: one strip, three units of 4 + 1 + 1 live blocks."""
    m, _ = run(harness, 16, 16, 2, 4)
    assert m.tolist() == [[0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 1, 1], [0, 0, 0, 2, 2, 2], [0, 0, 0, 3, 3, 3],
                          [0, 1, 1, 64, 0, 4], [0, 2, 2, 80, 0, 5]]


def test_sanitized_host_build_is_clean(harness, harness_san):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for w, h in GEOMETRIES:
        if w * h > 1 << 22:
            continue  # (the 4032 x 3008 walk is the unsanitised test's)
        for orient, bpp in ((0, 4), (1, 3), (2, 4), (1, 4)):
            want, _ = run(harness, w, h, orient, bpp)
            got, err = run(harness_san, w, h, orient, bpp, env=env)
            assert b"runtime error" not in err and b"AddressSanitizer" not in err, (w, h, orient, bpp)
            assert (got == want).all(), (w, h, orient, bpp)


def test_host_program_refuses_bad_arguments(harness):
    for args in (["24", "16", "0", "4"], ["16", "16", "3", "4"], ["16", "16", "0", "2"], ["16", "16", "0"],
                 ["0", "16", "0", "4"]):
        assert subprocess.run([harness, *args], capture_output=True).returncode == 2, args


def test_handle_and_pointer_errors_need_no_device():
    import myyuv_hip

    L = myyuv_hip.load()
    px = np.zeros(16 * 16 * 4, np.uint8)
    out = np.zeros(64, np.uint8)
    qa = np.array([50, 50, 50], np.uint8)
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    size = ctypes.c_uint32(7)
    assert L.myyuv_gpu_bmp_dct_compress(None, u8(px), 16, 16, 32, u8(qa), u8(out), 64,
                                        ctypes.byref(size)) == myyuv_hip.E_ARG
    assert L.myyuv_gpu_bmp_dct_compress_device(None, 256, 1, 16, 16, 32, u8(qa), 1024, 64, 2048,
                                               None) == myyuv_hip.E_ARG
    assert size.value == 7 and not out.any()


def test_bindings_name_the_kernel_and_the_symbols():
    import myyuv_hip

    for name in ("myyuv_gpu_bmp_dct_compress", "myyuv_gpu_bmp_dct_compress_device"):
        assert name in myyuv_hip.EXPORTS
    # the frozen bounds keep their values
    assert (myyuv_hip.K_TOTAL, myyuv_hip.K_END, myyuv_hip.K_LIMIT, myyuv_hip.K_BOUND) == (18, 21, 23, 24)
    assert len(myyuv_hip.KERNELS) == 17 and len(myyuv_hip.KERNELS_FULL) == 24
    # the new id after them, under its own bound, in a longer list
    assert myyuv_hip.K_BMP_FDCT == 24 and myyuv_hip.K_TOP == 25 == len(myyuv_hip.KERNELS_TOP)
    assert myyuv_hip.KERNELS_TOP[:24] == myyuv_hip.KERNELS_FULL and myyuv_hip.KERNELS_TOP[24] == "bmp_fdct"
    src = open(HEADER).read()
    for name, v in (("COUNT", 17), ("TOTAL", 18), ("END", 21), ("LIMIT", 23), ("BOUND", 24), ("BMP_FDCT", 24),
                    ("TOP", 25)):
        assert re.search(rf"^#define MYYUV_K_{name} {v}\b", src, re.M), name
    for name in ("compress_bmp", "compress_bmp_into", "compress_bmp_device"):
        assert callable(getattr(myyuv_hip.Codec, name))


def cli(*args):
    return subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True)


def test_cli_usage_and_malformed_commands(tmp_path):
    """A malformed `IMAGE.bmp -compress`: one fixed first line, the usage, exit
    1, no file; before the pixels matter (no GPU is touched)."""
    bmp = tmp_path / "chef.bmp"
    with gzip.open(os.path.join(GOLDEN, "chef-with-trumpet.bmp.gz"), "rb") as f:
        bmp.write_bytes(f.read())
    out = tmp_path / "x.myyuv"
    first = "Invalid argument, -compress must be followed by `DCT Q [Q [Q]] -o /path/to/new_image.myyuv`"
    for tail in (["-compress"], ["-compress", "DCT"], ["-compress", "DCT", "50"], ["-compress", "DCT", "50", "-o"],
                 ["-compress", "50", "-o", out], ["-compress", "LZ", "50", "-o", out],
                 ["-compress", "DCT", "50", "-o", out, "extra"], ["-compress", "DCT", "50", out]):
        r = cli(bmp, *tail)
        assert r.returncode == 1 and "Usage" in r.stdout, (tail, r.stdout)
        assert r.stdout.splitlines()[0] == first, (tail, r.stdout)
        assert not out.exists()
    assert "  myyuv_cli IMAGE.bmp -compress DCT Q [Q [Q]] -o OUT.myyuv" in cli(bmp, "-compress").stdout.splitlines()
    assert "  myyuv_cli IMAGE.bmp -compress DCT Q [Q [Q]] -o OUT.myyuv" in cli().stdout.splitlines()
    # the qualities parse as the .myyuv -compress DCT's do
    for qs, msg in ((["101"], "must range between [1..100]"), (["1", "2", "3", "4"], "Too many compression parameters"),
                    ([], "Too few compression parameters")):
        r = cli(bmp, "-compress", "DCT", *qs, "-o", out)
        assert r.returncode != 0 and msg in r.stderr and not out.exists(), (qs, r.stderr)

"""Host programs around K8 (no GPU): the kernel's division-free divisions,
checked on the code the kernel compiles (csrc/color_div.hpp), and the size
guard of myyuv::yuv_to_bmp, which must refuse an image BMP's 32-bit sizes
cannot describe before it allocates or reaches for a device."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")


def build(tmp, name, extra):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp / name)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-o", exe,
                    os.path.join(ROOT, "tools", name + ".cpp")] + extra, check=True)
    return exe


def test_divisions_are_correctly_rounded(tmp_path):
    """div255 / div4080 equal the compiler's fp32 division for all 256 luma
    values and all 4081 chroma sums (the GPU tests reach every luma value but
    only the multiples of 16 and a random sample of the sums)."""
    exe = build(tmp_path, "color_div_check", ["-I", CSRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(256 + 4081)]


def test_yuv_to_bmp_refuses_what_a_bmp_cannot_hold(tmp_path):
    """BMP::imageSize() is |w| * |h| * bit_count / 8 in 32 bits and wraps from
    w * h * bit_count = 2^32 (2^27 pixels at 32 bpp): such a frame is refused
    with "Invalid argument" before any allocation."""
    exe = build(tmp_path, "yuv_to_bmp_guard", ["-I", os.path.join(CSRC, "host"), "-I", os.path.join(ROOT, "include"),
                                               "-L", PKG, "-lmyyuv_amd", "-lmyyuv_hip", "-pthread",
                                               "-Wl,-rpath," + PKG])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"

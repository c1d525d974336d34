"""myyuv_cli -downscale on the GPU: the golden q50 file cropped to 960 x 704
(the largest 64-aligned window of 992 x 736, cut by the existing -crop, so
every scale down to 1/4 is a compressible frame), downscaled by the CLI.  The
output file, header included, is compared with the file the C++ mirror's two
calls write for the same picture (-decompress -scale, then -compress DCT: the
header compress_DCT_planar makes for the scaled size) and with the reference
expression (downscaleref)."""
import os
import subprocess

import pytest

import downscaleref as D
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
W, H = 960, 704


def cli(*args):
    r = subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True)
    return r


def ok(r):
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    return r


@pytest.fixture(scope="module")
def cropped(tmp_path_factory):
    import myyuv_file

    path = str(tmp_path_factory.mktemp("downscale_cli") / "crop.myyuv")
    ok(cli(C50, "-crop", 0, 0, W, H, "-o", path))
    f = myyuv_file.YUVFile.load(path)
    assert (f.width, f.height, tuple(f.params)) == (W, H, (50, 50, 50))
    return path, f


@pytest.mark.parametrize("denom,qargs,qd", [(2, [], (50, 50, 50)), (4, ["-q", "90", "50"], (90, 50, 50))])
def test_cli_downscale(cropped, tmp_path, denom, qargs, qd):
    import myyuv_file

    path, f = cropped
    out = tmp_path / "small.myyuv"
    r = ok(cli(path, "-downscale", f"1/{denom}", *qargs, "-o", out))
    label = " ".join([f"1/{denom}"] + qargs[1:])
    assert r.stdout.splitlines()[0].startswith(f"YUV DCT downscale ( {label} ) : ")
    got = out.read_bytes()
    # the reference expression, in compress_DCT_planar's header
    want = D.cached(f.data, W, H, (50, 50, 50), denom, qd)
    assert got == myyuv_file.YUVFile(f.fourcc, W // denom, H // denom, myyuv_file.DCT, bytes(qd), want,
                                     f.unused).dumps()
    # the mirror's two calls, with the small frame as a file in between
    raw = tmp_path / "raw.myyuv"
    two = tmp_path / "two.myyuv"
    ok(cli(path, "-decompress", "-scale", f"1/{denom}", "-o", raw))
    ok(cli(raw, "-compress", "DCT", *[str(q) for q in qd], "-o", two))
    assert got == two.read_bytes()
    # and it decodes
    back = tmp_path / "back.myyuv"
    ok(cli(out, "-decompress", "-o", back))
    assert len(back.read_bytes()) == 64 + (W // denom) * (H // denom) * 3 // 2


def test_cli_downscale_usage_error(cropped, tmp_path):
    path, _ = cropped
    out = tmp_path / "x.myyuv"
    r = cli(path, "-downscale", "1/3", "-o", out)
    assert r.returncode == 1 and "Usage" in r.stdout
    assert r.stdout.splitlines()[0] == "Invalid argument, -downscale must be followed by `1/2`, `1/4` or `1/8`"
    assert not out.exists()
    # 1/8 of 960 x 704 is 120 x 88: no frame compress takes (the width rule of the scaled size)
    r = cli(path, "-downscale", "1/8", "-o", out)
    assert r.returncode != 0 and "width % 8 must be 0" in r.stderr and not out.exists()

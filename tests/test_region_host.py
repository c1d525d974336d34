"""Region decode, the parts that need no GPU: the numpy statement of a crop,
the CLI's -crop argument errors, and -crop on an uncompressed file (rows
copied on the host)."""
import os
import subprocess

import numpy as np

import regionref as R
from conftest import GOLDEN, PKG

CLI = os.path.join(PKG, "myyuv_cli")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def test_crop_of_a_hand_written_frame():
    """32x32: Y[y][x] = 8y + x/4 (mod 256), U[y][x] = 100 + 16y + x, V = 200 - that."""
    w = h = 32
    y = np.array([[(8 * r + c // 4) % 256 for c in range(w)] for r in range(h)], np.uint8)
    u = np.array([[(100 + 16 * r + c) % 256 for c in range(w // 2)] for r in range(h // 2)], np.uint8)
    v = np.array([[(200 - 16 * r - c) % 256 for c in range(w // 2)] for r in range(h // 2)], np.uint8)
    fr = y.tobytes() + u.tobytes() + v.tobytes()
    assert R.crop(fr, w, h, (0, 0, 32, 32)) == fr
    got = R.crop(fr, w, h, (16, 0, 16, 16))
    assert len(got) == 16 * 16 * 3 // 2
    # first luma row: pixels (16..31, 0); last luma row: (16..31, 15)
    assert got[:16] == bytes([4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7])
    assert got[15 * 16: 16 * 16] == bytes(v + 120 for v in (4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7))
    # chroma: columns 8..15, rows 0..7 of U, then of V
    assert got[256: 256 + 8] == bytes(range(108, 116))
    assert got[256 + 56: 256 + 64] == bytes(range(108 + 112, 116 + 112))
    assert got[320: 328] == bytes(range(192, 184, -1))
    got = R.crop(fr, w, h, (0, 16, 16, 16))
    assert got[:4] == bytes([128] * 4) and got[256] == 100 + 16 * 8 and got[320] == 200 - 16 * 8
    assert R.contains_block(w, h, (16, 0, 16, 16), 2) and R.contains_block(w, h, (16, 0, 16, 16), 7)
    assert not R.contains_block(w, h, (16, 0, 16, 16), 1) and not R.contains_block(w, h, (16, 0, 16, 16), 10)
    # blocks 16..19 are U's, 20..23 V's: each 16x16 of luma has one of each
    assert R.contains_block(w, h, (16, 0, 16, 16), 17) and R.contains_block(w, h, (16, 0, 16, 16), 21)
    assert not R.contains_block(w, h, (16, 0, 16, 16), 16) and not R.contains_block(w, h, (16, 0, 16, 16), 23)
    assert R.block_rect(w, h, 0, 7) == (16, 0, 16, 16) and R.block_rect(w, h, 2, 3) == (16, 16, 16, 16)


def test_cli_crop_argument_errors(tmp_path):
    """Fewer than four numbers, or something that is no number: the usage and
    a non-zero exit, before the file's content matters (a compressed input
    would need the GPU; none is touched)."""
    out = str(tmp_path / "x.out")
    bad = (["-crop"], ["-crop", "0", "0", "16"], ["-crop", "0", "0", "16", "-o"], ["-crop", "0", "0", "16", "x"],
           ["-crop", "-16", "0", "16", "16"], ["-crop", "0", "0", "1e2", "16"], ["-crop", "0", "0", "16", "99999999999"],
           ["-crop", "0", "0", "16", "16", "16"])
    for src in (RAW, C50):
        for head in (["-decompress"], ["-to_bmp"], ["-to_bmp", "24", "-chroma", "nearest"]):
            for b in bad:
                r = run(src, *head, *b, "-o", out)
                assert r.returncode == 1 and "Usage" in r.stdout, (src, head, b, r.stdout)
                if len(b) != 6:  # (five numbers: the fifth is not `-o`, that command's own message)
                    assert r.stdout.splitlines()[0] == \
                        "Invalid argument, -crop must be followed by four numbers `X Y W H`", (src, head, b)
                assert not os.path.exists(out)
    r = run(RAW, "-decompress", "-crop", "0", "0", "16", "-o", out)
    assert r.stdout.splitlines()[0] == "Invalid argument, -crop must be followed by four numbers `X Y W H`"
    # without -crop an uncompressed input still has nothing to decompress
    r = run(RAW, "-decompress", "-o", out)
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "Nothing to decompress, image is not compressed"


def test_cli_crop_of_an_uncompressed_file(tmp_path, golden):
    import myyuv_file

    f = golden("chef-with-trumpet.myyuv")
    assert (f.width, f.height) == (992, 736)
    region = (496, 368, 256, 128)
    out = tmp_path / "crop.myyuv"
    r = run(RAW, "-decompress", "-crop", *map(str, region), "-o", str(out))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "Success!"
    want = R.crop(f.data, f.width, f.height, region)
    # the header decompress writes (compression 0, no parameters, data at 64) with the region's size
    assert out.read_bytes() == myyuv_file.YUVFile(f.fourcc, 256, 128, myyuv_file.NONE, b"", want, f.unused).dumps()
    g = myyuv_file.YUVFile.load(str(out))
    assert (g.width, g.height, g.compression, g.params, g.data) == (256, 128, 0, b"", want)


def test_cli_crop_region_constraints_on_the_host(tmp_path):
    """An uncompressed input's region is checked on the host, with the C
    ABI's rules: the reference's "Invalid argument" text, no output."""
    out = tmp_path / "x.myyuv"
    for region in ((8, 0, 16, 16), (0, 8, 16, 16), (0, 0, 24, 16), (0, 0, 16, 24), (0, 0, 0, 16), (0, 0, 16, 0),
                   (992, 0, 16, 16), (0, 736, 16, 16), (4294967280, 0, 32, 16)):
        r = run(RAW, "-decompress", "-crop", *map(str, region), "-o", str(out))
        assert r.returncode != 0 and "Invalid argument" in r.stderr, (region, r.stdout, r.stderr)
        assert not out.exists()

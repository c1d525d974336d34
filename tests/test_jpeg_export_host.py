"""Export to JPEG, the parts that need no GPU: the block code and header
writer of csrc/jpeg_export.h (the code k_jpeg_export runs) compiled for the
host (tools/jpeg_export_host.cpp) against the Python restatement (jpegref) of
the definition in include/myyuv_hip.h, byte for byte; the restatement against
its own independent parser and against libjpeg (Pillow): the DHT constants, and
the decoded picture against the oracle's decode of the same stream; the bound;
the argument errors of the CLI and the C ABI that come before any device is
touched."""
import ctypes
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import coefgen
import jpegref as J
import regionref as R
import scaleref as S
from conftest import GOLDEN, PKG, ROOT

SRC = os.path.join(ROOT, "tools", "jpeg_export_host.cpp")
CLI = os.path.join(PKG, "myyuv_cli")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
FRAMES = ((16, 16, (50, 50, 50)), (208, 96, (90, 50, 30)), (1040, 64, (50, 50, 50)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jpeg") / "jpeg_export_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), SRC, "-o", exe],
                   check=True)
    return exe


def run(exe, planes, w, h, qtables):
    inp = struct.pack("<II", w, h) + b"".join(bytes(int(v) for v in np.asarray(t).reshape(64)) for t in qtables)
    inp += b"".join(np.ascontiguousarray(p, "<i2").tobytes() for p in planes)
    r = subprocess.run([exe], input=inp, capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-2000:])
    return r.stdout


def first_difference(a, b):
    n = min(len(a), len(b))
    x, y = np.frombuffer(a[:n], np.uint8), np.frombuffer(b[:n], np.uint8)
    d = np.nonzero(x != y)[0]
    return (len(a), len(b), int(d[0]) if len(d) else None, len(d))


def maximal_planes(w, h, seed=5):
    """Every AC +-1023 and the DC alternating -1024 / 1023 in every block: the
    longest code of every block (natural order)."""
    rng = np.random.default_rng(seed)
    out = []
    for n in coefgen.plane_counts(w, h):
        b = np.where(rng.integers(0, 2, (n, 64)) == 1, 1023, -1023).astype(np.int16)
        b[0::2, 0] = -1024
        b[1::2, 0] = 1023
        out.append(b)
    return out


def crafted_planes(w, h, seed=9):
    """Natural-order planes of blocks around every branch of the block code:
    zero runs of 15, 16, 31, 32 and 47, coefficient 63 alone and among others,
    +-1023 and -1024, the DC swing, all-zero blocks."""
    rng = np.random.default_rng(seed)
    pool = []
    for run_ in (15, 16, 31, 32, 47):
        b = np.zeros(64, np.int16)
        b[0], b[1 + run_] = 5, -3
        pool.append(b)
    b = np.zeros(64, np.int16)
    b[63] = -2
    pool.append(b)
    b = np.zeros(64, np.int16)
    b[0], b[1], b[40], b[63] = 100, -1, 9, 1
    pool.append(b)
    for ac in (1023, -1024, -1023):
        b = np.zeros(64, np.int16)
        b[0], b[1], b[17], b[62] = 1, ac, ac, ac
        pool.append(b)
    for dc in (-1024, 1023, -1024, 1023, 0):
        b = np.zeros(64, np.int16)
        b[0] = dc
        pool.append(b)
    pool = np.stack(pool)
    return [coefgen.natural(pool[np.concatenate([np.arange(len(pool)), rng.integers(0, len(pool), n)])[:n]])
            for n in coefgen.plane_counts(w, h)]


# ---------------------------------------------------------- the shared header
@pytest.mark.parametrize("w,h,q", FRAMES)
def test_shared_header_equals_the_reference_on_frames(harness, oracle, w, h, q):
    pay = R.tiled_stream(w, h, q)[0]
    want = J.export(pay, w, h, q)
    got = run(harness, S.coefficients(pay), w, h, J.qtables_of(q))
    assert got == want, first_difference(got, want)


def test_shared_header_equals_the_reference_on_noise(harness, oracle):
    w, h, q = 208, 96, (100, 100, 100)
    pay = R.noise_stream(w, h)[0]
    want = J.export(pay, w, h, q)
    assert want.count(b"\xff\x00") >= 50  # the byte stuffing works
    got = run(harness, S.coefficients(pay), w, h, J.qtables_of(q))
    assert got == want, first_difference(got, want)


@pytest.mark.parametrize("planes", ["crafted", "maximal"])
def test_shared_header_equals_the_reference_on_crafted_blocks(harness, oracle, planes):
    w, h, q = 128, 64, (50, 60, 70)
    pl = crafted_planes(w, h) if planes == "crafted" else maximal_planes(w, h)
    qt = J.qtables_of(q)
    want = J.export_planes(pl, w, h, qt)
    got = run(harness, pl, w, h, qt)
    assert got == want, first_difference(got, want)


def test_host_tool_rejects_bad_dimensions(harness):
    qt = [np.ones(64)] * 3
    for w, h in ((0, 16), (24, 16), (16, 8)):
        r = subprocess.run([harness], input=struct.pack("<II", w, h) + bytes(192), capture_output=True)
        assert r.returncode == 2, (w, h)
    assert len(run(harness, [np.zeros((4, 64), np.int16)] + [np.zeros((1, 64), np.int16)] * 2, 16, 16, qt)) > 600


# ------------------------------------------------- the reference's own parser
@pytest.mark.parametrize("w,h,q", FRAMES)
def test_parse_returns_the_coefficients_and_tables(oracle, w, h, q):
    pay = R.tiled_stream(w, h, q)[0]
    pw, ph, planes, qt = J.parse(J.export(pay, w, h, q))
    assert (pw, ph) == (w, h)
    for p, want in enumerate(S.coefficients(pay)):
        assert planes[p].shape == want.shape and (planes[p] == want).all(), p
        assert (qt[p] == np.asarray(oracle.qtable(q[p], p != 0)).reshape(64)).all(), p


def test_parse_returns_crafted_blocks_but_for_the_clamp(oracle):
    w, h, q = 128, 64, (1, 50, 100)
    for pl in (crafted_planes(w, h), maximal_planes(w, h)):
        _, _, planes, _ = J.parse(J.export_planes(pl, w, h, J.qtables_of(q)))
        for p in range(3):
            want = np.where(pl[p] == -1024, -1023, pl[p])
            want[:, 0] = pl[p][:, 0]  # DC differences have category 11: no clamp
            assert (planes[p] == want).all(), p
    assert all((crafted_planes(w, h)[p][:, 1:] == -1024).any() for p in range(3))  # the clamp was reached


def test_rst_sequence_and_interval_counts(oracle):
    w, h, q = 1040, 64, (50, 50, 50)
    data = J.export(R.tiled_stream(w, h, q)[0], w, h, q)
    scans = data.split(b"\xff\xda")[1:]
    assert len(scans) == 3
    for p, sc in enumerate(scans):
        ms = [sc[i + 1] - 0xD0 for i in range(len(sc) - 1) if sc[i] == 0xFF and 0xD0 <= sc[i + 1] <= 0xD7]
        n = 17 if p == 0 else 5
        assert ms == [i % 8 for i in range(n - 1)], p
    assert data.endswith(b"\xff\xd9") and data.count(b"\xff\xd9") == 1


# ------------------------------------------------------------------- libjpeg
def test_dht_constants_are_libjpegs():
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.new("YCbCr", (32, 32)).save(buf, "JPEG", optimize=False)
    theirs = J.dht_segments(buf.getvalue())
    assert sorted(theirs) == [0x00, 0x01, 0x10, 0x11]
    for tc_th, (bits, vals) in J.DHT:
        assert theirs[tc_th] == (bits, vals), hex(tc_th)


def fancy_upsample(plane):
    """libjpeg's h2v2 fancy upsampling (jdsample.c) of one chroma plane."""
    ph, pw = plane.shape
    p = np.pad(np.asarray(plane, int), 1, mode="edge")
    out = np.zeros((2 * ph, 2 * pw), int)
    for y in range(2 * ph):
        for x in range(2 * pw):
            sy, sx = y // 2 + 1, x // 2 + 1
            ny, nx = sy + (1 if y % 2 else -1), sx + (1 if x % 2 else -1)
            near, far = 3 * p[sy, sx] + p[ny, sx], 3 * p[sy, nx] + p[ny, nx]
            out[y, x] = (3 * near + far + (8 if x % 2 == 0 else 7)) >> 4
    return out


@pytest.mark.parametrize("w,h,q", FRAMES)
def test_libjpeg_decodes_the_file_to_the_oracles_frame(oracle, w, h, q):
    """Luma within 1 of the oracle's decode (libjpeg's integer inverse
    transform against the fp32 one); at 16x16, where each chroma plane is one
    block and the upsampler has no neighbour to smooth with, chroma too."""
    Image = pytest.importorskip("PIL.Image")
    pay, dec = R.tiled_stream(w, h, q)
    im = Image.open(io.BytesIO(J.export(pay, w, h, q)))
    im.draft("YCbCr", (w, h))
    assert im.mode == "YCbCr" and im.size == (w, h)
    px = np.asarray(im).astype(int)
    ref = np.frombuffer(dec, np.uint8).astype(int)
    y = ref[:w * h].reshape(h, w)
    d = np.abs(px[:, :, 0] - y)
    print(f"{w}x{h} q{q}: luma max |diff| {d.max()}, differing {np.count_nonzero(d) / d.size:.4f}")
    assert d.max() <= 1
    if (w, h) == (16, 16):
        for c in (1, 2):
            plane = ref[w * h + (c - 1) * (w * h // 4):w * h + c * (w * h // 4)].reshape(h // 2, w // 2)
            # Pillow shows chroma only through libjpeg's h2v2 "fancy" upsampler
            # (3:1 vertically, then 3:1 horizontally, rounding 8 / 7 on even /
            # odd columns, edges replicated).  The same filter over the oracle's
            # plane must give libjpeg's picture exactly: every chroma SAMPLE is
            # equal.  The four corners pass through the filter unchanged.
            assert (px[:, :, c] == fancy_upsample(plane)).all(), c
            for y, x in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
                assert px[y, x, c] == plane[y, x], (c, y, x)


# ----------------------------------------------------------------- the bound
def test_bound_covers_the_worst_case(oracle):
    import myyuv_hip

    for w, h in ((16, 16), (128, 64)):
        worst = J.export_planes(maximal_planes(w, h), w, h, J.qtables_of((100, 100, 100)))
        ny, nc, _ = coefgen.plane_counts(w, h)
        assert len(worst) > (ny + 2 * nc) * 170  # (luma blocks 1,658 bits, chroma blocks 1,408)
        assert myyuv_hip.jpeg_bound(w, h) >= len(worst)
    # header bytes, scan headers and EOI; per block twice 208 B; the restart markers
    for w, h in ((16, 16), (1040, 64), (8192, 8192), (65520, 65520)):
        ny, nc, _ = coefgen.plane_counts(w, h)
        iv = -(-ny // 64) + 2 * -(-nc // 64)
        assert myyuv_hip.jpeg_bound(w, h) == len(J.header(16, 16, [np.ones(64)] * 3)) + 32 + (ny + 2 * nc) * 416 + 2 * iv


# ---------------------------------------- argument errors that need no device
def test_handle_and_pointer_errors_need_no_device():
    import myyuv_hip

    L = myyuv_hip.load()
    pay = np.zeros(64, np.uint8)
    out = np.zeros(64, np.uint8)
    qa = np.array([50, 50, 50], np.uint8)
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    size = ctypes.c_uint32(9)
    bad = ctypes.c_int64(7)
    assert L.myyuv_gpu_dct_to_jpeg(None, u8(pay), 64, 16, 16, u8(qa), u8(out), 64, ctypes.byref(size),
                                   ctypes.byref(bad)) == myyuv_hip.E_ARG
    assert bad.value == -1 and size.value == 9
    assert L.myyuv_gpu_dct_to_jpeg_device(None, 256, 512, 64, 1, 16, 16, u8(qa), 1024, 64, 2048,
                                          None) == myyuv_hip.E_ARG
    assert L.myyuv_gpu_iyuv_to_jpeg(None, u8(pay), 16, 16, u8(qa), u8(out), 64, ctypes.byref(size)) == myyuv_hip.E_ARG
    assert not (out != 0).any() and size.value == 9
    for name in ("myyuv_jpeg_bound", "myyuv_gpu_dct_to_jpeg", "myyuv_gpu_dct_to_jpeg_device",
                 "myyuv_gpu_iyuv_to_jpeg"):
        assert name in myyuv_hip.EXPORTS and getattr(L, name)
    assert (myyuv_hip.K_JPEG, myyuv_hip.K_JPEG_PLACE, myyuv_hip.K_MAX) == (25, 26, 27)
    assert myyuv_hip.KERNELS_MAX[:25] == myyuv_hip.KERNELS_TOP and len(myyuv_hip.KERNELS_MAX) == 27
    assert myyuv_hip.KERNELS_MAX[25:] == ["jpeg_export", "jpeg_place"]
    assert myyuv_hip.E_JPEG_DIM == 20
    assert myyuv_hip.error_message(20) == "JPEG width and height must not exceed 65535"


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def test_cli_to_jpeg_argument_errors(tmp_path):
    out = str(tmp_path / "x.jpg")
    # no output file, or more after it
    for tail in ([], ["-o"], ["-o", out, "extra"], ["50", "-o", out]):
        r = cli(C50, "-to_jpeg", *tail)
        assert r.returncode == 1 and "Usage" in r.stdout, (tail, r.stdout)
        assert r.stdout.splitlines()[0] == "Invalid argument, last arguments must be `-o /path/to/new_image.jpg`"
    # -q belongs to an uncompressed input, and such an input needs it
    r = cli(C50, "-to_jpeg", "-q", "50", "-o", out)
    assert r.returncode == 1 and r.stdout.startswith("Invalid argument, -to_jpeg takes -q for an uncompressed image")
    r = cli(RAW, "-to_jpeg", "-o", out)
    assert r.returncode == 1 and "Usage" in r.stdout
    assert r.stdout.splitlines()[0] == "Invalid argument, -to_jpeg of an uncompressed image needs `-q Q [Q [Q]]`"
    # the qualities, parsed as -compress DCT's (the exception propagates, as in the reference CLI)
    for params, msg in ((["0"], "must range between [1..100]"), (["101"], "must range between [1..100]"),
                        (["50", "50", "50", "50"], "Too many compression parameters"),
                        ([], "Too few compression parameters")):
        r = cli(RAW, "-to_jpeg", "-q", *params, "-o", out)
        assert r.returncode != 0 and msg in r.stderr, (params, r.returncode, r.stderr)
    assert not os.path.exists(out)
    assert "-to_jpeg [-q Q [Q [Q]]] -o OUT.jpg" in cli(C50, "-to_jpeg").stdout

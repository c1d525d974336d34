"""K8 IYUV -> BMP on the GPU (csrc/k_color.hip) against the restatement in
tests/colorref.py: byte equality everywhere, no tolerances."""
import functools
import os
import subprocess

import numpy as np
import pytest

import colorref as C
import malformed
from conftest import GOLDEN, PKG, ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "myyuv_cli_ref")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")

# one tile with every neighbour clamped; two tiles; a vertical neighbour on one
# side only; a tile row that is no multiple of a wave; a long row; many rows
SHAPES = [(4, 2), (8, 2), (4, 4), (44, 6), (992, 6), (64, 48)]


# ------------------------------------------------------------- small shapes
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("mode", [C.NEAREST, C.LINEAR])
def test_small_shapes(codec, w, h, mode):
    fr = C.random_frame(w, h, 1000 * w + h)
    for bits in (24, 32):
        for sw, sh in C.ORIENTS:
            got = codec.iyuv_to_bmp(fr, sw * w, sh * h, bits, mode)
            assert got == C.to_bmp(fr, sw * w, sh * h, bits, mode), (bits, sw, sh)


# -------------------------------------------------------------------- batch
@pytest.mark.parametrize("mode", [C.NEAREST, C.LINEAR])
@pytest.mark.parametrize("bits", [24, 32])
def test_batch_of_three(codec, mode, bits):
    """Three frames in one launch: each equals its single-frame call, and the
    chroma clamp is per frame (frame 0's last chroma row and column, frame 1's
    first: a kernel that let a neighbour cross into the next plane or frame
    would differ from the restatement there)."""
    import torch

    w, h, nf = 12, 4, 3
    fr = C.random_frame(w, h, 77, nf)
    fb, ob = w * h * 3 // 2, w * h * bits // 8
    dev = torch.device("cuda", 0)
    d_in = torch.frombuffer(bytearray(fr), dtype=torch.uint8).to(dev)
    d_out = torch.zeros(nf * ob, dtype=torch.uint8, device=dev)
    codec.iyuv_to_bmp_device(d_in.data_ptr(), nf, w, -h, bits, mode, d_out.data_ptr(),
                             torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = bytes(d_out.cpu().numpy())
    want = C.pixels(C.restate(fr, w, h, mode, nf), bits)
    for f in range(nf):
        assert got[f * ob:(f + 1) * ob] == codec.iyuv_to_bmp(fr[f * fb:(f + 1) * fb], w, -h, bits, mode), f
        assert got[f * ob:(f + 1) * ob] == want[f].tobytes(), f
    if mode == C.LINEAR:
        # the per-frame clamp, spelt out: frame 0's last row and column, frame 1's first
        g = np.frombuffer(got, np.uint8).reshape(nf, h, w, bits // 8)
        assert np.array_equal(g[0, h - 1], want[0, h - 1]) and np.array_equal(g[0, :, w - 1], want[0, :, w - 1])
        assert np.array_equal(g[1, 0], want[1, 0]) and np.array_equal(g[1, :, 0], want[1, :, 0])


# ------------------------------------------------------- exhaustive NEAREST
@functools.lru_cache(maxsize=None)
def exhaustive():
    fr = C.exhaustive_frame()
    y, u, v = C.planes(fr, 4096, 4096)
    up = lambda p: np.repeat(np.repeat(p[0], 2, 0), 2, 1)
    want = C.pixels(C.nearest_table()[y[0], up(u), up(v)], 32)
    return fr, want.tobytes()


def test_exhaustive_nearest(codec):
    """All 2^24 (Y, U, V) triples in one 4096x4096 frame, 32 bpp, rows as stored."""
    fr, want = exhaustive()
    got = codec.iyuv_to_bmp(fr, 4096, -4096, 32, C.NEAREST)
    if got != want:
        g = np.frombuffer(got, np.uint8).reshape(-1, 4)
        w = np.frombuffer(want, np.uint8).reshape(-1, 4)
        bad = np.flatnonzero((g != w).any(1))
        pytest.fail(f"{bad.size} pixels differ, first at {bad[0]}: {g[bad[0]]} != {w[bad[0]]}")


# ------------------------------------------------- order sensitivity, LINEAR
@functools.lru_cache(maxsize=None)
def sensitive():
    w = h = 2048
    fr = C.random_frame(w, h, 1)
    f32 = C.restate(fr, w, h, C.LINEAR)[0]
    n64 = int((f32 != C.restate(fr, w, h, C.LINEAR, variant="f64")[0]).any(-1).sum())
    nfma = int((f32 != C.restate(fr, w, h, C.LINEAR, variant="fma")[0]).any(-1).sum())
    return fr, C.pixels(f32, 32).tobytes(), n64, nfma


def test_linear_keeps_the_order(codec):
    """A random 2048x2048 frame has pixels (green only) whose byte depends on
    fp32 versus float64 (seed 1: 140) and on green's products not being fused
    (20): the kernel must match the restatement on all of them."""
    fr, want, n64, nfma = sensitive()
    assert n64 >= 50 and nfma >= 8, (n64, nfma)
    got = codec.iyuv_to_bmp(fr, 2048, -2048, 32, C.LINEAR)
    if got != want:
        g = np.frombuffer(got, np.uint8).reshape(-1, 4)
        w = np.frombuffer(want, np.uint8).reshape(-1, 4)
        bad = np.flatnonzero((g != w).any(1))
        pytest.fail(f"{bad.size} pixels differ, first at {bad[0]}: {g[bad[0]]} != {w[bad[0]]}")


# -------------------------------------------------------- decompress_to_bmp
@functools.lru_cache(maxsize=None)
def decoded(name):
    import myyuv_file
    from oracle import oracle as O

    f = myyuv_file.YUVFile.load(os.path.join(GOLDEN, name))
    return f, O.decompress(f.data, f.width, f.height, tuple(f.params))


@pytest.mark.parametrize("bits,mode", [(32, C.LINEAR), (24, C.NEAREST)])
def test_decompress_to_bmp(codec, bits, mode):
    f, raw = decoded("chef-with-trumpet-DCT-50.myyuv")
    got = codec.decompress_to_bmp(f.data, f.width, f.height, tuple(f.params), bits, mode)
    assert got == C.to_bmp(raw, f.width, f.height, bits, mode)


def test_decompress_to_bmp_frames(codec, oracle):
    """Three streams of one geometry and different lengths through the
    pipeline: the q50 golden, the q90 golden, the q50 one again.  A call has
    one quality triple; the q90 stream dequantised with the q50 tables is as
    well defined as any (the oracle decodes it the same way)."""
    f50, _ = decoded("chef-with-trumpet-DCT-50.myyuv")
    f90, _ = decoded("chef-with-trumpet-DCT-90.myyuv")
    assert (f50.width, f50.height) == (f90.width, f90.height)
    w, h, q = f50.width, f50.height, tuple(f50.params)
    streams = [f50.data, f90.data, f50.data]
    got = codec.decompress_to_bmp_frames(streams, w, -h, q, 32, C.LINEAR)
    assert len(got) == 3
    for g, s in zip(got, streams):
        assert g == C.to_bmp(oracle.decompress(s, w, h, q), w, -h, 32, C.LINEAR)
    assert got[0] == got[2] != got[1]


def test_decompress_to_bmp_frames_in_chunks(codec):
    """17 streams run as chunks of two frames and a last chunk of one (the
    pipeline takes a batch in about eight chunks): the decoder's frames of a
    chunk lie side by side in the scratch K8 reads."""
    f50, raw50 = decoded("chef-with-trumpet-DCT-50.myyuv")
    w, h, q = f50.width, f50.height, tuple(f50.params)
    want = C.to_bmp(raw50, w, h, 24, C.LINEAR)
    got = codec.decompress_to_bmp_frames([f50.data] * 17, w, h, q, 24, C.LINEAR)
    assert len(got) == 17 and all(g == want for g in got)


def test_decompress_to_bmp_errors_are_decompress_errors(codec):
    import myyuv_hip

    f, _ = decoded("chef-with-trumpet-DCT-50.myyuv")
    q = tuple(f.params)
    for name, payload, kind in malformed.cases(f.data):
        if kind != "defined":
            continue
        with pytest.raises(myyuv_hip.CodecError) as a:
            codec.decompress(payload, f.width, f.height, q)
        with pytest.raises(myyuv_hip.CodecError) as b:
            codec.decompress_to_bmp(payload, f.width, f.height, q)
        assert (b.value.code, b.value.bad_block) == (a.value.code, a.value.bad_block), name
        with pytest.raises(myyuv_hip.CodecError) as c:
            codec.decompress_to_bmp_frames([f.data, payload, f.data], f.width, f.height, q)
        with pytest.raises(myyuv_hip.CodecError) as d:
            codec.decompress_frames([f.data, payload, f.data], f.width, f.height, q)
        assert (c.value.code, c.value.bad_block) == (d.value.code, d.value.bad_block), name
    # the context still works
    assert codec.decompress_to_bmp(f.data, f.width, f.height, q) == C.to_bmp(decoded(
        "chef-with-trumpet-DCT-50.myyuv")[1], f.width, f.height, 32, C.LINEAR)


@pytest.mark.parametrize("w,h,bits,chroma,code", [(6, -2, 32, 1, 15), (-4, -2, 32, 1, 16), (4, -3, 32, 1, 17),
                                                  (4, -2, 16, 1, 17), (4, -2, 32, 2, 1)])
def test_argument_errors_with_a_context(codec, w, h, bits, chroma, code):
    import myyuv_hip

    with pytest.raises(myyuv_hip.CodecError) as e:
        codec.iyuv_to_bmp(bytes(64), w, h, bits, chroma)
    assert e.value.code == code


def test_decompress_to_bmp_needs_whole_blocks(codec):
    """|width| and |height| pass the decoder's % 8 checks (per plane) too."""
    import myyuv_hip

    f, _ = decoded("chef-with-trumpet-DCT-50.myyuv")
    with pytest.raises(myyuv_hip.CodecError) as e:
        codec.decompress_to_bmp(f.data, 24, -16, tuple(f.params))
    assert e.value.code == myyuv_hip.E_WIDTH


# ------------------------------------------------------------- kernel stats
def test_kernel_stats_count_the_launches(codec):
    fr = C.random_frame(64, 48, 9)
    codec.profile(True)
    try:
        for _ in range(3):
            codec.iyuv_to_bmp(fr, 64, -48, 32, C.LINEAR)
        codec.iyuv_to_bmp(fr, 64, -48, 24, C.NEAREST)
        ms, n = codec.kernel_stats()["iyuv_to_bmp"]
    finally:
        codec.profile(False)
    assert n == 4 and ms > 0


# ---------------------------------------------------------------------- CLI
def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True)


@pytest.mark.parametrize("src", [RAW, C50])
@pytest.mark.parametrize("opts,bits,mode", [([], 32, C.LINEAR), (["24", "-chroma", "nearest"], 24, C.NEAREST)])
def test_cli_to_bmp(tmp_path, oracle, golden, src, opts, bits, mode):
    import myyuv_file

    f = golden(os.path.basename(src))
    raw = f.data if f.compression == myyuv_file.NONE else decoded(os.path.basename(src))[1]
    out = tmp_path / "out.bmp"
    r = run(CLI, src, "-to_bmp", *opts, "-o", str(out))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith(f"YUV to BMP ({bits} {'linear' if mode else 'nearest'}) : ") and lines[0].endswith(" ms")
    assert lines[-1] == "Success!"
    b = myyuv_file.BMPFile.load(str(out))
    assert b.is_valid_header()
    assert (b.width, b.height, b.bit_count) == (f.width, f.height, bits)  # bottom-up
    want = C.to_bmp(raw, f.width, f.height, bits, mode)
    assert b.data == want
    # the headers are the ones BMPFile.dumps (BMP::dump's layout) writes
    assert out.read_bytes() == myyuv_file.BMPFile(f.width, f.height, bits, want).dumps()
    # and back through K7
    back = tmp_path / "back.myyuv"
    r = run(CLI, str(out), "-to_yuv", "IYUV", "-o", str(back))
    assert r.returncode == 0, r.stdout + r.stderr
    assert myyuv_file.YUVFile.load(str(back)).data == oracle.bmp_to_iyuv(want, f.width, f.height, bits)


def test_cli_to_bmp_is_valid_for_the_reference(tmp_path):
    if not os.path.exists(REF_CLI):
        pytest.skip("reference CLI not built (make -C oracle ref)")
    out = tmp_path / "out.bmp"
    assert run(CLI, RAW, "-to_bmp", "-o", str(out)).returncode == 0
    r = run(REF_CLI, str(out), "-info")
    assert r.returncode == 0 and "Valid: 1" in r.stdout.splitlines()


def test_cli_to_bmp_argument_errors(tmp_path):
    out = str(tmp_path / "x.bmp")
    for args in ([RAW, "-to_bmp"], [RAW, "-to_bmp", "32"], [RAW, "-to_bmp", "32", out],
                 [RAW, "-to_bmp", "16", "-o", out], [RAW, "-to_bmp", "-chroma", "cubic", "-o", out]):
        r = run(CLI, *args)
        assert r.returncode == 1 and "Usage" in r.stdout, args
        assert not os.path.exists(out)
    assert run(CLI, RAW, "-to_bmp", "16", "-o", out).stdout.splitlines()[0] == "Invalid bit count 16, must be 24 or 32"
    assert run(CLI, RAW, "-bogus").stdout.splitlines()[0] == "Invalid command -bogus"

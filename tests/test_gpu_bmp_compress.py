"""Compress from BMP on the GPU (k_bmp_fdct<BPP>, csrc/k_transform.hip, then K2
and K4; include/myyuv_hip.h, "Compress from BMP"): every stream equals
oracle.compress(oracle.bmp_to_iyuv(...), ...) byte for byte, with no tolerance.
Every case runs twice on one context.

The shapes follow the kernel's work map (csrc/bmp_fdct.h: a wave owns a strip
of 16 pixel rows by up to 256 columns): 16 x 16 is the smallest frame (one
strip of one macroblock: 4 + 1 + 1 blocks, every unit mostly unused slots);
272 x 32 a full strip plus a one-macroblock strip, in two strip rows (block
rows of 34 and 17); 528 x 16 three strips with a narrow last one; 1056 x 512
(8448 / 2112 / 2112 blocks) puts the ends of the 4096-block scan tiles inside Y
and across both plane boundaries; the golden 992 x 736 picture has a last strip
224 wide."""
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from test_color import ORIENTS, chef_bmp

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
Q50 = (50, 50, 50)


def pixels(w, h, bits, kind, seed=0):
    """A BMP pixel array of |w| x |h| as stored."""
    W, H, bpp = abs(w), abs(h), bits // 8
    rng = np.random.default_rng(1000 * seed + W + H + bits)
    if kind == "noise":  # every block to the overflow tiers
        a = rng.integers(0, 256, (H, W, bpp), dtype=np.uint8)
    elif kind == "flat":  # one-symbol blocks, closed-form chunks
        a = np.empty((H, W, bpp), np.uint8)
        a[...] = np.array([37, 150, 201, 255][:bpp], np.uint8)
    elif kind == "blue":  # saturated blue: the chroma sum wraps
        a = np.zeros((H, W, bpp), np.uint8)
        a[..., 0] = 255
    elif kind == "gradient":
        y, x = np.mgrid[0:H, 0:W]
        a = np.zeros((H, W, bpp), np.uint8)
        a[..., 0] = (x * 255 // max(1, W - 1)).astype(np.uint8)
        a[..., 1] = (y * 255 // max(1, H - 1)).astype(np.uint8)
        a[..., 2] = ((x + y) * 255 // max(1, W + H - 2)).astype(np.uint8)
    else:
        raise ValueError(kind)
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def case(w, h, bits, kind, seed, q):
    """(pixel array, the oracle's IYUV frame, the oracle's stream), computed once."""
    from oracle import oracle as O

    data = pixels(w, h, bits, kind, seed)
    iyuv = O.bmp_to_iyuv(data, w, h, bits)
    return data, iyuv, O.compress(iyuv, abs(w), abs(h), q)


def twice(codec, data, w, h, bits, q):
    a = codec.compress_bmp(data, w, h, bits, q)
    b = codec.compress_bmp(data, w, h, bits, q)
    assert a == b
    return a


def check(codec, w, h, bits, kind="noise", seed=0, q=Q50):
    data, _, want = case(w, h, bits, kind, seed, q)
    got = twice(codec, data, w, h, bits, q)
    assert len(got) == len(want)
    assert got == want


@pytest.mark.parametrize("bits", [24, 32])
@pytest.mark.parametrize("sw,sh", ORIENTS)
def test_smallest_frame(codec, sw, sh, bits):
    check(codec, sw * 16, sh * 16, bits)


@pytest.mark.parametrize("bits", [24, 32])
@pytest.mark.parametrize("sw,sh", ORIENTS)
@pytest.mark.parametrize("w,h", [(272, 32), (528, 16)])
def test_partial_strips(codec, w, h, sw, sh, bits):
    check(codec, sw * w, sh * h, bits)


@pytest.mark.parametrize("bits,sw,sh", [(32, 1, 1), (24, -1, 1)])
def test_scan_tile_boundaries(codec, bits, sw, sh):
    check(codec, sw * 1056, sh * 512, bits, "gradient")


def test_golden_chef(codec, golden):
    b = chef_bmp()
    assert (abs(b.width), abs(b.height), b.bit_count) == (992, 736, 32)
    assert twice(codec, b.data, b.width, b.height, b.bit_count, Q50) == golden("chef-with-trumpet-DCT-50.myyuv").data


@pytest.mark.parametrize("bits", [24, 32])
@pytest.mark.parametrize("kind", ["noise", "flat", "blue", "gradient"])
def test_content(codec, kind, bits):
    check(codec, 272, -32, bits, kind, seed=1)


@pytest.mark.parametrize("q", [(50, 50, 50), (90, 50, 20), (100, 100, 100), (1, 1, 1)])
def test_qualities(codec, q):
    check(codec, 272, 32, 32, "gradient", seed=2, q=q)
    check(codec, -272, 32, 24, "noise", seed=2, q=q)


def test_exact_path(codec, oracle):
    """Noise at q100: K1's proof fails for blocks of this frame (asserted on
    the oracle's own Y plane with K1's listing), so the kernel's same-wave
    exact path produces part of this stream."""
    w, h, q = 272, 32, (100, 100, 100)
    data, iyuv, want = case(w, h, 32, "noise", 3, q)
    y = np.frombuffer(iyuv, np.uint8)[: w * h].reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    _, listed, _ = codec.fdct_blocks_listed(y, oracle.qtable(100, 0))
    assert listed.any(), "no unproven block in this input: pick another"
    assert twice(codec, data, w, h, 32, q) == want


def test_device_batch(codec):
    import torch
    import myyuv_hip

    w, h, nf = 272, 32, 3
    for bits in (32, 24):
        cases = [case(w, -h, bits, kind, 4, Q50) for kind in ("noise", "gradient", "flat")]
        dev = torch.device("cuda", 0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        d_bmp = torch.frombuffer(bytearray(b"".join(c[0] for c in cases)), dtype=torch.uint8).to(dev)
        cap = myyuv_hip.payload_bound(w, h)
        assert cap % 4 == 0 and d_bmp.data_ptr() % 16 == 0
        for _ in range(2):
            d_pay = torch.zeros(nf * cap, dtype=torch.uint8, device=dev)
            d_sz = torch.zeros(nf, dtype=torch.int32, device=dev)
            codec.compress_bmp_device(d_bmp.data_ptr(), nf, w, -h, bits, Q50, d_pay.data_ptr(), cap, d_sz.data_ptr(),
                                      stream)
            assert codec.sync_status(stream) == (0, -1)
            sizes = d_sz.cpu().numpy()
            pay = d_pay.cpu().numpy()
            for f, (data, _, want) in enumerate(cases):
                assert int(sizes[f]) == len(want), f
                assert pay[f * cap: f * cap + len(want)].tobytes() == want, f
                assert codec.compress_bmp(data, w, -h, bits, Q50) == want  # the single-frame result
        # argument errors: returned at once, nothing queued
        for args in ((d_bmp.data_ptr() + (4 if bits == 32 else 2), nf), (d_bmp.data_ptr(), 0)):
            with pytest.raises(myyuv_hip.CodecError) as e:
                codec.compress_bmp_device(args[0], args[1], w, -h, bits, Q50, d_pay.data_ptr(), cap, d_sz.data_ptr(), stream)
            assert e.value.code == myyuv_hip.E_ARG
        with pytest.raises(myyuv_hip.CodecError) as e:  # the BMP's own errors come before the alignment's
            codec.compress_bmp_device(d_bmp.data_ptr() + 1, nf, 6, -2, bits, Q50, d_pay.data_ptr(), cap, d_sz.data_ptr(),
                                      stream)
        assert e.value.code == myyuv_hip.E_BMP_INVALID
        assert codec.sync_status(stream) == (0, -1)


def test_context_state(codec, oracle):
    """compress and compress_bmp interleaved on one context, different
    geometries: K1's fix-list parity and the shared workspace survive."""
    rng = np.random.default_rng(5)
    wa, ha = 64, 48
    a = rng.integers(0, 256, wa * ha * 3 // 2, dtype=np.uint8).tobytes()
    qa = (90, 90, 90)  # (noise at q90: K1 lists blocks for its fix kernel)
    want_a = oracle.compress(a, wa, ha, qa)
    data, _, want_b = case(272, 32, 32, "noise", 6, Q50)
    for _ in range(2):
        assert codec.compress(a, wa, ha, qa) == want_a
        assert codec.compress_bmp(data, 272, 32, 32, Q50) == want_b


@pytest.mark.parametrize("w,h,bits,q,code", [
    (6, -2, 32, Q50, 15), (4, -2, 0, Q50, 15), (-4, -2, 32, Q50, 16), (0, 2, 32, Q50, 16), (4, 0, 32, Q50, 16),
    (4, -3, 32, Q50, 17), (4, -2, 16, Q50, 17),
    # bmp_to_iyuv's codes come before compress's
    (6, -2, 32, (0, 50, 50), 15), (-24, -16, 32, (0, 50, 50), 16), (24, -17, 32, (50, 101, 50), 17),
    # then compress's: the quality, then per plane the width before the height
    (24, -16, 32, (0, 50, 50), 2), (16, 16, 24, (50, 50, 101), 2),
    (24, -16, 32, Q50, 3), (24, 24, 24, Q50, 3), (4, -2, 32, Q50, 3), (16, -24, 32, Q50, 4), (-16, 8, 24, Q50, 4),
])
def test_error_codes_and_order(codec, w, h, bits, q, code):
    import myyuv_hip

    data = bytes(abs(w) * abs(h) * 4)
    for _ in range(2):
        with pytest.raises(myyuv_hip.CodecError) as e:
            codec.compress_bmp(data, w, h, bits, q)
        assert e.value.code == code


def test_short_capacity(codec):
    import myyuv_hip

    data, _, want = case(272, 32, 32, "noise", 7, Q50)
    for cap in (16, len(want) - 1):
        out = np.zeros(cap, np.uint8)
        with pytest.raises(myyuv_hip.CodecError) as e:
            codec.compress_bmp_into(np.frombuffer(data, np.uint8), 272, 32, 32, Q50, out)
        assert e.value.code == myyuv_hip.E_CAPACITY and e.value.need == len(want)
        assert not out.any()
    out = np.zeros(len(want), np.uint8)  # exactly enough
    assert codec.compress_bmp_into(np.frombuffer(data, np.uint8), 272, 32, 32, Q50, out) == len(want)
    assert out.tobytes() == want


def test_kernel_stats(codec):
    data, _, want = case(272, 32, 32, "gradient", 8, Q50)
    codec.profile(True)
    try:
        assert codec.compress_bmp(data, 272, 32, 32, Q50) == want
        stats = codec.kernel_stats()
    finally:
        codec.profile(False)
    assert stats["bmp_fdct"][1] == 1 and stats["bmp_fdct"][0] > 0
    assert stats["huff_encode"][1] == 1 and stats["stream_out"][1] == 1
    for k in ("bmp_to_iyuv", "fdct_quant", "fdct_fix", "encode_tile"):  # one launch replaces them
        assert stats[k][1] == 0, k


def test_fused_encoder_context_runs_the_same_kernel(fused_encoder):
    """MYYUV_ENCODER=fused changes nothing here: the call always runs k_bmp_fdct."""
    data, _, want = case(272, 32, 24, "noise", 9, Q50)
    fused_encoder.profile(True)
    try:
        assert fused_encoder.compress_bmp(data, 272, 32, 24, Q50) == want
        stats = fused_encoder.kernel_stats()
    finally:
        fused_encoder.profile(False)
    assert stats["bmp_fdct"][1] == 1 and stats["encode_tile"][1] == 0


def test_cli_compress_from_bmp(tmp_path, golden):
    """in.bmp -compress DCT 50: the file of -to_yuv IYUV followed by -compress
    DCT 50, header included."""
    def cli(*args):
        r = subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
        return r

    bmp = tmp_path / "chef.bmp"
    with gzip.open(os.path.join(GOLDEN, "chef-with-trumpet.bmp.gz"), "rb") as f:
        bmp.write_bytes(f.read())
    one, raw, two = tmp_path / "one.myyuv", tmp_path / "raw.myyuv", tmp_path / "two.myyuv"
    r = cli(bmp, "-compress", "DCT", 50, "-o", one)
    assert r.stdout.splitlines()[0].startswith("BMP DCT compression ( 50 ) : ")
    cli(bmp, "-to_yuv", "IYUV", "-o", raw)
    cli(raw, "-compress", "DCT", 50, "-o", two)
    assert one.read_bytes() == two.read_bytes()
    import myyuv_file
    assert myyuv_file.YUVFile.load(str(one)).data == golden("chef-with-trumpet-DCT-50.myyuv").data
    three = tmp_path / "three.myyuv"
    cli(bmp, "-compress", "DCT", 90, 50, "-o", three)
    four = tmp_path / "four.myyuv"
    cli(raw, "-compress", "DCT", 90, 50, "-o", four)
    assert three.read_bytes() == four.read_bytes()

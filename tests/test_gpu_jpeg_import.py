"""Import from JPEG on the GPU (k_jpeg_import and k_jpeg_import_coef,
csrc/k_jpeg_import.hip): every stream is compared byte for byte with what the
oracle's Huffman encoder writes for the coefficients the independent Python
parser / writer (jpegimportref) holds, twice on one context.  Files are small:
one MCU, 48x32, 144x128 with a restart per MCU (72 intervals: a second wave
with a partial lane set), non-interleaved files whose intervals end short,
whose RSTm wraps past 7 and whose Ri changes per scan, a picture whose last MCU
column and row are half empty; files below 64 intervals take the host decode
and k_jpeg_import_coef."""
import glob
import os
import subprocess

import numpy as np
import pytest

import jpegimportcases as C
import jpegimportref as JI
import regionref as R
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
GOLD = sorted(glob.glob(os.path.join(GOLDEN, "jpeg_import", "*.jpg")))


def first_difference(a, b):
    n = min(len(a), len(b))
    x, y = np.frombuffer(a[:n], np.uint8), np.frombuffer(b[:n], np.uint8)
    d = np.nonzero(x != y)[0]
    return (len(a), len(b), int(d[0]) if len(d) else None, len(d))


def error_of(fn, *args):
    import myyuv_hip

    with pytest.raises(myyuv_hip.CodecError) as e:
        fn(*args)
    return e.value.code, e.value.bad_block


def check(codec, data, want, Wp, Hp, q_out, q=None):
    for rep in range(2):
        got, w, h, qs = codec.from_jpeg(data, q)
        assert (w, h, qs) == (Wp, Hp, tuple(q_out)), (rep, w, h, qs)
        assert got == want, (rep, first_difference(got, want))


# ------------------------------------------------------------------ round trip
@pytest.mark.parametrize("w,h", [(16, 16), (48, 32), (512, 512)])
@pytest.mark.parametrize("q", [(10, 10, 10), (50, 50, 50), (90, 90, 90), (100, 100, 100), (90, 50, 30), (50, 2, 3)])
def test_import_of_an_export_is_the_stream(codec, oracle, w, h, q):
    """import(export(s)) == s for encoder-written streams, with the qualities
    the export was given (1 for a chroma quality of 1..3).  512x512 has 96
    intervals of 64 blocks (the segment path, non-interleaved, RSTm wrapping);
    the small frames take the coefficient-image path."""
    import myyuv_hip

    s = R.tiled_stream(w, h, q)[0]
    f = codec.to_jpeg(s, w, h, q)
    info = myyuv_hip.jpeg_inspect(f)
    assert info["on_gpu"] == (w == 512) and info["scans"] == 3
    check(codec, f, s, w, h, tuple(1 if p and v <= 3 else v for p, v in enumerate(q)))


# ---------------------------------------------------------------- golden files
@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_golden_file_gives_the_reference_parsers_stream(codec, oracle, path):
    import myyuv_hip

    data = open(path, "rb").read()
    P = JI.parse(data)
    keep = tuple(JI.keep_quality(P.qt[p], p != 0) for p in range(3))
    if all(keep):
        check(codec, data, JI.stream(P.planes), P.Wp, P.Hp, keep)
    else:
        assert error_of(codec.from_jpeg, data) == (myyuv_hip.E_JPEG_TABLES, -1)
    q = (60, 70, 80)
    check(codec, data, JI.stream(JI.rescaled(P.planes, P.qt, q)), P.Wp, P.Hp, q, q)


# --------------------------------------------------------------- crafted files
@pytest.mark.parametrize("name", [n for n in C.good_cases() if n != "144x128_own_tables"])
def test_crafted_file_gives_its_planes_stream(codec, oracle, name):
    import myyuv_hip

    c = C.good_cases()[name]
    assert myyuv_hip.jpeg_inspect(c.data)["on_gpu"] == (c.segments >= 64)
    q = tuple(JI.keep_quality(c.qt[p], p != 0) for p in range(3))
    check(codec, c.data, JI.stream(c.planes), c.Wp, c.Hp, q)


def test_both_paths_give_the_same_stream(codec, oracle):
    """The same planes with a restart per MCU (k_jpeg_import) and without any
    (the host decode and k_jpeg_import_coef), interleaved and not."""
    import myyuv_hip

    W, H, q = 144, 128, (50, 50, 50)
    planes = C.picture_planes(W, H, 21)
    want = JI.stream(planes)
    for il in (True, False):
        a = JI.write(planes, W, H, C.qtables(q), interleaved=il, ri=1)
        b = JI.write(planes, W, H, C.qtables(q), interleaved=il, ri=0)
        assert [myyuv_hip.jpeg_inspect(x)["on_gpu"] for x in (a, b)] == [True, False]
        check(codec, a, want, W, H, q)
        check(codec, b, want, W, H, q)


# ------------------------------------------------------- a destination quality
def test_a_destination_quality_is_a_requantise_of_the_kept_import(codec, oracle):
    for name in ("144x128_picture", "272x16_planar_ri123"):
        c = C.good_cases()[name]
        keep = tuple(JI.keep_quality(c.qt[p], p != 0) for p in range(3))
        kept = codec.from_jpeg(c.data)[0]
        for q in ((30, 30, 30), (95, keep[1], 20)):
            want = codec.requantize(kept, c.Wp, c.Hp, keep, q)
            assert want == JI.stream(JI.rescaled(c.planes, c.qt, q))
            check(codec, c.data, want, c.Wp, c.Hp, q, q)


def test_tables_that_are_no_qualitys_need_a_quality(codec, oracle):
    import myyuv_hip

    c = C.good_cases()["144x128_own_tables"]
    assert error_of(codec.from_jpeg, c.data) == (myyuv_hip.E_JPEG_TABLES, -1)
    assert error_of(codec.from_jpeg, c.data, (50, 0, 50)) == (myyuv_hip.E_QUALITY, -1)
    q = (50, 60, 100)
    check(codec, c.data, JI.stream(JI.rescaled(c.planes, c.qt, q)), c.Wp, c.Hp, q, q)


# --------------------------------------------------------------- refused files
def test_refused_files_give_their_codes(codec):
    for name, data, code in C.error_cases()[::5]:
        assert error_of(codec.from_jpeg, data) == (code, -1), name


@pytest.mark.parametrize("name", list(C.data_cases()))
def test_damaged_data_reports_the_lowest_block_and_the_context_goes_on(codec, oracle, name):
    """Decode errors are handled in the kernel by bounds and flags: the call
    returns with the block, and the next call on the context is correct."""
    import myyuv_hip

    c = C.data_cases()[name]
    assert myyuv_hip.jpeg_inspect(c.data)["on_gpu"]
    assert error_of(codec.from_jpeg, c.data) == (myyuv_hip.E_JPEG_DATA, c.bad)
    good = C.good_cases()["144x128_picture"]
    check(codec, good.data, JI.stream(good.planes), good.Wp, good.Hp, (90, 90, 90))


def test_damaged_data_below_the_threshold(codec, oracle):
    import myyuv_hip

    W, H = 48, 32
    planes = C.picture_planes(W, H, 8)
    data = JI.write(planes, W, H, C.qtables((50, 50, 50)), raw={(0, 7): [(0, 2), (0xFFFF, 16)]})
    assert not myyuv_hip.jpeg_inspect(data)["on_gpu"]
    assert error_of(codec.from_jpeg, data) == (myyuv_hip.E_JPEG_DATA, 7)


# ------------------------------------------------------------------ device form
def test_device_form_agrees_and_rejects_a_file_without_restarts(codec, oracle):
    import myyuv_hip
    import torch

    stream = torch.cuda.current_stream().cuda_stream
    for name in ("144x128_picture", "200x40_planar_ri1"):
        c = C.good_cases()[name]
        want, _, _, keep = codec.from_jpeg(c.data)
        assert want == JI.stream(c.planes)
        pad = bytes(c.data) + bytes(-len(c.data) % 4)
        d_file = torch.frombuffer(bytearray(pad), dtype=torch.uint8).cuda()
        cap = len(want) + 64
        d_out = torch.full((cap + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        d_size = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        for rep in range(2):
            got = codec.from_jpeg_device(d_file.data_ptr(), c.data, d_out.data_ptr(), cap, d_size.data_ptr(),
                                         None, stream)
            assert got == (c.Wp, c.Hp, keep)
            assert codec.sync_status(stream) == (0, -1)
            out = bytes(d_out.cpu().numpy())
            assert d_size.cpu().tolist() == [len(want)] and out[:len(want)] == want
            assert out[cap:] == b"\x5A" * 256
        # a stream larger than cap: reported, nothing past cap written
        d_out.fill_(0x5A)
        codec.from_jpeg_device(d_file.data_ptr(), c.data, d_out.data_ptr(), len(want) - 4, d_size.data_ptr(), None,
                               stream)
        assert codec.sync_status(stream)[0] == myyuv_hip.E_CAPACITY
        assert bytes(d_out.cpu().numpy())[len(want) - 4:] == b"\x5A" * (cap + 256 - len(want) + 4)
    bad = C.data_cases()["no_code_mcu31"]
    d_file = torch.frombuffer(bytearray(bytes(bad.data) + bytes(-len(bad.data) % 4)), dtype=torch.uint8).cuda()
    d_out = torch.zeros(myyuv_hip.payload_bound(bad.Wp, bad.Hp), dtype=torch.uint8, device="cuda")
    codec.from_jpeg_device(d_file.data_ptr(), bad.data, d_out.data_ptr(), d_out.numel(), d_size.data_ptr(), None,
                           stream)
    assert codec.sync_status(stream) == (myyuv_hip.E_JPEG_DATA, bad.bad)
    small = C.good_cases()["48x32_ri2"]
    assert error_of(codec.from_jpeg_device, d_file.data_ptr(), small.data, d_out.data_ptr(), d_out.numel(),
                    d_size.data_ptr(), None, stream)[0] == myyuv_hip.E_JPEG_UNSUPPORTED
    assert error_of(codec.from_jpeg_device, d_file.data_ptr() + 1, bad.data, d_out.data_ptr(), d_out.numel(),
                    d_size.data_ptr(), None, stream)[0] == myyuv_hip.E_ARG
    assert codec.sync_status(stream) == (0, -1)


# --------------------------------------------------------------------- capacity
def test_capacity_is_honoured(codec, oracle):
    import myyuv_hip

    for name in ("144x128_picture", "48x32_ri2"):
        c = C.good_cases()[name]
        want = JI.stream(c.planes)
        src = np.frombuffer(c.data, np.uint8).copy()
        out = np.full(len(want) + 100, 0x5A, np.uint8)
        with pytest.raises(myyuv_hip.CodecError) as e:
            codec.from_jpeg_into(src, out[:len(want) - 1])
        assert (e.value.code, e.value.size) == (myyuv_hip.E_CAPACITY, len(want))
        assert (out == 0x5A).all()
        n = codec.from_jpeg_into(src, out[:len(want)])[0]
        assert n == len(want) and out[:n].tobytes() == want and (out[n:] == 0x5A).all()


# ----------------------------------------------------------------- kernel stats
def test_kernel_stats_name_the_import_kernels(codec, oracle):
    big, small = C.good_cases()["144x128_picture"], C.good_cases()["48x32_ri2"]
    codec.profile(True, ["jpeg_import", "jpeg_import_coef", "requant", "huff_encode", "fdct_quant"])
    try:
        codec.from_jpeg(big.data)
        codec.from_jpeg(small.data)
        codec.from_jpeg(small.data, (40, 40, 40))
        stats = codec.kernel_stats()
    finally:
        codec.profile(False)
    assert stats["jpeg_import"][1] == 1 and stats["jpeg_import"][0] > 0
    assert stats["jpeg_import_coef"][1] == 2 and stats["huff_encode"][1] == 3
    assert stats["requant"][1] == 0 and stats["fdct_quant"][1] == 0


# -------------------------------------------------------------------------- CLI
def test_cli_from_jpeg(tmp_path, oracle):
    import myyuv_file

    path = os.path.join(GOLDEN, "jpeg_import", "odd.jpg")
    P = JI.parse(open(path, "rb").read())
    out = tmp_path / "odd.myyuv"
    r = subprocess.run([CLI, path, "-from_jpeg", "-q", "50", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Success!", r.stdout + r.stderr
    assert "37x21 padded to 48x32" in r.stdout
    f = myyuv_file.YUVFile.load(str(out))
    assert (f.width, f.height, tuple(f.params)) == (48, 32, (50, 50, 50))
    assert f.data == JI.stream(JI.rescaled(P.planes, P.qt, (50, 50, 50)))
    path = os.path.join(GOLDEN, "jpeg_import", "qt90.jpg")
    P = JI.parse(open(path, "rb").read())
    r = subprocess.run([CLI, path, "-from_jpeg", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "padded" not in r.stdout, r.stdout + r.stderr
    f = myyuv_file.YUVFile.load(str(out))
    assert (f.width, f.height, tuple(f.params)) == (64, 48, (90, 90, 90)) and f.data == JI.stream(P.planes)

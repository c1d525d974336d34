"""Import from JPEG, the parts that need no GPU: the marker parser and block
decoder of csrc/jpeg_import.h (the code k_jpeg_import and the library's host
decode run) compiled for the host (tools/jpeg_import_host.cpp) against the
independent Python parser and writer (jpegimportref) on the golden files that
Pillow wrote and on crafted files; every UNSUPPORTED / SYNTAX / DATA rule with
its code (and block); myyuv_jpeg_inspect; the same program under the address
and undefined-behaviour sanitizers over the malformed files; the imported
picture against libjpeg's decode; the argument errors of the C ABI and the CLI
that come before any device is touched."""
import ctypes
import glob
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import jpegimportcases as C
import jpegimportref as JI
from conftest import GOLDEN, PKG, ROOT

SRC = os.path.join(ROOT, "tools", "jpeg_import_host.cpp")
CLI = os.path.join(PKG, "myyuv_cli")
GOLD = sorted(glob.glob(os.path.join(GOLDEN, "jpeg_import", "*.jpg")))
GOLD_NAMES = ["default", "odd", "optimize", "qt50", "qt90", "rst_blocks", "rst_rows"]


def _build(tmp_path_factory, name, *flags):
    exe = str(tmp_path_factory.mktemp("jpegin") / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(PKG, "csrc"), SRC,
                    "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build(tmp_path_factory, "jpeg_import_host")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "jpeg_import_host_san", "-fsanitize=address,undefined",
                  "-fno-sanitize-recover=all")


class Out:
    pass


def run(exe, data):
    r = subprocess.run([exe], input=bytes(data), capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-3000:])
    o = Out()
    o.rc = struct.unpack_from("<i", r.stdout, 0)[0]
    if o.rc:
        assert len(r.stdout) == 4
        return o
    (o.W, o.H, o.Wp, o.Hp, o.scans, o.segments, r0, r1, r2, il) = struct.unpack_from("<10I", r.stdout, 4)
    o.ri, o.interleaved = [r0, r1, r2][:o.scans], bool(il)
    pos = 44
    o.qt = np.frombuffer(r.stdout, np.uint8, 192, pos).reshape(3, 64).astype(int)
    pos += 192
    o.segs = np.frombuffer(r.stdout, "<u4", 5 * o.segments, pos).reshape(-1, 5)
    pos += 20 * o.segments
    o.drc, o.bad = struct.unpack_from("<iq", r.stdout, pos)
    pos += 12
    img = np.frombuffer(r.stdout, "<i2", -1, pos).reshape(-1, 64)
    ny, nc = (o.Wp // 8) * (o.Hp // 8), (o.Wp // 16) * (o.Hp // 16)
    assert len(img) == ny + 2 * nc
    o.planes = [img[:ny], img[ny:ny + nc], img[ny + nc:]]
    return o


def same_planes(got, want):
    return all(np.asarray(g).shape == np.asarray(w).shape and (np.asarray(g) == np.asarray(w)).all()
               for g, w in zip(got, want))


# ------------------------------------------------------------ the golden files
def test_the_golden_files_are_all_there():
    assert [os.path.basename(p)[:-4] for p in GOLD] == GOLD_NAMES


@pytest.mark.parametrize("path", GOLD, ids=GOLD_NAMES)
def test_host_decode_of_a_golden_file_equals_the_reference_parser(harness, path):
    data = open(path, "rb").read()
    P = JI.parse(data)
    o = run(harness, data)
    assert (o.rc, o.drc, o.bad) == (0, 0, -1)
    assert (o.W, o.H, o.Wp, o.Hp) == (P.W, P.H, P.Wp, P.Hp)
    assert (o.interleaved, o.ri, o.segments) == (P.interleaved, P.ri, P.segments)
    assert all((o.qt[p] == P.qt[p]).all() for p in range(3))
    assert same_planes(o.planes, P.planes)
    assert any((pl != 0).any() for pl in P.planes)


def test_golden_layouts():
    seen = {}
    for path, name in zip(GOLD, GOLD_NAMES):
        P = JI.parse(open(path, "rb").read())
        seen[name] = (P.W, P.H, P.Wp, P.Hp, P.segments, P.ri)
    assert seen["odd"][:4] == (37, 21, 48, 32)
    assert seen["rst_blocks"][4:] == (72, [1]) and seen["qt50"][4:] == (72, [1])
    assert seen["rst_rows"][4:] == (3, [4]) and seen["default"][4:] == (1, [0])
    dht = {n: JI.J.dht_segments(open(p, "rb").read()) for p, n in zip(GOLD, GOLD_NAMES)}
    assert dht["optimize"] != dht["default"]  # the file's own Huffman tables
    assert all(dht["default"][k] == (list(b), list(v)) for k, (b, v) in JI.DEFAULT_DHT.items())


# ------------------------------------------------------------ crafted files
@pytest.mark.parametrize("name", list(C.good_cases()))
def test_host_decode_of_a_crafted_file_is_its_planes(harness, oracle, name):
    c = C.good_cases()[name]
    o = run(harness, c.data)
    assert (o.rc, o.drc, o.bad) == (0, 0, -1)
    assert (o.W, o.H, o.Wp, o.Hp, o.segments, o.interleaved) == (c.W, c.H, c.Wp, c.Hp, c.segments, c.interleaved)
    assert same_planes(o.planes, c.planes)
    assert all((o.qt[p] == np.asarray(c.qt[p]).reshape(64)).all() for p in range(3))
    P = JI.parse(c.data)  # the writer and the independent parser agree
    assert same_planes(P.planes, c.planes) and P.segments == c.segments
    # every interval's bytes lie inside the file, in file order, and cover each scan's MCUs once
    end = 0
    for off, length, mcu0, nmcu, scan in o.segs:
        assert end <= off and off + length <= len(c.data) and nmcu > 0
        end = off + length
    for s in range(o.scans):
        rows = o.segs[o.segs[:, 4] == s]
        assert (rows[1:, 2] == rows[:-1, 2] + rows[:-1, 3]).all() and rows[0, 2] == 0


def test_crafted_content_reaches_the_decoders_branches():
    c = C.good_cases()["144x128_ri1"]
    zz = np.concatenate(c.planes)[:, JI.ZZ]
    assert (zz[:, 63] != 0).any()  # no EOB
    run_len = lambda b: np.diff(np.flatnonzero(np.concatenate([[1], b[1:] != 0]))).max(initial=0)  # noqa: E731
    assert max(run_len(b) for b in zz) >= 48  # three ZRLs in a row
    assert np.abs(np.diff(np.concatenate(c.planes[:1])[:, 0].astype(int))).max() >= 1024  # DC category 11
    assert c.data.count(b"\xff\x00") >= 10  # 0xFF in the entropy data
    assert c.data.count(b"\xff\xff\xff\xff\xd0") >= 1  # fill bytes before RSTm
    assert c.data.count(b"\xff\xc4") == 1 and c.data.count(b"\xff\xdb") == 1  # several tables per segment
    codes = JI.J.codes(*map(list, JI.DEFAULT_DHT[0x10]))
    used = (np.abs(zz[:, 17]) >= 512) & (zz[:, 2:17] == 0).all(1) & (zz[:, 1] != 0)  # run 15, size 10
    assert codes[0xFA][1] == 16 and used.any()  # a 16-bit code is used
    assert len(set(C.good_cases()["272x16_planar_ri123"].data.split(b"\xff\xdd")[1:])) == 3  # Ri changes per scan


def test_stream_of_crafted_planes_decodes_to_their_picture(oracle):
    """The stream an import must return (the oracle's Huffman encoder over the
    planes) holds exactly those coefficients."""
    import scaleref as S

    c = C.good_cases()["48x32_ri2"]
    pay = JI.stream(c.planes)
    assert same_planes(S.coefficients(pay), c.planes)


# ------------------------------------------------------------ refused files
@pytest.mark.parametrize("name", [n for n, _, _ in C.error_cases() if not n.startswith("truncated")])
def test_refused_file_gives_its_code(harness, name):
    data, code = next((d, c) for n, d, c in C.error_cases() if n == name)
    assert run(harness, data).rc == code


def test_truncation_at_every_marker_boundary_is_a_syntax_error(harness):
    cases = [(n, d) for n, d, _ in C.error_cases() if n.startswith("truncated")]
    assert len(cases) > 80
    for name, data in cases:
        assert run(harness, data).rc == C.E_SYNTAX, name


@pytest.mark.parametrize("name", list(C.data_cases()))
def test_damaged_data_gives_the_block_and_loses_the_rest_of_the_interval(harness, name):
    c = C.data_cases()[name]
    o = run(harness, c.data)
    assert (o.rc, o.drc, o.bad) == (0, C.E_DATA, c.bad)
    assert same_planes(o.planes, c.planes)


def test_sanitized_program_over_every_malformed_file(sanitized):
    """The stand-alone program built with -fsanitize=address,undefined (its
    file in an exact-size heap buffer) reads no byte outside any malformed file
    and gives the same answers."""
    for name, data, code in C.error_cases():
        assert run(sanitized, data).rc == code, name
    for name, c in C.data_cases().items():
        o = run(sanitized, c.data)
        assert (o.drc, o.bad) == (C.E_DATA, c.bad), name
    for c in C.good_cases().values():
        assert run(sanitized, c.data).drc == 0
    for path in GOLD:
        data = open(path, "rb").read()
        assert run(sanitized, data).drc == 0
        for cut in range(0, len(data), 7):  # any truncation: an answer, never a fault
            assert run(sanitized, data[:cut]).rc in (C.E_SYNTAX, C.E_UNSUPPORTED)
    rng = np.random.default_rng(1)
    base = bytearray(C.good_cases()["48x32_ri2"].data)
    for _ in range(200):  # random damage anywhere
        d = bytearray(base)
        for i in rng.integers(2, len(d), 3):
            d[i] = int(rng.integers(0, 256))
        run(sanitized, bytes(d))


# ------------------------------------------------------------ myyuv_jpeg_inspect
def test_inspect_reports_sizes_layout_and_keep_qualities(oracle):
    import myyuv_hip

    for path, name in zip(GOLD, GOLD_NAMES):
        data = open(path, "rb").read()
        P = JI.parse(data)
        info = myyuv_hip.jpeg_inspect(data)
        assert (info["width"], info["height"], info["padded_width"], info["padded_height"]) == (P.W, P.H, P.Wp, P.Hp)
        assert (info["scans"], info["restart_interval"], info["segments"]) == (1, P.ri, P.segments)
        assert info["keep_quality"] == tuple(JI.keep_quality(P.qt[p], p != 0) for p in range(3))
        assert info["on_gpu"] == (P.segments >= 64 and all(P.ri))
        assert info["payload_bound"] == myyuv_hip.payload_bound(P.Wp, P.Hp)
    assert myyuv_hip.jpeg_inspect(open(GOLD[GOLD_NAMES.index("qt50")], "rb").read())["keep_quality"] == (50, 50, 50)
    assert myyuv_hip.jpeg_inspect(open(GOLD[GOLD_NAMES.index("qt90")], "rb").read())["keep_quality"] == (90, 90, 90)
    own = myyuv_hip.jpeg_inspect(C.good_cases()["144x128_own_tables"].data)
    assert own["keep_quality"] == (0, 0, 0) and own["on_gpu"]
    c = C.good_cases()["272x16_planar_ri123"]
    info = myyuv_hip.jpeg_inspect(c.data)
    assert (info["scans"], info["restart_interval"], info["segments"]) == (3, [1, 2, 3], c.segments)
    # chroma qualities 1..3 share one table: the smallest is taken
    low = C._case(16, 16, C.crafted_planes(16, 16), q=(3, 3, 2))
    assert myyuv_hip.jpeg_inspect(low.data)["keep_quality"] == (3, 1, 1)
    for name, data, code in C.error_cases()[::7]:
        with pytest.raises(myyuv_hip.CodecError) as e:
            myyuv_hip.jpeg_inspect(data)
        assert e.value.code == code, name


def test_keep_quality_map_is_as_the_header_says(oracle):
    luma = {np.asarray(oracle.qtable(q, False)).tobytes() for q in range(1, 101)}
    assert len(luma) == 100  # injective
    chroma = [np.asarray(oracle.qtable(q, True)).tobytes() for q in range(1, 101)]
    assert len(set(chroma)) == 98 and chroma[0] == chroma[1] == chroma[2]
    assert (np.asarray(oracle.qtable(1, True)) == 255).all()


# ------------------------------------------------------------------- libjpeg
@pytest.mark.parametrize("name", ["qt50", "qt90"])
def test_imported_luma_is_within_1_of_libjpegs_decode(harness, oracle, name):
    """The file imported with its tables kept, decoded by the oracle, against
    Pillow's decode of the same file: libjpeg's integer inverse transform
    against the fp32 one, the bound the export's test holds for the reverse
    direction."""
    Image = pytest.importorskip("PIL.Image")
    data = open(GOLD[GOLD_NAMES.index(name)], "rb").read()
    o = run(harness, data)
    q = tuple(JI.keep_quality(o.qt[p], p != 0) for p in range(3))
    assert q == ((50,) * 3 if name == "qt50" else (90,) * 3)
    dec = oracle.decompress(JI.stream(o.planes), o.Wp, o.Hp, q)
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", (o.W, o.H))
    assert im.mode == "YCbCr" and im.size == (o.W, o.H)
    px = np.asarray(im).astype(int)
    y = np.frombuffer(dec, np.uint8)[:o.Wp * o.Hp].reshape(o.Hp, o.Wp)[:o.H, :o.W].astype(int)
    d = np.abs(px[:, :, 0] - y)
    print(f"{name}: luma max |diff| {d.max()}, differing {np.count_nonzero(d) / d.size:.4f}")
    assert d.max() <= 1


# ---------------------------------------- argument errors that need no device
def test_handle_and_pointer_errors_need_no_device():
    import myyuv_hip

    L = myyuv_hip.load()
    data = np.frombuffer(open(GOLD[0], "rb").read(), np.uint8).copy()
    out = np.zeros(64, np.uint8)
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    size, w, h = ctypes.c_uint32(9), ctypes.c_uint32(8), ctypes.c_uint32(7)
    qs = np.zeros(3, np.uint8)
    bad = ctypes.c_int64(7)
    assert L.myyuv_gpu_jpeg_to_dct(None, u8(data), data.nbytes, None, u8(out), 64, ctypes.byref(size),
                                   ctypes.byref(w), ctypes.byref(h), u8(qs), ctypes.byref(bad)) == myyuv_hip.E_ARG
    assert (bad.value, size.value, w.value, h.value) == (-1, 9, 8, 7) and not (out != 0).any()
    assert L.myyuv_gpu_jpeg_to_dct_device(None, 256, u8(data), data.nbytes, None, 1024, 64, 2048, ctypes.byref(w),
                                          ctypes.byref(h), u8(qs), None) == myyuv_hip.E_ARG
    assert L.myyuv_jpeg_inspect(None, 0, None) == myyuv_hip.E_ARG
    for name in ("myyuv_jpeg_inspect", "myyuv_gpu_jpeg_to_dct", "myyuv_gpu_jpeg_to_dct_device"):
        assert name in myyuv_hip.EXPORTS and getattr(L, name)
    assert (myyuv_hip.K_JPEG_IMPORT, myyuv_hip.K_JPEG_IMPORT_COEF, myyuv_hip.K_CEIL) == (27, 28, 29)
    assert myyuv_hip.KERNELS_CEIL[:27] == myyuv_hip.KERNELS_MAX
    assert myyuv_hip.KERNELS_CEIL[27:] == ["jpeg_import", "jpeg_import_coef"]
    assert (myyuv_hip.E_JPEG_UNSUPPORTED, myyuv_hip.E_JPEG_SYNTAX, myyuv_hip.E_JPEG_DATA,
            myyuv_hip.E_JPEG_TABLES) == (21, 22, 23, 24)
    assert myyuv_hip.error_message(21) == "JPEG file is not a baseline 4:2:0 picture the container can hold"
    assert myyuv_hip.error_message(22) == "JPEG file is damaged"
    assert myyuv_hip.error_message(23) == "JPEG entropy data is damaged"
    assert myyuv_hip.error_message(24) == "the file's tables are not the codec's: name a quality"
    assert myyuv_hip.JPEG_SEGMENTS_MIN == 64


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def test_cli_from_jpeg_argument_errors(tmp_path):
    out = str(tmp_path / "x.myyuv")
    jpg = GOLD[0]
    for tail in ([], ["-o"], ["-o", out, "extra"], ["50", "-o", out]):
        r = cli(jpg, "-from_jpeg", *tail)
        assert r.returncode == 1 and "Usage" in r.stdout, (tail, r.stdout)
        assert r.stdout.splitlines()[0] == "Invalid argument, last arguments must be `-o /path/to/new_image.myyuv`"
    for params, msg in ((["0"], "must range between [1..100]"), (["101"], "must range between [1..100]"),
                        (["50", "50", "50", "50"], "Too many compression parameters"),
                        ([], "Too few compression parameters")):
        r = cli(jpg, "-from_jpeg", "-q", *params, "-o", out)
        assert r.returncode != 0 and msg in r.stderr, (params, r.returncode, r.stderr)
    bad = tmp_path / "bad.jpg"
    bad.write_bytes(open(jpg, "rb").read()[:100])
    r = cli(str(bad), "-from_jpeg", "-o", out)
    assert r.returncode != 0 and "JPEG file is damaged" in r.stderr
    assert not os.path.exists(out)
    assert "-from_jpeg [-q Q [Q [Q]]] -o OUT.myyuv" in cli(jpg, "-from_jpeg").stdout

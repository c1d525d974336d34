"""Encode to a target on the GPU (include/myyuv_hip.h): the quality, the probe
count and the `at` record equal ratesearchref's search driven by the oracle's
tables, and the payload is oracle.compress at the chosen qualities, byte for
byte.  Frames: 16x16 (sizes and errors not monotone in the quality) and 208x96
tiled, 208x96 noise; budgets and ceilings are those of
tests/test_rate_search_host.py."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import metricref as M
import ratesearchref as S
import regionref as R
import synth
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

CLI = os.path.join(PKG, "myyuv_cli")
RAW = os.path.join(GOLDEN, "chef-with-trumpet.myyuv")
C50 = os.path.join(GOLDEN, "chef-with-trumpet-DCT-50.myyuv")
FRAMES = ["tiled_16x16", "tiled_208x96", "noise_208x96"]


@functools.lru_cache(maxsize=None)
def frame(name):
    f = R.chef()
    if name == "tiled_16x16":
        return synth.tiled_frame(f.data, f.width, f.height, 16, 16, 400, 300).tobytes(), 16, 16
    if name == "tiled_208x96":
        return synth.tiled_frame(f.data, f.width, f.height, 208, 96, 400, 300).tobytes(), 208, 96
    if name == "noise_208x96":
        return synth.noise_frame(208, 96, 77).tobytes(), 208, 96
    if name == "tiled_1040x512":
        return synth.tiled_frame(f.data, f.width, f.height, 1040, 512, 400, 300).tobytes(), 1040, 512
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def tables(name):
    from oracle import oracle as O

    src, w, h = frame(name)
    return S.oracle_tables(O, src, w, h)


@functools.lru_cache(maxsize=None)
def at_record(name, q3):
    """The probe record of the frame at the triple q3: (plane sizes, payload
    bytes, metricref's records), and the oracle's payload."""
    from oracle import oracle as O

    src, w, h = frame(name)
    pay = O.compress(src, w, h, q3)
    recs, _ = M.frame_metric(src, O.decompress(pay, w, h, q3), w, h)
    return (struct.unpack("<III", pay[:12]), len(pay), recs), pay


def error_of(fn, *args):
    import myyuv_hip

    with pytest.raises(myyuv_hip.CodecError) as e:
        fn(*args)
    return e.value


def check_size(codec, name, budget):
    import myyuv_hip

    src, w, h = frame(name)
    sizes, _ = tables(name)
    ok, q, asked = S.size_search(lambda k: sizes[k - 1], budget)
    at, pay = at_record(name, (q, q, q))
    want = {"quality": (q, q, q), "failed_planes": 0, "probes": len(asked), "at": at}
    if ok:
        got_pay, res = codec.compress_to_size(src, w, h, budget)
        assert res == want, (name, budget, res, want)
        assert got_pay == pay and len(pay) <= budget
    else:
        e = error_of(codec.compress_to_size, src, w, h, budget)
        assert e.code == myyuv_hip.E_TARGET and e.result == want, (name, budget, e.result, want)
        assert q == 1 and len(asked) == 2 and str(e) == "target not reachable"
    return ok


def check_sse(codec, name, ceilings):
    import myyuv_hip

    src, w, h = frame(name)
    _, sses = tables(name)
    ok, q3, failed, asked = S.sse_search(lambda k: tuple(sses[k[p] - 1][p] for p in range(3)), ceilings)
    at, pay = at_record(name, q3)
    want = {"quality": q3, "failed_planes": failed, "probes": len(asked), "at": at}
    if ok:
        got_pay, res = codec.compress_to_sse(src, w, h, ceilings)
        assert res == want, (name, ceilings, res, want)
        assert got_pay == pay
        assert all(at[2][p][0] <= ceilings[p] for p in range(3))
    else:
        e = error_of(codec.compress_to_sse, src, w, h, ceilings)
        assert e.code == myyuv_hip.E_TARGET and e.result == want, (name, ceilings, e.result, want)
        assert q3 == (100, 100, 100) and failed != 0
    return ok


@pytest.mark.parametrize("name", FRAMES)
def test_size_targets(codec, oracle, name):
    sizes, _ = tables(name)
    outcomes = [check_size(codec, name, b) for b in S.size_budgets(sizes)]
    assert not all(outcomes) and any(outcomes)
    if name == "tiled_16x16":  # every size the frame can have, as a budget
        for b in sorted(set(sizes)):
            assert check_size(codec, name, b)


@pytest.mark.parametrize("name", FRAMES)
def test_sse_targets(codec, oracle, name):
    _, sses = tables(name)
    outcomes = [check_sse(codec, name, t) for t in S.sse_ceilings(sses)]
    assert not all(outcomes) and any(outcomes)


@pytest.mark.parametrize("name", FRAMES)
def test_psnr_targets(codec, oracle, name):
    import myyuv_hip

    src, w, h = frame(name)
    _, sses = tables(name)
    n = (w * h, w * h // 4, w * h // 4)
    mono = all(a[p] >= b[p] for a, b in zip(sses, sses[1:]) for p in range(3))
    assert mono == (name != "tiled_16x16")
    for db in (20, 30, 35, 40, 50):
        ceil = tuple(S.sse_for_psnr(db, n[p]) for p in range(3))
        assert ceil == tuple(myyuv_hip.metric_sse_for_psnr(db, n[p]) for p in range(3))
        if any(sses[99][p] > ceil[p] for p in range(3)):
            e = error_of(codec.compress_to_psnr, src, w, h, db)
            assert e.code == myyuv_hip.E_TARGET and e.result["quality"] == (100, 100, 100)
            assert e.result["failed_planes"] == sum(1 << p for p in range(3) if sses[99][p] > ceil[p])
            continue
        pay, res = codec.compress_to_psnr(src, w, h, db)
        assert check_sse(codec, name, ceil) and res["at"] == at_record(name, res["quality"])[0]
        assert pay == at_record(name, res["quality"])[1]
        for p in range(3):
            q = res["quality"][p]
            assert M.psnr(res["at"][2][p][0], n[p]) >= db
            if mono and q > 1:
                assert M.psnr(sses[q - 2][p], n[p]) < db, (name, db, p, q)
    e = error_of(codec.compress_to_psnr, src, w, h, float("nan"))
    assert e.code == myyuv_hip.E_ARG


def test_target_failures_leave_the_output_alone(codec, oracle):
    import ctypes

    import myyuv_hip

    name = "tiled_208x96"
    src, w, h = frame(name)
    sizes, sses = tables(name)
    L = myyuv_hip.load()
    a = np.frombuffer(src, np.uint8)
    u8 = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    out = np.full(myyuv_hip.payload_bound(w, h), 0x5A, np.uint8)
    size = ctypes.c_uint32(0xDEADBEEF)
    res = myyuv_hip.TargetResult()
    rc = L.myyuv_gpu_dct_compress_to_size(codec._h, u8(a), w, h, sizes[0] - 1, u8(out), out.size, ctypes.byref(size),
                                          ctypes.byref(res))
    assert rc == myyuv_hip.E_TARGET and size.value == 0xDEADBEEF and (out == 0x5A).all()
    assert res.as_dict() == {"quality": (1, 1, 1), "failed_planes": 0, "probes": 2,
                             "at": at_record(name, (1, 1, 1))[0]}
    t = (ctypes.c_uint64 * 3)(S.HUGE, S.HUGE, sses[99][2] - 1)
    rc = L.myyuv_gpu_dct_compress_to_sse(codec._h, u8(a), w, h, t, u8(out), out.size, ctypes.byref(size),
                                         ctypes.byref(res))
    assert rc == myyuv_hip.E_TARGET and size.value == 0xDEADBEEF and (out == 0x5A).all()
    assert res.as_dict() == {"quality": (100, 100, 100), "failed_planes": 4, "probes": 1,
                             "at": at_record(name, (100, 100, 100))[0]}
    # a payload buffer that is too small: compress's E_CAPACITY with the size needed
    small = np.zeros(64, np.uint8)
    rc = L.myyuv_gpu_dct_compress_to_size(codec._h, u8(a), w, h, sizes[49], u8(small), small.size, ctypes.byref(size),
                                          ctypes.byref(res))
    assert rc == myyuv_hip.E_CAPACITY and size.value == sizes[49] and tuple(res.quality) == (50, 50, 50)
    assert check_size(codec, name, sizes[49])  # the context works afterwards
    assert codec.compress(src, w, h, (50, 50, 50)) == at_record(name, (50, 50, 50))[1]


def test_one_larger_size_search(codec, oracle):
    from oracle import oracle as O

    name = "tiled_1040x512"
    src, w, h = frame(name)
    budget = len(O.compress(src, w, h, (50, 50, 50)))
    pay, res = codec.compress_to_size(src, w, h, budget)
    q = res["quality"][0]
    assert res["quality"] == (q, q, q) and pay == O.compress(src, w, h, (q, q, q)) and len(pay) <= budget
    ok, rq, asked = S.size_search(lambda k: len(O.compress(src, w, h, (k, k, k))), budget)
    assert ok and rq == q and res["probes"] == len(asked) and res["at"][1] == len(pay)
    assert q == 100 or len(O.compress(src, w, h, (q + 1,) * 3)) > budget


def test_device_forms(codec, oracle):
    import myyuv_hip
    import torch

    name = "tiled_208x96"
    src, w, h = frame(name)
    sizes, sses = tables(name)
    cap = myyuv_hip.payload_bound(w, h)
    stream = torch.cuda.current_stream().cuda_stream
    d_in = torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda()
    for mode, target in (("size", sizes[36] + 1), ("sse", (sses[36][0], sses[49][1] + 1, sses[98][2])),
                         ("size", sizes[0] - 1)):
        for rep in range(2):
            d_pay = torch.full((cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            d_size = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            call = codec.compress_to_size_device if mode == "size" else codec.compress_to_sse_device
            if mode == "size":
                ok, q, asked = S.size_search(lambda k: sizes[k - 1], target)
                q3 = (q, q, q)
            else:
                ok, q3, _, asked = S.sse_search(lambda k: tuple(sses[k[p] - 1][p] for p in range(3)), target)
            at, pay = at_record(name, q3)
            want = {"quality": q3, "failed_planes": 0, "probes": len(asked), "at": at}
            if not ok:
                e = error_of(call, d_in.data_ptr(), w, h, target, d_pay.data_ptr(), cap, d_size.data_ptr(), stream)
                assert e.code == myyuv_hip.E_TARGET and e.result == want
                assert codec.sync_status(stream) == (0, -1)
                assert (d_pay.cpu().numpy() == 0x5A).all() and (d_size.cpu().numpy() == 0x5A5A5A5A).all()
                continue
            res = call(d_in.data_ptr(), w, h, target, d_pay.data_ptr(), cap, d_size.data_ptr(), stream)
            # (no synchronisation here: the call itself blocks until the payload is written)
            got = d_pay.cpu().numpy()
            sz = d_size.cpu().numpy()
            assert codec.sync_status(stream) == (0, -1)
            assert res == want, (mode, target, res, want)
            assert int(sz[0]) == len(pay) and (sz[1:] == 0x5A5A5A5A).all()
            assert got[:len(pay)].tobytes() == pay and (got[cap:] == 0x5A).all()


# ----------------------------------------------------------------------- CLI
def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def psnr_text(v):
    return "inf" if v == float("inf") else "%.6f" % v


def target_line(q3, at, w, h, probes):
    n = (w * h, w * h // 4, w * h // 4)
    return "quality %d %d %d : size %d : psnr %s dB : %d probes" % (
        *q3, at[1] + 67, " ".join(psnr_text(M.psnr(at[2][p][0], n[p])) for p in range(3)), probes)


@functools.lru_cache(maxsize=None)
def chef_size(q):
    from oracle import oracle as O

    f = R.chef()
    return len(O.compress(f.data, f.width, f.height, (q, q, q)))


@functools.lru_cache(maxsize=None)
def chef_at(q3):
    from oracle import oracle as O

    f = R.chef()
    pay = O.compress(f.data, f.width, f.height, q3)
    recs, _ = M.frame_metric(bytes(f.data), O.decompress(pay, f.width, f.height, q3), f.width, f.height)
    return (struct.unpack("<III", pay[:12]), len(pay), recs), pay


def test_cli_target_size_reproduces_the_golden(oracle, tmp_path):
    f = R.chef()
    gold = open(C50, "rb").read()
    assert len(gold) == chef_size(50) + 67
    ok, q, asked = S.size_search(chef_size, len(gold) - 67)
    assert ok and chef_size(49) <= chef_size(50) < chef_size(51)
    assert q == 50  # (the sizes at the qualities the bisection visits order as the qualities do)
    out = tmp_path / "out.myyuv"
    r = cli(RAW, "-compress", "DCT", "-target_size", str(len(gold)), "-o", str(out))
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes() == gold
    lines = r.stdout.splitlines()
    assert lines[0] == target_line((50, 50, 50), chef_at((50, 50, 50))[0], f.width, f.height, len(asked)), r.stdout
    assert lines[1].startswith("YUV DCT compression ( -target_size ") and lines[-1] == "Success!"


def test_cli_target_psnr_and_probe(oracle, tmp_path):
    import myyuv_file
    from oracle import oracle as O

    f = R.chef()
    w, h = f.width, f.height
    n = (w * h, w * h // 4, w * h // 4)
    ceil = tuple(S.sse_for_psnr(35.0, n[p]) for p in range(3))

    @functools.lru_cache(maxsize=None)
    def sse_at(q):
        return S.plane_sse(bytes(f.data), O.decompress(O.compress(f.data, w, h, (q, q, q)), w, h, (q, q, q)), w, h)

    ok, q3, failed, asked = S.sse_search(lambda k: tuple(sse_at(k[p])[p] for p in range(3)), ceil)
    assert ok
    out = tmp_path / "out.myyuv"
    r = cli(RAW, "-compress", "DCT", "-target_psnr", "35", "-o", str(out))
    assert r.returncode == 0, r.stdout + r.stderr
    g = myyuv_file.YUVFile.load(str(out))
    assert tuple(g.params) == q3 and bytes(g.data) == chef_at(q3)[1]
    assert r.stdout.splitlines()[0] == target_line(q3, chef_at(q3)[0], w, h, len(asked)), r.stdout
    r = cli(RAW, "-probe", "50")
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[0] == target_line((50, 50, 50), chef_at((50, 50, 50))[0], w, h, 1), r.stdout
    r = cli(RAW, "-probe", "90", "50", "20")
    assert r.stdout.splitlines()[0] == target_line((90, 50, 20), chef_at((90, 50, 20))[0], w, h, 1), r.stdout


def test_cli_unreachable_target(oracle, tmp_path):
    out = tmp_path / "out.myyuv"
    for args in (("-target_size", str(chef_size(1) + 67 - 1)), ("-target_size", "10"), ("-target_psnr", "99")):
        r = cli(RAW, "-compress", "DCT", *args, "-o", str(out))
        assert r.returncode == 1 and r.stdout.splitlines() == ["Error compressing: target not reachable"], r.stdout
        assert not out.exists()
    r = cli(RAW, "-compress", "DCT", "-target_size", str(chef_size(1) + 67), "-o", str(out))
    assert r.returncode == 0 and out.exists(), r.stdout + r.stderr
    r = cli(RAW, "-compress", "DCT", "-target_size", "x", "-o", str(out))
    assert r.returncode == 1 and "Usage" in r.stdout

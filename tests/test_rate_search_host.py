"""Encode to a target, the part that needs no GPU: the search of
csrc/rate_search.h (the code the library's compress_to_* entry points run)
compiled into a host program (tools/rate_search_host.cpp) and driven from
tables, against its restatement (ratesearchref) of the definition in
include/myyuv_hip.h.  Tables: the oracle's sizes and squared errors of three
small frames at q = 1 .. 100 (the 16x16 one is not monotone, which tells the
defined bisection from a scan for "the best" quality), and synthetic ones.
Also myyuv_metric_sse_for_psnr against the definition, and the new entry
points' argument checks."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import metricref as M
import ratesearchref as S
import regionref as R
import synth
from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tools", "rate_search_host.cpp")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rate") / "rate_search_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(PKG, "csrc"), SRC, "-o", exe], check=True)
    return exe


def run(exe, mode, table, targets):
    text = [mode, " ".join(str(v) for v in table), str(len(targets))]
    text += [" ".join(str(v) for v in (t if isinstance(t, (tuple, list)) else (t,))) for t in targets]
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(targets)
    return lines


def parse(line):
    head, tail = line.split(":")
    ok, q0, q1, q2, failed, probes = (int(v) for v in head.split())
    asked = [tuple(int(v) for v in part.split()) for part in tail.split(";") if part.strip()]
    return bool(ok), (q0, q1, q2), failed, probes, asked


def frames():
    f = R.chef()
    return {"tiled_208x96": (synth.tiled_frame(f.data, f.width, f.height, 208, 96, 400, 300).tobytes(), 208, 96),
            "noise_208x96": (synth.noise_frame(208, 96, 77).tobytes(), 208, 96),
            "tiled_16x16": (synth.tiled_frame(f.data, f.width, f.height, 16, 16, 400, 300).tobytes(), 16, 16)}


@functools.lru_cache(maxsize=None)
def oracle_tables(name):
    from oracle import oracle as O

    src, w, h = frames()[name]
    return S.oracle_tables(O, src, w, h)


def synthetic():
    """{name: (sizes, sses)}; sizes rise (or not), the error columns fall (or not)."""
    q = np.arange(1, 101)
    rising = (100 + 7 * q).tolist()
    const = [1000] * 100
    step = [500 if v < 60 else 900 for v in q]
    saw = (1000 + 10 * q - 37 * (q % 5)).tolist()
    assert any(a > b for a, b in zip(saw, saw[1:]))

    def cols(a, b, c):
        return [tuple(t) for t in zip(a, b, c)]

    return {"constant": (const, cols(const, const, const)),
            "rising": (rising, cols(rising[::-1], [3 * v for v in rising[::-1]], [v + 5 for v in rising[::-1]])),
            "step": (step, cols(step[::-1], rising[::-1], step[::-1])),
            "sawtooth": (saw, cols(saw[::-1], [2 * v + 1 for v in saw[::-1]], rising[::-1]))}


def all_tables():
    t = {name: oracle_tables(name) for name in frames()}
    t.update(synthetic())
    return t


def monotone(col, rising):
    return all((a <= b) if rising else (a >= b) for a, b in zip(col, col[1:]))


def test_oracle_tables_are_the_issues():
    """The figures the design was checked with, and which tables are monotone."""
    sizes, sses = oracle_tables("tiled_208x96")
    assert (sizes[0], sizes[49], sizes[89], sizes[99]) == (4181, 9972, 17642, 34795)
    assert (sses[0][0], sses[49][0], sses[99][0]) == (8516476, 796125, 1619)
    assert monotone(sizes, True) and all(monotone([s[p] for s in sses], False) for p in range(3))
    sizes, sses = oracle_tables("noise_208x96")
    assert (sizes[0], sizes[99]) == (8669, 62591)
    assert monotone(sizes, True) and all(monotone([s[p] for s in sses], False) for p in range(3))
    sizes, sses = oracle_tables("tiled_16x16")
    assert (min(sizes), max(sizes)) == (90, 513) and sizes[0] == 90 and sizes[99] == 513
    falls = [q for q in range(2, 101) if sizes[q - 1] < sizes[q - 2]]
    assert falls[:6] == [11, 14, 15, 26, 29, 37] and len(falls) == 21
    for p in range(3):
        col = [s[p] for s in sses]
        assert 13 <= sum(1 for a, b in zip(col, col[1:]) if b > a) <= 23


def test_size_search_equals_the_reference(harness):
    for name, (sizes, _) in all_tables().items():
        budgets = S.size_budgets(sizes)
        for b, line in zip(budgets, run(harness, "size", sizes, budgets)):
            ok, q3, failed, probes, asked = parse(line)
            rok, rq, rasked = S.size_search(lambda q: sizes[q - 1], b)
            assert (ok, q3, asked) == (rok, (rq, rq, rq), rasked), (name, b, line)
            assert probes == len(asked) <= 9 and failed == 0
            if not ok:
                assert sizes[0] > b and q3 == (1, 1, 1) and asked == [(100,) * 3, (1,) * 3]
                continue
            q = q3[0]
            assert sizes[q - 1] <= b and (q == 100 or sizes[q] > b), (name, b, q)
            if monotone(sizes, True):
                assert q == max(k for k in range(1, 101) if sizes[k - 1] <= b), (name, b, q)
        assert not S.size_search(lambda q: sizes[q - 1], sizes[0] - 1)[0], name  # (the unreachable budget is there)


def test_sse_search_equals_the_reference(harness):
    for name, (_, sses) in all_tables().items():
        flat = [v for s in sses for v in s]
        ceilings = S.sse_ceilings(sses)
        fails = 0
        for t, line in zip(ceilings, run(harness, "sse", flat, ceilings)):
            ok, q3, failed, probes, asked = parse(line)
            rok, rq3, rfailed, rasked = S.sse_search(lambda q: tuple(sses[q[p] - 1][p] for p in range(3)), t)
            assert (ok, q3, failed, asked) == (rok, rq3, rfailed, rasked), (name, t, line)
            assert probes == len(asked) <= 9
            if not ok:
                fails += 1
                assert q3 == (100, 100, 100) and asked == [(100,) * 3]
                assert failed == sum(1 << p for p in range(3) if sses[99][p] > t[p]) != 0
                continue
            for p in range(3):
                col = [s[p] for s in sses]
                assert col[q3[p] - 1] <= t[p] and (q3[p] == 1 or col[q3[p] - 2] > t[p]), (name, t, p, q3)
                if monotone(col, False):
                    assert q3[p] == min(k for k in range(1, 101) if col[k - 1] <= t[p]), (name, t, p, q3)
        assert fails >= 1, name


def test_the_16x16_frame_tells_the_bisection_from_the_best_quality(harness):
    """Where sizes fall with rising quality a larger fitting quality can exist
    than the bisection's; the definition is the bisection."""
    sizes, _ = oracle_tables("tiled_16x16")
    differs = 0
    budgets = sorted(set(sizes))
    for b, line in zip(budgets, run(harness, "size", sizes, budgets)):
        ok, q3, _, _, _ = parse(line)
        assert ok and q3[0] == S.size_search(lambda q: sizes[q - 1], b)[1]
        differs += q3[0] != max(k for k in range(1, 101) if sizes[k - 1] <= b)
    assert differs > 0


DBS = [float(v) for v in np.linspace(0.0, 100.0, 201)] + [math.pi * 10, 33.333333333, 48.13, 1e-9, 99.999999]
NS = [64, 19968, 1 << 26]


def test_sse_for_psnr(harness):
    import myyuv_hip

    targets = [(repr(db), n) for db in DBS for n in NS] + [("inf", 64), ("-5", 64), ("0", 19968)]
    got = [int(v) for v in run(harness, "psnr", [], targets)]
    for (text, n), s in zip(targets, got):
        db = float(text)
        top = 65025 * n
        assert s == S.sse_for_psnr(db, n), (text, n, s)
        assert s == myyuv_hip.metric_sse_for_psnr(db, n), (text, n, s)
        if db <= 0:
            assert s == top
        elif math.isinf(db):
            assert s == 0
        else:  # the definition, next to the boundary
            assert M.psnr(s, n) >= db and (s == top or M.psnr(s + 1, n) < db), (text, n, s)
            assert all(M.psnr(k, n) >= db for k in range(max(0, s - 3), s + 1))
            assert all(M.psnr(k, n) < db for k in range(s + 1, min(top, s + 4) + 1))
    assert myyuv_hip.metric_sse_for_psnr(float("nan"), 64) == 0


def test_argument_errors_need_no_device():
    """The new entry points' pointer, quality, dimension and `what` checks come
    before any device is touched, in compress's order."""
    import myyuv_hip

    L = myyuv_hip.load()
    E = myyuv_hip
    fake = ctypes.c_void_p(8)  # (never dereferenced: the argument checks come first)
    frame = np.zeros(384, np.uint8)
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    q = np.array([50, 50, 50], np.uint8)
    out = myyuv_hip.Probe()
    assert L.myyuv_gpu_dct_probe(None, u8(frame), 16, 16, u8(q), 3, ctypes.byref(out), None) == E.E_ARG
    assert L.myyuv_gpu_dct_probe(fake, None, 16, 16, u8(q), 3, ctypes.byref(out), None) == E.E_ARG
    assert L.myyuv_gpu_dct_probe(fake, u8(frame), 16, 16, u8(q), 3, None, None) == E.E_ARG
    for bad in ((0, 50, 50), (50, 101, 50)):
        qb = np.array(bad, np.uint8)
        assert L.myyuv_gpu_dct_probe(fake, u8(frame), 16, 16, u8(qb), 0, ctypes.byref(out), None) == E.E_QUALITY
    assert L.myyuv_gpu_dct_probe(fake, u8(frame), 12, 16, u8(q), 0, ctypes.byref(out), None) == E.E_WIDTH
    assert L.myyuv_gpu_dct_probe(fake, u8(frame), 16, 24, u8(q), 0, ctypes.byref(out), None) == E.E_HEIGHT
    for what in (0, 4, 7, 1 << 31):
        assert L.myyuv_gpu_dct_probe(fake, u8(frame), 16, 16, u8(q), what, ctypes.byref(out), None) == E.E_ARG
        assert L.myyuv_gpu_dct_probe_device(fake, 256, 1, 16, 16, u8(q), what, 1024, None, None) == E.E_ARG
    assert L.myyuv_gpu_dct_probe_device(fake, 256, 0, 16, 16, u8(q), 3, 1024, None, None) == E.E_ARG  # no frames
    assert L.myyuv_gpu_dct_probe_device(fake, 260, 1, 16, 16, u8(q), 3, 1024, None, None) == E.E_ARG  # alignment
    assert L.myyuv_gpu_dct_probe_device(fake, 256, 1, 16, 16, u8(q), 3, 1028, None, None) == E.E_ARG
    assert L.myyuv_gpu_dct_probe_device(fake, 256, 1, 16, 24, u8(q), 3, 1024, None, None) == E.E_HEIGHT
    res = myyuv_hip.TargetResult()
    size = ctypes.c_uint32(77)
    pay = np.zeros(64, np.uint8)
    t = (ctypes.c_uint64 * 3)(1, 2, 3)
    assert L.myyuv_gpu_dct_compress_to_size(None, u8(frame), 16, 16, 100, u8(pay), 64, ctypes.byref(size),
                                            ctypes.byref(res)) == E.E_ARG
    assert L.myyuv_gpu_dct_compress_to_size(fake, u8(frame), 16, 16, 100, u8(pay), 64, ctypes.byref(size),
                                            None) == E.E_ARG
    assert L.myyuv_gpu_dct_compress_to_size(fake, u8(frame), 12, 16, 100, u8(pay), 64, ctypes.byref(size),
                                            ctypes.byref(res)) == E.E_WIDTH
    assert L.myyuv_gpu_dct_compress_to_sse(fake, u8(frame), 16, 16, None, u8(pay), 64, ctypes.byref(size),
                                           ctypes.byref(res)) == E.E_ARG
    assert L.myyuv_gpu_dct_compress_to_sse(fake, u8(frame), 16, 20, t, u8(pay), 64, ctypes.byref(size),
                                           ctypes.byref(res)) == E.E_HEIGHT
    assert L.myyuv_gpu_dct_compress_to_size_device(fake, 256, 16, 16, 100, None, 64, 512, ctypes.byref(res),
                                                   None) == E.E_ARG
    assert L.myyuv_gpu_dct_compress_to_sse_device(fake, 256, 16, 16, t, 1026, 64, 512, ctypes.byref(res),
                                                  None) == E.E_ARG  # d_payload not 4-byte aligned
    assert size.value == 77
    assert E.E_TARGET == 18 and myyuv_hip.error_message(18) == "target not reachable"
    assert myyuv_hip.strerror(18) == "Unknown error"  # (strerror's table is closed at 17)
    assert all(myyuv_hip.error_message(k) == myyuv_hip.strerror(k) for k in list(range(18)) + [19, -1])
    assert ctypes.sizeof(myyuv_hip.Probe) == 88 == myyuv_hip.PROBE_DTYPE.itemsize
    assert ctypes.sizeof(myyuv_hip.TargetResult) == 96
    assert myyuv_hip.KERNELS_EVERY[myyuv_hip.K_COEF_CMP] == "coef_compare" and myyuv_hip.K_COEF_CMP == 21
    assert myyuv_hip.KERNELS_EVERY[myyuv_hip.K_PROBE_OUT] == "probe_out" and myyuv_hip.K_PROBE_OUT == 22
    assert myyuv_hip.KERNELS_EVERY[:myyuv_hip.K_END] == myyuv_hip.KERNELS_ALL and myyuv_hip.K_END == 21
    assert myyuv_hip.K_LIMIT == 23 == len(myyuv_hip.KERNELS_EVERY) and myyuv_hip.K_TOTAL == 18

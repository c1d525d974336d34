"""The search of "Encode to a target", restated from its definition in
include/myyuv_hip.h over a callable: size(q) -> payload bytes of the quality
(q, q, q), or sse(q3) -> the three planes' squared errors at the triple q3.
Each returns the probe sequence (a list of triples) beside the result, so the
library's search (csrc/rate_search.h) can be compared step by step.  Plain
Python integers; nothing outside the repository is read."""
import math

import metricref as M


QS = (2, 37, 50, 51, 99)  # the qualities whose sizes and errors the tests aim at, beside 1 and 100
HUGE = (1 << 64) - 1


def plane_sse(ref, test, w, h):
    """The three planes' squared errors between two frames (metricref's sse)."""
    import numpy as np

    out = []
    for px, py in zip(M.planes(ref, w, h), M.planes(test, w, h)):
        d = px.astype(np.int64) - py.astype(np.int64)
        out.append(int((d * d).sum()))
    return tuple(out)


def oracle_tables(O, src, w, h):
    """(sizes, sses) of the frame for q = 1 .. 100 (index q - 1) from the
    oracle: payload bytes of (q, q, q), and the planes' sse of its decode
    against src.  A plane's figures depend on its own quality alone."""
    sizes, sses = [], []
    for q in range(1, 101):
        pay = O.compress(src, w, h, (q, q, q))
        sizes.append(len(pay))
        sses.append(plane_sse(src, O.decompress(pay, w, h, (q, q, q)), w, h))
    return sizes, sses


def size_budgets(sizes):
    b = [sizes[0] - 1, sizes[0], sizes[99] - 1, sizes[99], (1 << 32) - 1]
    for q in QS:
        b += [sizes[q - 1] - 1, sizes[q - 1], sizes[q - 1] + 1]
    return [v for v in b if v >= 0]


def sse_ceilings(sses):
    """Triples of ceilings: per plane the mirror of size_budgets with the other
    planes unconstrained, three different ones at once, one failing plane."""
    out = []
    for p in range(3):
        col = [s[p] for s in sses]
        vals = [col[99] - 1, col[99], col[0] - 1, col[0], HUGE]
        for q in QS:
            vals += [col[q - 1] - 1, col[q - 1], col[q - 1] + 1]
        for v in vals:
            if v >= 0:
                t = [HUGE, HUGE, HUGE]
                t[p] = v
                out.append(tuple(t))
    out.append((sses[36][0], sses[49][1] + 1, max(0, sses[98][2] - 1)))
    out.append((sses[1][0], sses[98][1], sses[50][2]))
    if sses[99][1] > 0:
        out.append((sses[49][0], sses[99][1] - 1, sses[49][2]))  # U cannot be met
    return out


def size_search(size, budget):
    """-> (ok, q, probes): probes the list of triples asked, q the chosen
    quality, or with ok False the failing probe's (1)."""
    probes = []

    def ask(q):
        probes.append((q, q, q))
        return size(q)

    if ask(100) <= budget:
        return True, 100, probes
    if ask(1) > budget:
        return False, 1, probes
    lo, hi = 1, 100
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ask(mid) <= budget:
            lo = mid
        else:
            hi = mid
    return True, lo, probes


def sse_search(sse, max_sse):
    """-> (ok, q3, failed_planes, probes): q3 the chosen triple, or with ok
    False (100, 100, 100) and the failing planes as a bit mask."""
    probes = []

    def ask(q3):
        probes.append(tuple(q3))
        return sse(tuple(q3))

    got = ask((100, 100, 100))
    failed = sum(1 << p for p in range(3) if got[p] > max_sse[p])
    if failed:
        return False, (100, 100, 100), failed, probes
    got = ask((1, 1, 1))
    res = [1 if got[p] <= max_sse[p] else None for p in range(3)]
    lo, hi = [1, 1, 1], [100, 100, 100]
    while any(r is None for r in res):
        q3 = [res[p] if res[p] is not None else (lo[p] + hi[p]) // 2 for p in range(3)]
        got = ask(q3)
        for p in range(3):
            if res[p] is not None:
                continue
            if got[p] <= max_sse[p]:
                hi[p] = q3[p]
            else:
                lo[p] = q3[p]
            if hi[p] - lo[p] <= 1:
                res[p] = hi[p]
    return True, tuple(res), 0, probes


def sse_for_psnr(db, nsamples):
    """The largest s with metricref.psnr(s, nsamples) >= db; 65025 * nsamples
    for db <= 0, 0 for +inf."""
    top = 65025 * nsamples
    if db <= 0:
        return top
    if math.isinf(db):
        return 0
    s = min(top, max(0, int(65025.0 * nsamples / 10.0 ** (db / 10.0))))
    while s < top and M.psnr(s + 1, nsamples) >= db:
        s += 1
    while s > 0 and not M.psnr(s, nsamples) >= db:
        s -= 1
    return s

"""What Compare must return, restated with numpy and Python integers from the
definition in include/myyuv_hip.h ("Compare"): per 8x8 block of a plane the
squared error, the largest difference and the 2^24-scaled block SSIM, per
plane their sums.  Every figure is an exact integer: the sums in int64, the
quotient as (num << 24) // den on Python ints (floor towards minus infinity).
Nothing outside the repository is read."""
import math

import numpy as np

C1 = 26634    # round(4096 * (0.01 * 255) ** 2)
C2 = 239708   # round(4096 * (0.03 * 255) ** 2)
ONE = 1 << 24
BLOCK = np.dtype([("sse", np.uint32), ("ssim", np.int32)])
PLANES = "YUV"

assert C1 == round(4096 * (0.01 * 255) ** 2) and C2 == round(4096 * (0.03 * 255) ** 2)


def sums(x, y):
    """(sse, max, Sx, Sy, Sxx, Syy, Sxy) of blocks x, y: int64 arrays [n] from
    samples [n, 64]."""
    x = np.asarray(x).reshape(-1, 64).astype(np.int64)
    y = np.asarray(y).reshape(-1, 64).astype(np.int64)
    d = x - y
    return ((d * d).sum(1), np.abs(d).max(1), x.sum(1), y.sum(1), (x * x).sum(1), (y * y).sum(1), (x * y).sum(1))


def terms(sx, sy, sxx, syy, sxy):
    """(A1, A2, B1, B2) as Python ints."""
    sx, sy, sxx, syy, sxy = int(sx), int(sy), int(sxx), int(syy), int(sxy)
    a1 = 2 * sx * sy + C1
    a2 = 2 * (64 * sxy - sx * sy) + C2
    b1 = sx * sx + sy * sy + C1
    b2 = 64 * (sxx + syy) - sx * sx - sy * sy + C2
    return a1, a2, b1, b2


def ssim_of_sums(sx, sy, sxx, syy, sxy):
    a1, a2, b1, b2 = terms(sx, sy, sxx, syy, sxy)
    assert 0 < b1 < 1 << 29 and 0 < b2 < 1 << 27 and abs(a1 * a2) <= b1 * b2
    return ((a1 * a2) << 24) // (b1 * b2)


def ssim_blocks(x, y):
    """ssim_k of every block pair: a list of Python ints."""
    _, _, sx, sy, sxx, syy, sxy = sums(x, y)
    return [ssim_of_sums(*t) for t in zip(sx, sy, sxx, syy, sxy)]


def plane_blocks(plane):
    """uint8[h, w] -> [n, 64], the codec's block order k = (y/8) * bw + x/8."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


def planes(iyuv, w, h):
    a = np.frombuffer(bytes(iyuv), np.uint8)
    assert a.size == w * h * 3 // 2
    return (a[:w * h].reshape(h, w), a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2),
            a[w * h * 5 // 4:].reshape(h // 2, w // 2))


def frame_metric(ref, test, w, h):
    """(records, map): records = ((sse, ssim_sum, nblocks, max_abs) of Y, U,
    V) as Python ints, map = BLOCK array over the blocks of Y, then U, then V."""
    recs, maps = [], []
    for px, py in zip(planes(ref, w, h), planes(test, w, h)):
        x, y = plane_blocks(px), plane_blocks(py)
        sse, mx = sums(x, y)[:2]
        ss = ssim_blocks(x, y)
        m = np.zeros(len(ss), BLOCK)
        m["sse"] = sse
        m["ssim"] = ss
        maps.append(m)
        recs.append((int(sse.sum()), int(sum(ss)), len(ss), int(mx.max())))
    return tuple(recs), np.concatenate(maps)


def psnr(sse, nsamples):
    return math.inf if sse == 0 else 10.0 * math.log10(65025.0 * nsamples / sse)


def ssim(ssim_sum, nblocks):
    return ssim_sum / (nblocks * 16777216.0)


def _psnr_text(v):
    return "inf" if math.isinf(v) else "%.6f" % v


def report(recs, bmap, w, h):
    """The text myyuv_cli -compare prints for these integers."""
    lines = []
    samples = (w * h, w * h // 4, w * h // 4)
    for p, (sse, ss, nb, mx) in enumerate(recs):
        lines.append("%s: psnr %s dB ssim %.6f sse %d max %d" %
                     (PLANES[p], _psnr_text(psnr(sse, samples[p])), ssim(ss, nb), sse, mx))
    lines.append("all: psnr %s dB ssim %.6f" %
                 (_psnr_text(psnr(sum(r[0] for r in recs), w * h * 3 // 2)),
                  ssim(sum(r[1] for r in recs), sum(r[2] for r in recs))))
    k = int(np.argmin(bmap["ssim"]))  # the first of the lowest: plane, then index
    ny, nc = (w // 8) * (h // 8), (w // 16) * (h // 16)
    p = 0 if k < ny else (1 if k < ny + nc else 2)
    local = k - (0, ny, ny + nc)[p]
    bw = w // 8 if p == 0 else w // 16
    lines.append("worst block: plane %s x %d y %d sse %d ssim %.6f" %
                 (PLANES[p], (local % bw) * 8, (local // bw) * 8, int(bmap["sse"][k]),
                  int(bmap["ssim"][k]) / 16777216.0))
    return "\n".join(lines) + "\n"

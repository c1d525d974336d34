#!/usr/bin/env python3
"""Kernel rates of the two colour conversions, K7 (BMP -> IYUV) and K8
(IYUV -> BMP), from one process and one frame size.

The method of bench.py's K7 side figure: 3 warm-up launches, 50 launches
stamped through profile(kernels=[...]) (the kernels' own dispatch-packet
times), then kernel_stats.  Both kernels stream, so the bound is HBM and the
algorithmic bytes are 1.5 + bpp per pixel.  The whole series runs --repeats
times; each variant reports the median fraction of peak and the spread
(min .. max) over the repeats, alternating the variants inside a repeat so
that drift hits all of them alike.

  python tools/color_rate.py [--width 4032 --height 3008] [--repeats 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yuv-manipulations-2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0  # MI355X, as bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=4032)
    ap.add_argument("--height", type=int, default=3008)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import myyuv_hip

    if not torch.cuda.is_available():
        sys.exit("color_rate: no GPU (a rate is only ever measured on one)")
    dev = torch.device("cuda", 0)
    w, h = args.width, args.height
    codec = myyuv_hip.Codec(0)
    sp = torch.cuda.current_stream(dev).cuda_stream
    bgra = torch.randint(0, 256, (w * h * 4,), dtype=torch.uint8, device=dev)
    iyuv = torch.randint(0, 256, (w * h * 3 // 2,), dtype=torch.uint8, device=dev)
    d_iy = torch.empty(w * h * 3 // 2, dtype=torch.uint8, device=dev)
    d_px = torch.empty(w * h * 4, dtype=torch.uint8, device=dev)

    # (name, stamped kernel, bytes per pixel moved, launch); bottom-up frames, as bench.py's K7 figure
    variants = [
        ("k7_bgra", "bmp_to_iyuv", 5.5,
         lambda: codec.bmp_to_iyuv_device(bgra.data_ptr(), w, h, 32, d_iy.data_ptr(), sp)),
        ("k8_32_nearest", "iyuv_to_bmp", 5.5,
         lambda: codec.iyuv_to_bmp_device(iyuv.data_ptr(), 1, w, h, 32, myyuv_hip.CHROMA_NEAREST, d_px.data_ptr(), sp)),
        ("k8_32_linear", "iyuv_to_bmp", 5.5,
         lambda: codec.iyuv_to_bmp_device(iyuv.data_ptr(), 1, w, h, 32, myyuv_hip.CHROMA_LINEAR, d_px.data_ptr(), sp)),
        ("k8_24_linear", "iyuv_to_bmp", 4.5,
         lambda: codec.iyuv_to_bmp_device(iyuv.data_ptr(), 1, w, h, 24, myyuv_hip.CHROMA_LINEAR, d_px.data_ptr(), sp)),
    ]
    fracs = {name: [] for name, *_ in variants}
    times = {name: [] for name, *_ in variants}
    for _ in range(args.repeats):
        for name, kernel, bpp, launch in variants:
            for _ in range(3):
                launch()
            codec.sync_status(sp)
            codec.profile(True, kernels=[kernel])
            for _ in range(args.launches):
                launch()
            codec.sync_status(sp)
            ms, n = codec.kernel_stats()[kernel]
            codec.profile(False)
            if n != args.launches:
                sys.exit(f"color_rate: {name}: {n} stamped launches, expected {args.launches}")
            us = ms / n * 1e3
            times[name].append(us)
            fracs[name].append(w * h * bpp / (us * 1e-6) / 1e9 / HBM_PEAK_GBS)
    res = {"frame": f"{w}x{h}", "launches": args.launches, "repeats": args.repeats, "bound": "hbm",
           "peak_gbs": HBM_PEAK_GBS, "variants": {}}
    for name, _k, bpp, _l in variants:
        f = fracs[name]
        res["variants"][name] = {
            "algorithmic_bytes_per_launch": int(w * h * bpp),
            "avg_launch_us": [round(t, 2) for t in times[name]],
            "frac": [round(x, 4) for x in f],
            "frac_median": round(statistics.median(f), 4),
            "frac_spread": round(max(f) - min(f), 4),
            "achieved_gbs_median": round(statistics.median(f) * HBM_PEAK_GBS, 1),
        }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()

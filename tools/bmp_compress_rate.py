#!/usr/bin/env python3
"""Compress from BMP against bmp_to_iyuv + compress, on one stream of one process.

The pictures are the decoded chef-big golden (4032x3008) and the 8192x8192
tiled frame (SURVEY.md §8d generator), turned into BGRA and BGR pixel arrays on
the GPU (K8, nearest chroma), at q50 and q90.  Per (frame, depth, quality),
device-resident, after 3 warm-up calls of each variant, the variants ALTERNATE
call by call inside one loop of --calls rounds, each call bracketed by HIP
events on the calls' stream; the median (min - max) per variant:
  * bmp_to_iyuv_device followed by compress_device (unchanged code: the
    yardstick of the same run),
  * compress_bmp_device (the new path).
Then the per-kernel split of both paths from kernel_stats (a separate loop with
event stamping on: stamping costs queue time, so the split is not taken from
the timed calls): k_bmp_fdct's time against K7 + K1 + the fix kernel's, and its
achieved share of the 8 TB/s HBM peak on the bytes the algorithm needs
(bpp + 2 B per pixel: the pixels in, the int16 coefficients out as K1 counts
them).  Then the host-buffer forms (pageable buffers, PCIe both ways, wall
clock, alternating, the median of --host-calls): compress_bmp_into against
bmp_to_iyuv + compress_into.

Recorded besides: the payload size, and that the two paths' streams are equal
byte for byte.  Nothing is gated on the times: the table goes to DESIGN.md as
measured.

  python tools/bmp_compress_rate.py [--calls 20] [--out profiles/bmp_compress_rate.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yuv-manipulations-2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12  # B/s (MI355X)


def summary(v, nd=1):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--sizes", default="4032x3008,8192x8192")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import myyuv_file
    import myyuv_hip
    import synth

    if not torch.cuda.is_available():
        sys.exit("bmp_compress_rate: no GPU (a time is only ever measured on one)")
    dev = torch.device("cuda", 0)
    codec = myyuv_hip.Codec(0)
    st = torch.cuda.Stream(dev)  # explicit: handle 0 would mean the context's own stream
    sp = st.cuda_stream
    torch.cuda.set_stream(st)

    def u8(a):
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))

    def ok(what):
        rc, bad = codec.sync_status(sp)
        if rc:
            sys.exit(f"bmp_compress_rate: {what} failed: {rc} at {bad}")

    g = myyuv_file.YUVFile.load(os.path.join(ROOT, "tests", "golden", "chef-with-trumpet-big-DCT-50.myyuv"))
    src = torch.frombuffer(bytearray(codec.decompress(g.data, g.width, g.height, tuple(g.params))),
                           dtype=torch.uint8).to(dev)

    def alternate_us(calls, what):
        """calls: {name: fn}; the variants one after the other, round by round."""
        for fn in calls.values():
            for _ in range(3):
                fn()
        ok(what)
        out = {k: [] for k in calls}
        for _ in range(args.calls):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                e1.synchronize()
                out[k].append(e0.elapsed_time(e1) * 1e3)
        ok(what)
        return {k: summary(v) for k, v in out.items()}

    def split(call, what):
        codec.profile(True)
        try:
            for _ in range(args.calls):
                call()
            ok(what)
            stats = codec.kernel_stats()
        finally:
            codec.profile(False)
        return {k: round(ms * 1e3 / args.calls, 1) for k, (ms, n) in stats.items() if n}

    res = {"calls": args.calls, "host_calls": args.host_calls, "hbm_peak_bytes_per_s": HBM_PEAK, "cases": []}
    for size in args.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        d_iyuv0 = src if (w, h) == (g.width, g.height) else synth.tiled_frame_torch(src, g.width, g.height, w, h).contiguous()
        n_iyuv = w * h * 3 // 2
        cap = myyuv_hip.payload_bound(w, h)
        codec.reserve(w, h)
        for bits in (32, 24):
            bpp = bits // 8
            d_bmp = torch.empty(w * h * bpp, dtype=torch.uint8, device=dev)
            codec.iyuv_to_bmp_device(d_iyuv0.data_ptr(), 1, w, h, bits, myyuv_hip.CHROMA_NEAREST, d_bmp.data_ptr(), sp)
            ok("iyuv_to_bmp")
            h_bmp = d_bmp.cpu().numpy()
            d_iyuv = torch.empty(n_iyuv, dtype=torch.uint8, device=dev)
            d_two = torch.empty(cap, dtype=torch.uint8, device=dev)
            d_stwo = torch.zeros(1, dtype=torch.int32, device=dev)
            d_one = torch.empty(cap, dtype=torch.uint8, device=dev)
            d_sone = torch.zeros(1, dtype=torch.int32, device=dev)
            for q in ((50, 50, 50), (90, 90, 90)):
                def chain():
                    codec.bmp_to_iyuv_device(d_bmp.data_ptr(), w, h, bits, d_iyuv.data_ptr(), sp)
                    codec.compress_device(d_iyuv.data_ptr(), w, h, q, d_two.data_ptr(), cap, d_stwo.data_ptr(), sp)

                def fused():
                    codec.compress_bmp_device(d_bmp.data_ptr(), 1, w, h, bits, q, d_one.data_ptr(), cap, d_sone.data_ptr(), sp)

                r = {"frame": f"{w}x{h}", "bit_count": bits, "quality": q[0]}
                r["device_us"] = alternate_us({"bmp_to_iyuv_then_compress": chain, "compress_bmp": fused}, "device calls")
                n1, n2 = int(d_sone.item()), int(d_stwo.item())
                r["payload_bytes"] = n1
                r["streams_equal"] = bool(n1 == n2 and torch.equal(d_one[:n1], d_two[:n2]))
                ku = {"compress_bmp": split(fused, "compress_bmp"), "bmp_to_iyuv_then_compress": split(chain, "chain")}
                r["kernel_us"] = ku
                t_new = ku["compress_bmp"].get("bmp_fdct", 0.0)
                t_old = sum(ku["bmp_to_iyuv_then_compress"].get(k, 0.0) for k in ("bmp_to_iyuv", "fdct_quant", "fdct_fix"))
                r["bmp_fdct_us"] = t_new
                r["k7_k1_fix_us"] = round(t_old, 1)
                if t_new > 0:
                    r["bmp_fdct_hbm_fraction"] = round(w * h * (bpp + 2) / (t_new * 1e-6) / HBM_PEAK, 3)
                out = np.empty(cap, np.uint8)
                iyuv = np.empty(n_iyuv, np.uint8)

                def host_chain():  # (the C call, into a buffer kept across calls: no copy of the binding's)
                    rc = myyuv_hip.load().myyuv_gpu_bmp_to_iyuv(codec._h, u8(h_bmp), w, h, bits, u8(iyuv))
                    if rc:
                        sys.exit(f"bmp_compress_rate: bmp_to_iyuv failed: {rc}")
                    codec.compress_into(iyuv, w, h, q, out)

                def host_fused():
                    codec.compress_bmp_into(h_bmp, w, h, bits, q, out)

                hv = {"bmp_to_iyuv_then_compress": host_chain, "compress_bmp": host_fused}
                for fn in hv.values():
                    fn()
                ts = {k: [] for k in hv}
                for _ in range(args.host_calls):
                    for k, fn in hv.items():
                        t0 = time.perf_counter()
                        fn()
                        ts[k].append((time.perf_counter() - t0) * 1e3)
                r["host_ms"] = {k: summary(v, 2) for k, v in ts.items()}
                res["cases"].append(r)

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()

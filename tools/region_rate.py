#!/usr/bin/env python3
"""Region decode against the full decode, on one stream of one process.

The frame is the 8192x8192 tiled q50 frame (SURVEY.md §8d generator from the
decoded chef-big golden; BASELINE.json configs[2]), built and compressed on
the GPU.  Device-resident, after 3 warm-up calls, each call bracketed by HIP
events on the call's stream, the median of --calls calls:
  * decompress_device (the full decode, unchanged by the region path),
  * decompress_region_device for a 1920x1088 and a 256x256 region at the
    frame's centre and for the whole frame through the region path.
Then the host-buffer calls (pageable buffers, PCIe both ways, wall clock):
decompress_into against decompress_region_into for the same regions.

Exits non-zero when the 1920x1088 region call is not faster than the full
decode of the same run: it decodes 2 % of the blocks.

  python tools/region_rate.py [--size 8192] [--calls 20] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yuv-manipulations-2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def centred(size, rw, rh):
    return ((size - rw) // 2 & ~15, (size - rh) // 2 & ~15, rw, rh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import myyuv_file
    import myyuv_hip
    import synth

    if not torch.cuda.is_available():
        sys.exit("region_rate: no GPU (a time is only ever measured on one)")
    dev = torch.device("cuda", 0)
    w = h = args.size
    q = (50, 50, 50)
    codec = myyuv_hip.Codec(0)
    st = torch.cuda.Stream(dev)  # explicit: handle 0 would mean the context's own stream
    sp = st.cuda_stream
    torch.cuda.set_stream(st)

    g = myyuv_file.YUVFile.load(os.path.join(ROOT, "tests", "golden", "chef-with-trumpet-big-DCT-50.myyuv"))
    src = torch.frombuffer(bytearray(codec.decompress(g.data, g.width, g.height, tuple(g.params))),
                           dtype=torch.uint8).to(dev)
    d_in = synth.tiled_frame_torch(src, g.width, g.height, w, h).contiguous()
    cap = myyuv_hip.payload_bound(w, h)
    d_pay = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_size = torch.zeros(1, dtype=torch.int32, device=dev)
    codec.compress_device(d_in.data_ptr(), w, h, q, d_pay.data_ptr(), cap, d_size.data_ptr(), sp)
    rc, bad = codec.sync_status(sp)
    if rc:
        sys.exit(f"region_rate: compress failed: {rc} at {bad}")
    size = int(d_size.item())
    d_full = torch.empty(w * h * 3 // 2, dtype=torch.uint8, device=dev)
    d_reg = torch.empty(w * h * 3 // 2, dtype=torch.uint8, device=dev)

    regions = {"1920x1088": centred(w, 1920, 1088), "256x256": centred(w, 256, 256), "full": (0, 0, w, h)}

    def full():
        codec.decompress_device(d_pay.data_ptr(), d_size.data_ptr(), cap, w, h, q, d_full.data_ptr(), sp)

    def region(rg):
        return lambda: codec.decompress_region_device(d_pay.data_ptr(), d_size.data_ptr(), cap, 1, w, h, q, rg,
                                                      d_reg.data_ptr(), sp)

    def device_us(call):
        for _ in range(3):
            call()
        codec.sync_status(sp)
        out = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
        rc, bad = codec.sync_status(sp)
        if rc:
            sys.exit(f"region_rate: decode failed: {rc} at {bad}")
        return out

    res = {"frame": f"{w}x{h} tiled q50", "payload_bytes": size, "calls": args.calls, "device_us": {}, "host_ms": {}}
    t = device_us(full)
    res["device_us"]["decompress_device"] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1),
                                             "max": round(max(t), 1)}
    # the region path computes the crop of the full decode (checked once here, not timed)
    fy = d_full[: w * h].view(h, w)
    for name, rg in regions.items():
        t = device_us(region(rg))
        rx, ry, rw, rh = rg
        same = bool(torch.equal(d_reg[: rw * rh].view(rh, rw), fy[ry:ry + rh, rx:rx + rw]))
        res["device_us"]["region_" + name] = {"region": list(rg), "median": round(statistics.median(t), 1),
                                              "min": round(min(t), 1), "max": round(max(t), 1),
                                              "luma_equals_crop": same}
        if not same:
            sys.exit(f"region_rate: region {rg} is not the crop of the full decode")

    # host buffers (PCIe included)
    pay = d_pay[:size].cpu().numpy()
    out = np.empty(w * h * 3 // 2, np.uint8)

    def host_ms(call):
        call()
        ts = []
        for _ in range(args.host_calls):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}

    res["host_ms"]["decompress"] = host_ms(lambda: codec.decompress_into(pay, w, h, q, out))
    for name, rg in regions.items():
        res["host_ms"]["region_" + name] = host_ms(lambda rg=rg: codec.decompress_region_into(pay, w, h, q, rg, out))

    gate = res["device_us"]["region_1920x1088"]["median"] < res["device_us"]["decompress_device"]["median"]
    res["region_1920x1088_faster_than_full"] = gate
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    codec.close()
    if not gate:
        sys.exit("region_rate: the 1920x1088 region call is not faster than the full decode")


if __name__ == "__main__":
    main()

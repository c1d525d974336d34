#!/usr/bin/env python3
"""Scaled decode against the full decode, on one stream of one process.

The frame is the 8192x8192 tiled q50 frame (SURVEY.md §8d generator from the
decoded chef-big golden; BASELINE.json configs[2]), built and compressed on
the GPU.  Device-resident, after 3 warm-up calls, each call bracketed by HIP
events on the call's stream, the median of --calls calls:
  * decompress_device (the full decode, the yardstick of the same run),
  * decompress_scaled_device at 1/2, 1/4 and 1/8.
Then the host-buffer calls (pageable buffers, PCIe both ways, wall clock):
decompress_into against decompress_scaled_into at the three scales.

Each scaled frame is checked once, not timed, to be a picture of the frame:
its luma against the box average of the full decode's (mean absolute
difference below 2 grey levels).  Nothing is gated on the times: the table
goes to DESIGN.md §4 as measured.

  python tools/scaled_rate.py [--size 8192] [--calls 20] [--out FILE.json]
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
        sys.exit("scaled_rate: no GPU (a time is only ever measured on one)")
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
        sys.exit(f"scaled_rate: compress failed: {rc} at {bad}")
    size = int(d_size.item())
    d_full = torch.empty(w * h * 3 // 2, dtype=torch.uint8, device=dev)
    d_small = torch.empty(w * h * 3 // 2 // 4, dtype=torch.uint8, device=dev)

    def full():
        codec.decompress_device(d_pay.data_ptr(), d_size.data_ptr(), cap, w, h, q, d_full.data_ptr(), sp)

    def scaled(denom):
        return lambda: codec.decompress_scaled_device(d_pay.data_ptr(), d_size.data_ptr(), cap, 1, w, h, q, denom,
                                                      d_small.data_ptr(), sp)

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
            sys.exit(f"scaled_rate: decode failed: {rc} at {bad}")
        return {"median": round(statistics.median(out), 1), "min": round(min(out), 1), "max": round(max(out), 1)}

    res = {"frame": f"{w}x{h} tiled q50", "payload_bytes": size, "calls": args.calls, "device_us": {}, "host_ms": {}}
    res["device_us"]["decompress_device"] = device_us(full)
    fy = d_full[: w * h].view(h, w).float()
    for denom in (2, 4, 8):
        r = device_us(scaled(denom))
        sw, sh_ = w // denom, h // denom
        box = fy.view(sh_, denom, sw, denom).mean(dim=(1, 3))
        mad = float((d_small[: sw * sh_].view(sh_, sw).float() - box).abs().mean().item())
        r["bytes_out"] = w * h * 3 // 2 // denom ** 2
        r["luma_mad_vs_box_average"] = round(mad, 3)
        res["device_us"][f"scaled_1/{denom}"] = r
        if not mad < 2.0:
            sys.exit(f"scaled_rate: the 1/{denom} frame is no picture of the full decode (MAD {mad})")
    # the full decode again, after the scaled calls: the spread of the yardstick within the run
    res["device_us"]["decompress_device_again"] = device_us(full)

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
    for denom in (2, 4, 8):
        res["host_ms"][f"scaled_1/{denom}"] = host_ms(lambda d=denom: codec.decompress_scaled_into(pay, w, h, q, d, out))

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()

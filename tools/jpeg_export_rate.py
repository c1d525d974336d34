#!/usr/bin/env python3
"""Export to JPEG against requantise and decompress, on one stream of one process.

Frames: the 8192x8192 tiled frame (SURVEY.md §8d generator from the decoded
chef-big golden) compressed on the GPU at q50 and at q90, and the 4032x3008
chef-big golden stream itself (q50).  Per frame, device-resident, after 3
warm-up calls, each measurement bracketed by HIP events on the calls' stream,
min / median / max of --calls:
  * to_jpeg_device (the new path: sizing launch, placement, writing launch),
  * requantize_device q -> q of the same stream and decompress_device alone
    (unchanged code: the yardsticks of the same run), before and after the new
    path's measurement.
Then the host-buffer form (pageable buffers, PCIe both ways, wall clock):
to_jpeg_into against requantize_into.  Recorded besides: the file's bytes
against the stream's, and the per-kernel split from kernel_stats (a loop of its
own with event stamping on: stamping costs queue time).  Nothing is gated on
the times: the table goes to DESIGN.md as measured.

  python tools/jpeg_export_rate.py [--calls 20] [--out profiles/jpeg_export_rate.json]
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
        sys.exit("jpeg_export_rate: no GPU (a time is only ever measured on one)")
    dev = torch.device("cuda", 0)
    codec = myyuv_hip.Codec(0)
    st = torch.cuda.Stream(dev)  # explicit: handle 0 would mean the context's own stream
    sp = st.cuda_stream
    torch.cuda.set_stream(st)

    def ok(what):
        rc, bad = codec.sync_status(sp)
        if rc:
            sys.exit(f"jpeg_export_rate: {what} failed: {rc} at {bad}")

    def device_us(call, what):
        for _ in range(3):
            call()
        ok(what)
        out = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
        ok(what)
        return {"median": round(statistics.median(out), 1), "min": round(min(out), 1), "max": round(max(out), 1)}

    def host_ms(call):
        call()
        ts = []
        for _ in range(args.host_calls):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}

    g = myyuv_file.YUVFile.load(os.path.join(ROOT, "tests", "golden", "chef-with-trumpet-big-DCT-50.myyuv"))
    src = torch.frombuffer(bytearray(codec.decompress(g.data, g.width, g.height, tuple(g.params))),
                           dtype=torch.uint8).to(dev)
    big = synth.tiled_frame_torch(src, g.width, g.height, args.size, args.size).contiguous()

    def one(name, w, h, q, d_pay, d_size):
        cap = d_pay.numel()
        nbytes = int(d_size.item())
        d_rq = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_srq = torch.zeros(1, dtype=torch.int32, device=dev)
        d_jpg = torch.empty(nbytes + 4096, dtype=torch.uint8, device=dev)  # a picture's file is below its stream
        d_sjpg = torch.zeros(1, dtype=torch.int32, device=dev)
        d_frame = torch.empty(w * h * 3 // 2, dtype=torch.uint8, device=dev)

        def export():
            codec.to_jpeg_device(d_pay.data_ptr(), d_size.data_ptr(), cap, 1, w, h, q, d_jpg.data_ptr(),
                                 d_jpg.numel(), d_sjpg.data_ptr(), sp)

        def requant():
            codec.requantize_device(d_pay.data_ptr(), d_size.data_ptr(), cap, 1, w, h, q, q, d_rq.data_ptr(), cap,
                                    d_srq.data_ptr(), sp)

        def dec():
            codec.decompress_device(d_pay.data_ptr(), d_size.data_ptr(), cap, w, h, q, d_frame.data_ptr(), sp)

        res = {"frame": name, "quality": list(q), "calls": args.calls, "device_us": {}, "host_ms": {}}
        du = res["device_us"]
        du["requantize_device_q_to_q"] = device_us(requant, "requantize")
        du["decompress_device"] = device_us(dec, "decompress")
        du["to_jpeg_device"] = device_us(export, "to_jpeg")
        du["requantize_device_q_to_q_again"] = device_us(requant, "requantize")
        du["decompress_device_again"] = device_us(dec, "decompress")
        res["bytes"] = {"stream": nbytes, "jpeg": int(d_sjpg.item()), "requantized": int(d_srq.item())}
        res["bytes"]["jpeg_over_stream"] = round(res["bytes"]["jpeg"] / nbytes, 4)

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

        res["kernel_us"] = {"to_jpeg": split(export, "to_jpeg"), "requantize": split(requant, "requantize")}
        pay = d_pay[:nbytes].cpu().numpy()
        out = np.empty(cap, np.uint8)
        res["host_ms"]["requantize"] = host_ms(lambda: codec.requantize_into(pay, w, h, q, q, out))
        res["host_ms"]["to_jpeg"] = host_ms(lambda: codec.to_jpeg_into(pay, w, h, q, out))
        return res

    results = []
    for qv in (50, 90):
        q = (qv, qv, qv)
        w = h = args.size
        cap = myyuv_hip.payload_bound(w, h)
        d_pay = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_size = torch.zeros(1, dtype=torch.int32, device=dev)
        codec.compress_device(big.data_ptr(), w, h, q, d_pay.data_ptr(), cap, d_size.data_ptr(), sp)
        ok(f"compress q{qv}")
        results.append(one(f"{w}x{h} tiled", w, h, q, d_pay, d_size))
        del d_pay
    cap = (len(g.data) + 3) & ~3
    d_pay = torch.frombuffer(bytearray(g.data) + bytearray(cap - len(g.data)), dtype=torch.uint8).to(dev)
    d_size = torch.tensor([len(g.data)], dtype=torch.int32, device=dev)
    results.append(one(f"{g.width}x{g.height} chef-big", g.width, g.height, tuple(g.params), d_pay, d_size))

    line = json.dumps({"results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Downscale against decompress_scaled + compress, on one stream of one process.

The frame is the 8192x8192 tiled frame (SURVEY.md §8d generator from the
decoded chef-big golden), built and compressed at q50 on the GPU.  For denom
2, 4 and 8, device-resident, after 3 warm-up calls, each measurement bracketed
by HIP events on the calls' stream, the median (min - max) of --calls:
  * decompress_scaled_device followed by compress_device of the small frame at
    q_dst (unchanged code: the yardstick of the same run), as one bracket and
    each call alone,
  * downscale_device (the new path),
  * the yardstick again, after the new path: its spread within the run.
Then the host-buffer forms (pageable buffers, PCIe both ways, wall clock, the
median of --host-calls): downscale_into against decompress_scaled_into +
compress_into, the small frame downloaded and uploaded again in between.

Recorded besides: the payload sizes, that the two paths' streams are equal
byte for byte, and the per-kernel split of both paths from kernel_stats (a
separate loop of --calls calls with event stamping on: stamping costs queue
time, so the split is not taken from the timed calls).  Nothing is gated on
the times: the table goes to DESIGN.md as measured.

  python tools/downscale_rate.py [--size 8192] [--calls 20] [--out FILE.json]
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
        sys.exit("downscale_rate: no GPU (a time is only ever measured on one)")
    dev = torch.device("cuda", 0)
    w = h = args.size
    qs = qd = (50, 50, 50)
    codec = myyuv_hip.Codec(0)
    st = torch.cuda.Stream(dev)  # explicit: handle 0 would mean the context's own stream
    sp = st.cuda_stream
    torch.cuda.set_stream(st)

    def ok(what):
        rc, bad = codec.sync_status(sp)
        if rc:
            sys.exit(f"downscale_rate: {what} failed: {rc} at {bad}")

    g = myyuv_file.YUVFile.load(os.path.join(ROOT, "tests", "golden", "chef-with-trumpet-big-DCT-50.myyuv"))
    src = torch.frombuffer(bytearray(codec.decompress(g.data, g.width, g.height, tuple(g.params))),
                           dtype=torch.uint8).to(dev)
    d_orig = synth.tiled_frame_torch(src, g.width, g.height, w, h).contiguous()
    cap = myyuv_hip.payload_bound(w, h)
    d_src = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_ssrc = torch.zeros(1, dtype=torch.int32, device=dev)
    codec.compress_device(d_orig.data_ptr(), w, h, qs, d_src.data_ptr(), cap, d_ssrc.data_ptr(), sp)
    ok("compress q50")
    nsrc = int(d_ssrc.item())
    pay = d_src[:nsrc].cpu().numpy()

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

    def host_ms(call):
        call()
        ts = []
        for _ in range(args.host_calls):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}

    res = {"frame": f"{w}x{h} tiled, q50 -> q50", "source_bytes": nsrc, "calls": args.calls,
           "host_calls": args.host_calls, "denoms": {}}
    for denom in (2, 4, 8):
        sw, sh = w // denom, h // denom
        scap = myyuv_hip.payload_bound(sw, sh)
        d_small = torch.empty(sw * sh * 3 // 2, dtype=torch.uint8, device=dev)
        d_two = torch.empty(scap, dtype=torch.uint8, device=dev)  # decompress_scaled + compress
        d_stwo = torch.zeros(1, dtype=torch.int32, device=dev)
        d_one = torch.empty(scap, dtype=torch.uint8, device=dev)  # downscale
        d_sone = torch.zeros(1, dtype=torch.int32, device=dev)

        def dec():
            codec.decompress_scaled_device(d_src.data_ptr(), d_ssrc.data_ptr(), cap, 1, w, h, qs, denom,
                                           d_small.data_ptr(), sp)

        def comp():
            codec.compress_device(d_small.data_ptr(), sw, sh, qd, d_two.data_ptr(), scap, d_stwo.data_ptr(), sp)

        def both():
            dec()
            comp()

        def down():
            codec.downscale_device(d_src.data_ptr(), d_ssrc.data_ptr(), cap, 1, w, h, qs, denom, qd,
                                   d_one.data_ptr(), scap, d_sone.data_ptr(), sp)

        r = {"output": f"{sw}x{sh}", "device_us": {}, "host_ms": {}}
        du = r["device_us"]
        du["decompress_scaled_then_compress"] = device_us(both, "decompress_scaled + compress")
        du["decompress_scaled_device"] = device_us(dec, "decompress_scaled")
        du["compress_device"] = device_us(comp, "compress")
        du["downscale_device"] = device_us(down, "downscale")
        du["decompress_scaled_then_compress_again"] = device_us(both, "decompress_scaled + compress")
        n1, n2 = int(d_sone.item()), int(d_stwo.item())
        r["payload_bytes"] = {"downscale": n1, "decompress_scaled_then_compress": n2}
        r["streams_equal"] = bool(n1 == n2 and torch.equal(d_one[:n1], d_two[:n2]))
        r["kernel_us"] = {"downscale": split(down, "downscale"),
                          "decompress_scaled_then_compress": split(both, "decompress_scaled + compress")}
        small = np.empty(sw * sh * 3 // 2, np.uint8)
        out = np.empty(scap, np.uint8)

        def host_both():
            codec.decompress_scaled_into(pay, w, h, qs, denom, small)
            codec.compress_into(small, sw, sh, qd, out)

        r["host_ms"]["decompress_scaled_then_compress"] = host_ms(host_both)
        r["host_ms"]["downscale"] = host_ms(lambda: codec.downscale_into(pay, w, h, qs, denom, qd, out))
        r["host_ms"]["decompress_scaled_then_compress_again"] = host_ms(host_both)
        res["denoms"][f"1/{denom}"] = r

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()

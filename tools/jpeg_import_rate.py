#!/usr/bin/env python3
"""Import from JPEG against requantise and the export, on one stream of one process.

Frames: the 4032x3008 chef-big golden stream (q50) and its decode compressed
at q90, and the 8192x8192 tiled frame (SURVEY.md §8d generator) at q50 and
q90.  Each stream is exported on the GPU (three non-interleaved scans, Ri = 64
blocks); that file is the import's input.  Per frame, device-resident, after 3
warm-up calls, each measurement bracketed by HIP events on the calls' stream,
min / median / max of --calls:
  * from_jpeg_device (the new path: k_jpeg_import, then the encoder from K2 on),
  * requantize_device q -> q of the same stream (the same back half behind
    another front; unchanged code: the yardstick of the same run), before and
    after the new path's measurement.
Then the host-buffer form (pageable buffers, PCIe both ways, wall clock):
from_jpeg_into against to_jpeg_into, and the per-kernel split from
kernel_stats (a loop of its own with event stamping on).  import(export(s))
== s is checked on every frame.

--libjpeg FILE / --restartless FILE: two files of ONE picture written by
libjpeg (one interleaved scan), with a restart per MCU row and with none: the
poorly parallel case (a lane per MCU row) next to the host-decode fallback,
host-buffer calls, wall clock, with the host's share (inspect and, for the
fallback, the Huffman decode) taken from the kernels' sum.  Nothing is gated on
the times: the table goes to DESIGN.md as measured.

  python tools/jpeg_import_rate.py [--calls 20] [--out profiles/jpeg_import_rate.json]
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
    ap.add_argument("--libjpeg", default=None)
    ap.add_argument("--restartless", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import myyuv_file
    import myyuv_hip
    import synth

    if not torch.cuda.is_available():
        sys.exit("jpeg_import_rate: no GPU (a time is only ever measured on one)")
    dev = torch.device("cuda", 0)
    codec = myyuv_hip.Codec(0)
    st = torch.cuda.Stream(dev)  # explicit: handle 0 would mean the context's own stream
    sp = st.cuda_stream
    torch.cuda.set_stream(st)

    def ok(what):
        rc, bad = codec.sync_status(sp)
        if rc:
            sys.exit(f"jpeg_import_rate: {what} failed: {rc} at {bad}")

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

    def split(call, what, calls, sync=True):
        codec.profile(True)
        try:
            for _ in range(calls):
                call()
            if sync:
                ok(what)
            stats = codec.kernel_stats()
        finally:
            codec.profile(False)
        return {k: round(ms * 1e3 / calls, 1) for k, (ms, n) in stats.items() if n}

    g = myyuv_file.YUVFile.load(os.path.join(ROOT, "tests", "golden", "chef-with-trumpet-big-DCT-50.myyuv"))
    src = torch.frombuffer(bytearray(codec.decompress(g.data, g.width, g.height, tuple(g.params))),
                           dtype=torch.uint8).to(dev)
    big = synth.tiled_frame_torch(src, g.width, g.height, args.size, args.size).contiguous()

    def one(name, w, h, q, d_pay, d_size):
        cap = d_pay.numel()
        nbytes = int(d_size.item())
        pay = d_pay[:nbytes].cpu().numpy()
        jpg = np.empty(nbytes + 4096, np.uint8)
        nj = codec.to_jpeg_into(pay, w, h, q, jpg)
        jpg = jpg[:nj].copy()
        info = myyuv_hip.jpeg_inspect(jpg)
        d_jpg = torch.frombuffer(bytearray(jpg.tobytes()) + bytearray(-nj % 4), dtype=torch.uint8).to(dev)
        d_rq = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_srq = torch.zeros(1, dtype=torch.int32, device=dev)
        d_in = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_sin = torch.zeros(1, dtype=torch.int32, device=dev)

        def imp():
            codec.from_jpeg_device(d_jpg.data_ptr(), jpg, d_in.data_ptr(), cap, d_sin.data_ptr(), None, sp)

        def requant():
            codec.requantize_device(d_pay.data_ptr(), d_size.data_ptr(), cap, 1, w, h, q, q, d_rq.data_ptr(), cap,
                                    d_srq.data_ptr(), sp)

        res = {"frame": name, "quality": list(q), "calls": args.calls, "segments": info["segments"],
               "device_us": {}, "host_ms": {}}
        du = res["device_us"]
        du["requantize_device_q_to_q"] = device_us(requant, "requantize")
        du["from_jpeg_device"] = device_us(imp, "from_jpeg")
        du["requantize_device_q_to_q_again"] = device_us(requant, "requantize")
        got = d_in[:int(d_sin.item())].cpu().numpy()
        res["identity"] = bool(got.nbytes == nbytes and (got == pay).all())
        res["bytes"] = {"stream": nbytes, "jpeg": int(nj)}
        res["kernel_us"] = {"from_jpeg": split(imp, "from_jpeg", args.calls),
                            "requantize": split(requant, "requantize", args.calls)}
        out = np.empty(cap, np.uint8)
        res["host_ms"]["to_jpeg"] = host_ms(lambda: codec.to_jpeg_into(pay, w, h, q, out))
        res["host_ms"]["from_jpeg"] = host_ms(lambda: codec.from_jpeg_into(jpg, out))
        res["host_ms"]["inspect_alone"] = host_ms(lambda: myyuv_hip.jpeg_inspect(jpg))
        return res

    results = []
    cap = myyuv_hip.payload_bound(g.width, g.height)
    d_pay = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_pay[:len(g.data)] = torch.frombuffer(bytearray(g.data), dtype=torch.uint8).to(dev)
    d_size = torch.tensor([len(g.data)], dtype=torch.int32, device=dev)
    results.append(one(f"{g.width}x{g.height} chef-big", g.width, g.height, tuple(g.params), d_pay, d_size))
    codec.compress_device(src.data_ptr(), g.width, g.height, (90, 90, 90), d_pay.data_ptr(), cap, d_size.data_ptr(), sp)
    ok("compress q90")
    results.append(one(f"{g.width}x{g.height} chef-big", g.width, g.height, (90, 90, 90), d_pay, d_size))
    del d_pay
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

    libjpeg = []
    streams = []
    for path in (args.libjpeg, args.restartless):
        if not path:
            continue
        data = np.frombuffer(open(path, "rb").read(), np.uint8).copy()
        info = myyuv_hip.jpeg_inspect(data)
        out = np.empty(info["payload_bound"], np.uint8)
        n = codec.from_jpeg_into(data, out)[0]
        streams.append(out[:n].tobytes())
        r = {"file": os.path.basename(path), "bytes": int(data.nbytes), "stream_bytes": int(n),
             "size": [info["width"], info["height"]], "segments": info["segments"], "on_gpu": info["on_gpu"],
             "host_ms": {"from_jpeg": host_ms(lambda: codec.from_jpeg_into(data, out)),
                         "inspect_alone": host_ms(lambda: myyuv_hip.jpeg_inspect(data))},
             "kernel_us": split(lambda: codec.from_jpeg_into(data, out), "from_jpeg", args.host_calls, sync=False)}
        libjpeg.append(r)
    line = json.dumps({"results": results, "libjpeg": libjpeg,
                       "libjpeg_streams_equal": len(set(streams)) == 1 if len(streams) == 2 else None})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Crop and join against the decode / encode paths they replace, on one
stream of one process.

The frame is the 8192x8192 tiled q50 frame (SURVEY.md §8d generator from the
decoded chef-big golden; BASELINE.json configs[2]), built and compressed on
the GPU.  Device-resident, after 3 warm-up calls, each call bracketed by HIP
events on the call's stream, the median of --calls calls:
  * crop_device of the 1920x1088 centre window and of the whole frame (the
    identity), next to decompress_region_device of the same rectangle and to
    decompress_device + compress_device of the frame;
  * join_device of 4 x 4 tiles of 2048x2048 (crops of the frame, so the
    result is the frame's own stream), next to compress_device of the frame.
Then k_stream_gather's bytes read plus bytes written per second on the
identity crop, with k_stream_out's rate on the same frame in the same run
(kernel execution times from kernel_stats; k_stream_out does the same job
from K2's tiles).  Then the host-buffer forms (pageable buffers, PCIe both
ways, wall clock).

  python tools/gather_rate.py [--size 8192] [--calls 20] [--out FILE.json]
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
        sys.exit("gather_rate: no GPU (a time is only ever measured on one)")
    dev = torch.device("cuda", 0)
    w = h = args.size
    q = (50, 50, 50)
    codec = myyuv_hip.Codec(0)
    st = torch.cuda.Stream(dev)  # explicit: handle 0 would mean the context's own stream
    sp = st.cuda_stream
    torch.cuda.set_stream(st)

    def ok(what):
        rc, bad = codec.sync_status(sp)
        if rc:
            sys.exit(f"gather_rate: {what} failed: {rc} at {bad}")

    g = myyuv_file.YUVFile.load(os.path.join(ROOT, "tests", "golden", "chef-with-trumpet-big-DCT-50.myyuv"))
    src = torch.frombuffer(bytearray(codec.decompress(g.data, g.width, g.height, tuple(g.params))),
                           dtype=torch.uint8).to(dev)
    d_in = synth.tiled_frame_torch(src, g.width, g.height, w, h).contiguous()
    cap = myyuv_hip.payload_bound(w, h)
    d_pay = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_size = torch.zeros(1, dtype=torch.int32, device=dev)
    codec.compress_device(d_in.data_ptr(), w, h, q, d_pay.data_ptr(), cap, d_size.data_ptr(), sp)
    ok("compress")
    size = int(d_size.item())
    d_frame = torch.empty(w * h * 3 // 2, dtype=torch.uint8, device=dev)
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_osz = torch.zeros(1, dtype=torch.int32, device=dev)
    d_pay2 = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_size2 = torch.zeros(1, dtype=torch.int32, device=dev)

    window = centred(w, min(1920, w), min(1088, h))
    whole = (0, 0, w, h)

    def crop(rg):
        return lambda: codec.crop_device(d_pay.data_ptr(), d_size.data_ptr(), cap, 1, w, h, rg, d_out.data_ptr(), cap,
                                         d_osz.data_ptr(), sp)

    def region(rg):
        return lambda: codec.decompress_region_device(d_pay.data_ptr(), d_size.data_ptr(), cap, 1, w, h, q, rg,
                                                      d_frame.data_ptr(), sp)

    def recompress():
        codec.decompress_device(d_pay.data_ptr(), d_size.data_ptr(), cap, w, h, q, d_frame.data_ptr(), sp)
        codec.compress_device(d_frame.data_ptr(), w, h, q, d_pay2.data_ptr(), cap, d_size2.data_ptr(), sp)

    def compress():
        codec.compress_device(d_in.data_ptr(), w, h, q, d_pay2.data_ptr(), cap, d_size2.data_ptr(), sp)

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

    res = {"frame": f"{w}x{h} tiled q50", "payload_bytes": size, "calls": args.calls, "device_us": {}, "host_ms": {}}
    dv = res["device_us"]
    dv["crop_window"] = dict(device_us(crop(window), "crop"), region=list(window), out_bytes=int(d_osz.item()))
    dv["decompress_region_window"] = device_us(region(window), "region decode")
    dv["crop_whole"] = device_us(crop(whole), "crop")
    identity = int(d_osz.item()) == size and bool(torch.equal(d_out[:size], d_pay[:size]))
    dv["crop_whole"]["equals_source"] = identity
    if not identity:
        sys.exit("gather_rate: the whole-frame crop is not the source stream")
    dv["decompress_region_whole"] = device_us(region(whole), "region decode")
    dv["decompress_plus_compress"] = device_us(recompress, "decompress + compress")

    # join: 4 x 4 tiles, each a crop of the frame, side by side in one device array
    cols = rows = 4
    tw, th = w // cols, h // rows
    tcap = myyuv_hip.payload_bound(tw, th)
    d_tiles = torch.zeros(cols * rows * tcap, dtype=torch.uint8, device=dev)
    d_tsz = torch.zeros(cols * rows, dtype=torch.int32, device=dev)
    for t in range(cols * rows):
        codec.crop_device(d_pay.data_ptr(), d_size.data_ptr(), cap, 1, w, h, ((t % cols) * tw, (t // cols) * th, tw, th),
                          d_tiles.data_ptr() + t * tcap, tcap, d_tsz.data_ptr() + 4 * t, sp)
    ok("tile crops")

    def join():
        codec.join_device(d_tiles.data_ptr(), d_tsz.data_ptr(), tcap, cols, rows, tw, th, d_out.data_ptr(), cap,
                          d_osz.data_ptr(), sp)

    dv["join_4x4"] = device_us(join, "join")
    same = int(d_osz.item()) == size and bool(torch.equal(d_out[:size], d_pay[:size]))
    dv["join_4x4"]["equals_source"] = same
    if not same:
        sys.exit("gather_rate: the join of the frame's 16 crops is not the frame's stream")
    dv["compress_device"] = device_us(compress, "compress")

    # the two stream movers, per byte: kernel execution times of the same run
    nblk = (w // 8) * (h // 8) + 2 * (w // 16) * (h // 16)
    content = size - 36 - nblk

    def kernel_us(name, call, what):
        codec.profile(True, [name])
        try:
            for _ in range(args.calls):
                call()
            ok(what)
            ms, n = codec.kernel_stats()[name]
        finally:
            codec.profile(False)
        return ms * 1e3 / n

    tg = kernel_us("stream_gather", crop(whole), "crop")
    to = kernel_us("stream_out", compress, "compress")
    # both kernels read and write every content byte and every size byte once
    moved = 2 * (content + nblk)
    res["stream_movers"] = {
        "bytes_read_plus_written": moved,
        "k_stream_gather_us": round(tg, 1), "k_stream_gather_GBps": round(moved / tg / 1e3, 1),
        "k_stream_out_us": round(to, 1), "k_stream_out_GBps": round(moved / to / 1e3, 1),
    }

    # host buffers (PCIe included)
    pay = d_pay[:size].cpu().numpy()
    out = np.empty(size + 64, np.uint8)
    frame = np.empty(w * h * 3 // 2, np.uint8)
    tiles = [d_tiles[t * tcap:t * tcap + int(n)].cpu().numpy().tobytes() for t, n in enumerate(d_tsz.cpu().tolist())]

    def host_ms(call):
        call()
        ts = []
        for _ in range(args.host_calls):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}

    hm = res["host_ms"]
    hm["crop_window"] = host_ms(lambda: codec.crop_into(pay, w, h, window, out))
    hm["decompress_region_window"] = host_ms(lambda: codec.decompress_region_into(pay, w, h, q, window, frame))
    hm["crop_whole"] = host_ms(lambda: codec.crop_into(pay, w, h, whole, out))
    hm["join_4x4"] = host_ms(lambda: codec.join_into(tiles, cols, rows, tw, th, out))
    hm["decompress"] = host_ms(lambda: codec.decompress_into(pay, w, h, q, frame))

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()

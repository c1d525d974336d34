#!/usr/bin/env python3
"""Compare against decode + raw compare, on one stream of one process; and the
fidelity of requantise and transform, in figures.

The frame is the 8192x8192 tiled q50 frame (SURVEY.md §8d generator from the
decoded chef-big golden; BASELINE.json configs[2]), built and compressed on
the GPU.  Device-resident, after 3 warm-up calls, each call bracketed by HIP
events on the call's stream, the median of --calls calls (min and max kept):
  (a) decompress_device (the full decode),
  (b) compare_frames_device of the decoded frame against the original
      (k_frame_compare, with the map),
  (c) compare_stream_device of the stream against the original, with the map
      (k_decode_compare: the decoded frame never exists),
  (d) the same without the map,
then (a) again: the spread of the yardstick within the run.  (c) is checked
once, not timed, to return the integers of (a) then (b).
Host buffers (pageable, PCIe, wall clock, median of --host-calls):
  (e) compare_stream against decompress_into with its download.
Nothing is gated on the times: the table goes to DESIGN.md §4 as measured.

Untimed, the same frame as the original: PSNR and block SSIM of
  * compress at q50, and requantise of the q90 stream to q50;
  * transform rot90 of the q50 stream, and decode - rotate - encode at q50,
    both against the rotated original.

  python tools/metric_rate.py [--size 8192] [--calls 20] [--out FILE.json]
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
        sys.exit("metric_rate: no GPU (a time is only ever measured on one)")
    dev = torch.device("cuda", 0)
    w = h = args.size
    q50, q90 = (50, 50, 50), (90, 90, 90)
    nblk = (w // 8) * (h // 8) + 2 * (w // 16) * (h // 16)
    fbytes = w * h * 3 // 2
    codec = myyuv_hip.Codec(0)
    st = torch.cuda.Stream(dev)  # explicit: handle 0 would mean the context's own stream
    sp = st.cuda_stream
    torch.cuda.set_stream(st)

    def ok(what):
        rc, bad = codec.sync_status(sp)
        if rc:
            sys.exit(f"metric_rate: {what} failed: {rc} at {bad}")

    g = myyuv_file.YUVFile.load(os.path.join(ROOT, "tests", "golden", "chef-with-trumpet-big-DCT-50.myyuv"))
    src = torch.frombuffer(bytearray(codec.decompress(g.data, g.width, g.height, tuple(g.params))),
                           dtype=torch.uint8).to(dev)
    d_in = synth.tiled_frame_torch(src, g.width, g.height, w, h).contiguous()
    cap = myyuv_hip.payload_bound(w, h)

    def compress(d_frame, fw, fh, q):
        d_pay = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_size = torch.zeros(1, dtype=torch.int32, device=dev)
        codec.compress_device(d_frame.data_ptr(), fw, fh, q, d_pay.data_ptr(), cap, d_size.data_ptr(), sp)
        ok("compress")
        return d_pay, d_size

    d_pay, d_size = compress(d_in, w, h, q50)
    size = int(d_size.item())
    d_full = torch.empty(fbytes, dtype=torch.uint8, device=dev)
    d_rec = torch.zeros(72, dtype=torch.uint8, device=dev)
    d_map = torch.zeros(nblk * 8, dtype=torch.uint8, device=dev)

    def records():
        r = d_rec.cpu().numpy().view([("sse", "<u8"), ("ssim_sum", "<i8"), ("nblocks", "<u4"), ("max_abs", "<u4")])
        return tuple(tuple(int(v) for v in r[p].tolist()) for p in range(3))

    def full():
        codec.decompress_device(d_pay.data_ptr(), d_size.data_ptr(), cap, w, h, q50, d_full.data_ptr(), sp)

    def frames():
        codec.compare_frames_device(d_in.data_ptr(), d_full.data_ptr(), 1, 1, w, h, d_rec.data_ptr(), d_map.data_ptr(),
                                    sp)

    def fused(with_map):
        return lambda: codec.compare_stream_device(d_pay.data_ptr(), d_size.data_ptr(), cap, 1, w, h, q50,
                                                   d_in.data_ptr(), 1, d_rec.data_ptr(),
                                                   d_map.data_ptr() if with_map else None, sp)

    def device_us(call):
        for _ in range(3):
            call()
        ok("warm-up")
        out = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
        ok("a timed call")
        return {"median": round(statistics.median(out), 1), "min": round(min(out), 1), "max": round(max(out), 1)}

    res = {"frame": f"{w}x{h} tiled q50", "payload_bytes": size, "blocks": nblk, "calls": args.calls,
           "device_us": {}, "host_ms": {}, "fidelity": {}}
    du = res["device_us"]
    du["a_decompress_device"] = device_us(full)
    du["b_compare_frames_device_map"] = device_us(frames)
    ok("compare_frames")
    unfused = (records(), d_map.clone())
    du["c_compare_stream_device_map"] = device_us(fused(True))
    if records() != unfused[0] or not torch.equal(d_map, unfused[1]):
        sys.exit("metric_rate: the fused compare differs from decode + compare_frames")
    du["d_compare_stream_device_no_map"] = device_us(fused(False))
    if records() != unfused[0]:
        sys.exit("metric_rate: the fused compare without a map differs")
    du["a_decompress_device_again"] = device_us(full)
    ab = du["a_decompress_device"]["median"] + du["b_compare_frames_device_map"]["median"]
    spread = max(du[k]["max"] - du[k]["min"] for k in du)
    res["a_plus_b_us"] = round(ab, 1)
    res["largest_spread_us"] = round(spread, 1)
    res["c_below_a_plus_b_by_us"] = round(ab - du["c_compare_stream_device_map"]["median"], 1)

    # host buffers (PCIe included)
    pay = d_pay[:size].cpu().numpy()
    ref = d_in.cpu().numpy()
    out = np.empty(fbytes, np.uint8)

    def host_ms(call):
        call()
        ts = []
        for _ in range(args.host_calls):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}

    res["host_ms"]["decompress_into"] = host_ms(lambda: codec.decompress_into(pay, w, h, q50, out))
    res["host_ms"]["e_compare_stream"] = host_ms(lambda: codec.compare_stream(pay, w, h, q50, ref))
    if codec.compare_stream(pay, w, h, q50, ref) != unfused[0]:
        sys.exit("metric_rate: the host-buffer compare differs from the device one")

    # ---- fidelity, untimed: every stream against the frame it was made from
    def figures(d_stream, d_stream_size, fw, fh, q, d_orig):
        codec.compare_stream_device(d_stream.data_ptr(), d_stream_size.data_ptr(), cap, 1, fw, fh, q,
                                    d_orig.data_ptr(), 1, d_rec.data_ptr(), None, sp)
        ok("compare")
        r = records()
        sse, ss, nb = sum(p[0] for p in r), sum(p[1] for p in r), sum(p[2] for p in r)
        return {"psnr_db": round(myyuv_hip.metric_psnr(sse, fbytes), 4), "ssim": round(myyuv_hip.metric_ssim(ss, nb), 6),
                "psnr_y_db": round(myyuv_hip.metric_psnr(r[0][0], fw * fh), 4),
                "ssim_y": round(myyuv_hip.metric_ssim(r[0][1], r[0][2]), 6),
                "bytes": int(d_stream_size.item()), "records": r}

    fid = res["fidelity"]
    fid["compress_q50"] = figures(d_pay, d_size, w, h, q50, d_in)
    d_p90, d_s90 = compress(d_in, w, h, q90)
    fid["compress_q90"] = figures(d_p90, d_s90, w, h, q90, d_in)
    d_rq = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_rqs = torch.zeros(1, dtype=torch.int32, device=dev)
    codec.requantize_device(d_p90.data_ptr(), d_s90.data_ptr(), cap, 1, w, h, q90, q50, d_rq.data_ptr(), cap,
                            d_rqs.data_ptr(), sp)
    ok("requantize")
    fid["requantize_q90_to_q50"] = figures(d_rq, d_rqs, w, h, q50, d_in)

    def rot90(d_frame, fw, fh):  # clockwise, per plane (MYYUV_XF_ROT90: numpy's rot90(a, -1))
        y = d_frame[: fw * fh].view(fh, fw)
        u = d_frame[fw * fh: fw * fh * 5 // 4].view(fh // 2, fw // 2)
        v = d_frame[fw * fh * 5 // 4:].view(fh // 2, fw // 2)
        return torch.cat([torch.rot90(p, -1, (0, 1)).reshape(-1) for p in (y, u, v)]).contiguous()

    d_rot = rot90(d_in, w, h)
    d_xf = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_xfs = torch.zeros(1, dtype=torch.int32, device=dev)
    codec.transform_device(d_pay.data_ptr(), d_size.data_ptr(), cap, 1, w, h, q50, myyuv_hip.XF_ROT90, q50,
                           d_xf.data_ptr(), cap, d_xfs.data_ptr(), sp)
    ok("transform")
    fid["transform_rot90_q50"] = figures(d_xf, d_xfs, h, w, q50, d_rot)
    full()
    ok("decompress")
    d_re, d_res = compress(rot90(d_full, w, h), h, w, q50)
    fid["decode_rotate_encode_q50"] = figures(d_re, d_res, h, w, q50, d_rot)

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh_:
            fh_.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()

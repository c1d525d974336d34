#!/usr/bin/env python3
"""Probe and encode to a target against the long route, on one stream of one
process.

The frame is the 8192x8192 tiled q50 frame (SURVEY.md §8d generator from the
decoded chef-big golden; BASELINE.json configs[2]), built on the GPU.
Device-resident, after 3 warm-up calls, each call bracketed by HIP events on
the call's stream, the median of --calls calls (min and max kept), at q50:
  (a) probe_device, the size part   (K1 -> K2 -> tile scan; no stream writer)
  (b) probe_device, the metric part (K1 -> coef_compare -> metric_reduce; no Huffman stage)
  (c) probe_device, both parts      (K1 once)
  (d) compress_device
  (e) compress_device, then compare_stream_device of its stream against the frame
then (d) again: the spread of the yardstick within the run.  (c) is checked
once, not timed, to return the size of (d) and the integers of (e).
The searches block (they read each probe back), so they are timed by the wall
clock, the median of --search-calls calls, device buffers on both sides:
  (f) compress_to_size_device, budget = the q50 size, against a host loop that
      runs the same bisection with compress_device and a read of the size;
  (g) compress_to_sse_device, each plane's floor its own PSNR at q50 or at
      q100, whichever is lower (this frame is a decoded q50 image: q50
      reproduces it better than q100 does, so q50's figure alone is out of
      reach of the search's first probe), against a host loop with
      compress_device, compare_stream_device and a read of the records.
Both loops end, as the entry points do, with the figures and the payload of the
chosen qualities.  Nothing is gated on the times: the table goes to DESIGN.md
as measured.

  python tools/target_rate.py [--size 8192] [--calls 20] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yuv-manipulations-2_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--search-calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import myyuv_file
    import myyuv_hip
    import ratesearchref as S
    import synth

    if not torch.cuda.is_available():
        sys.exit("target_rate: no GPU (a time is only ever measured on one)")
    dev = torch.device("cuda", 0)
    w = h = args.size
    q50 = (50, 50, 50)
    nblk = (w // 8) * (h // 8) + 2 * (w // 16) * (h // 16)
    samples = (w * h, w * h // 4, w * h // 4)
    codec = myyuv_hip.Codec(0)
    st = torch.cuda.Stream(dev)  # explicit: handle 0 would mean the context's own stream
    sp = st.cuda_stream
    torch.cuda.set_stream(st)

    def ok(what):
        rc, bad = codec.sync_status(sp)
        if rc:
            sys.exit(f"target_rate: {what} failed: {rc} at {bad}")

    g = myyuv_file.YUVFile.load(os.path.join(ROOT, "tests", "golden", "chef-with-trumpet-big-DCT-50.myyuv"))
    src = torch.frombuffer(bytearray(codec.decompress(g.data, g.width, g.height, tuple(g.params))),
                           dtype=torch.uint8).to(dev)
    d_in = synth.tiled_frame_torch(src, g.width, g.height, w, h).contiguous()
    cap = myyuv_hip.payload_bound(w, h)
    d_pay = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_size = torch.zeros(1, dtype=torch.int32, device=dev)
    d_rec = torch.zeros(72, dtype=torch.uint8, device=dev)
    d_probe = torch.zeros(88, dtype=torch.uint8, device=dev)

    def records(t=None):
        r = (d_rec if t is None else t).cpu().numpy().view([("sse", "<u8"), ("ssim_sum", "<i8"), ("nblocks", "<u4"),
                                                            ("max_abs", "<u4")])
        return tuple(tuple(int(v) for v in r[p].tolist()) for p in range(3))

    def probe(what, q=q50):
        return lambda: codec.probe_device(d_in.data_ptr(), 1, w, h, q, what, d_probe.data_ptr(), None, sp)

    def compress(q=q50):
        codec.compress_device(d_in.data_ptr(), w, h, q, d_pay.data_ptr(), cap, d_size.data_ptr(), sp)

    def compare(q=q50):
        codec.compare_stream_device(d_pay.data_ptr(), d_size.data_ptr(), cap, 1, w, h, q, d_in.data_ptr(), 1,
                                    d_rec.data_ptr(), None, sp)

    def compress_compare():
        compress()
        compare()

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

    res = {"frame": f"{w}x{h} tiled q50", "blocks": nblk, "calls": args.calls, "device_us": {}, "search_ms": {}}
    du = res["device_us"]
    du["a_probe_size"] = device_us(probe(myyuv_hip.PROBE_SIZE))
    du["b_probe_metric"] = device_us(probe(myyuv_hip.PROBE_METRIC))
    du["c_probe_both"] = device_us(probe(myyuv_hip.PROBE_SIZE | myyuv_hip.PROBE_METRIC))
    got = d_probe.cpu().numpy().view(myyuv_hip.PROBE_DTYPE)[0]
    du["d_compress_device"] = device_us(compress)
    du["e_compress_then_compare_stream"] = device_us(compress_compare)
    size50, rec50 = int(d_size.item()), records()
    if int(got["payload_bytes"]) != size50 or records(torch.from_numpy(got["metric"].view(np.uint8).copy())) != rec50:
        sys.exit("target_rate: the probe differs from compress then compare")
    du["d_compress_device_again"] = device_us(compress)
    res["payload_bytes_q50"] = size50
    res["records_q50"] = rec50
    res["b_below_e_by_us"] = round(du["e_compress_then_compare_stream"]["median"] - du["b_probe_metric"]["median"], 1)
    res["largest_spread_us"] = round(max(du[k]["max"] - du[k]["min"] for k in du), 1)

    # kernel times of one probe of both parts and of one compress (profiled apart from the timed calls)
    names = ["fdct_quant", "fdct_fix", "huff_encode", "huff_encode_wide", "huff_encode_r16", "huff_encode_wave",
             "scan_tiles", "stream_out", "coef_compare", "metric_reduce", "probe_out", "decode_compare"]
    for label, call in (("probe_both", probe(3)), ("compress_then_compare", compress_compare)):
        codec.profile(True, names)
        for _ in range(args.calls):
            call()
        ok(label)
        stats = codec.kernel_stats()
        codec.profile(False)
        res.setdefault("kernel_us", {})[label] = {k: round(v[0] * 1e3 / v[1], 1) for k, v in stats.items() if v[1]}

    # ---- the searches, wall clock
    def wall_ms(call):
        call()
        ts = []
        for _ in range(args.search_calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}

    last = {}

    def to_size():
        last["size"] = codec.compress_to_size_device(d_in.data_ptr(), w, h, size50, d_pay.data_ptr(), cap,
                                                     d_size.data_ptr(), sp)

    def loop_size():
        def size_of(q):
            compress((q, q, q))
            return int(d_size.item())

        okk, q, asked = S.size_search(size_of, size50)
        compress((q, q, q))
        compare((q, q, q))
        last["loop_size"] = (q, len(asked), int(d_size.item()), records())

    q100 = (100, 100, 100)
    compress(q100)
    compare(q100)
    ok("q100")
    rec100 = records()
    res["records_q100"] = rec100
    dbs = [myyuv_hip.metric_psnr(max(rec50[p][0], rec100[p][0]), samples[p]) for p in range(3)]
    ceil = [myyuv_hip.metric_sse_for_psnr(dbs[p], samples[p]) for p in range(3)]

    def to_sse():
        last["sse"] = codec.compress_to_sse_device(d_in.data_ptr(), w, h, ceil, d_pay.data_ptr(), cap,
                                                   d_size.data_ptr(), sp)

    def loop_sse():
        def sse_of(q3):
            compress(q3)
            compare(q3)
            return tuple(r[0] for r in records())

        okk, q3, failed, asked = S.sse_search(sse_of, ceil)
        compress(q3)
        compare(q3)
        last["loop_sse"] = (q3, len(asked), int(d_size.item()), records())

    sm = res["search_ms"]
    sm["f_compress_to_size_device"] = wall_ms(to_size)
    sm["f_host_loop_compress"] = wall_ms(loop_size)
    sm["g_compress_to_sse_device"] = wall_ms(to_sse)
    sm["g_host_loop_compress_compare"] = wall_ms(loop_sse)
    ok("the searches")
    for mine, loop in (("size", "loop_size"), ("sse", "loop_sse")):
        r, (q, n, size, recs) = last[mine], last[loop]
        q3 = (q, q, q) if isinstance(q, int) else tuple(q)
        if (r["quality"], r["probes"], r["at"][1], r["at"][2]) != (q3, n, size, recs):
            sys.exit(f"target_rate: the {mine} search differs from the host loop: {r} {last[loop]}")
    res["size_search"] = {"budget": size50, "quality": last["size"]["quality"], "probes": last["size"]["probes"]}
    res["psnr_search"] = {"floor_db": [round(v, 4) for v in dbs], "quality": last["sse"]["quality"], "probes": last["sse"]["probes"]}

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh_:
            fh_.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Diagnostic: the fused decoder's kernel time per launch, a wave per
256-block span (MYYUV_DECODER=span) against a wave per 64-block group
(MYYUV_DECODER=group), by batch size: chef-big q50 (4032x3008, 4,443 groups a
frame), kernels alone on the GPU, HIP events, three alternating rounds in one
process.  The crossover sets MYYUV_DEC_SPAN_MIN's default (codec_common.hpp
kDecSpanMinDefault, in 64-block groups per launch):
  python3 tools/dec_span_cross.py [batch sizes, default 1 2 4 8 16 32]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yuv-manipulations-2_amd")]


def main():
    import torch
    import myyuv_file
    import myyuv_hip
    from oracle import oracle as O

    sizes = [int(a) for a in sys.argv[1:]] or [1, 2, 4, 8, 16, 32]
    g = myyuv_file.YUVFile.load(os.path.join(ROOT, "tests", "golden", "chef-with-trumpet-big-DCT-50.myyuv"))
    w, h, q = g.width, g.height, (50, 50, 50)
    groups = sum(-(-n // 64) for n in ((w // 8) * (h // 8), (w // 16) * (h // 16), (w // 16) * (h // 16)))
    dev = torch.device("cuda", 0)
    codecs = {}
    for name in ("group", "span"):
        os.environ["MYYUV_DECODER"] = name
        codecs[name] = myyuv_hip.Codec(0)
    del os.environ["MYYUV_DECODER"]
    st = torch.cuda.Stream(dev)
    sp = st.cuda_stream
    fb = w * h * 3 // 2
    cap = (len(g.data) + 3 & ~3) + 64
    B = max(sizes)
    d_pay = torch.zeros(B * cap, dtype=torch.uint8, device=dev)
    one = torch.frombuffer(bytearray(g.data), dtype=torch.uint8).to(dev)
    for f in range(B):
        d_pay[f * cap: f * cap + len(g.data)] = one
    d_sz = torch.full((B,), len(g.data), dtype=torch.int32, device=dev)
    d_out = torch.empty(B * fb, dtype=torch.uint8, device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    want = torch.frombuffer(bytearray(O.decompress(g.data, w, h, q)), dtype=torch.uint8).to(dev)
    for b in sizes:
        res = {name: [] for name in codecs}
        for rnd in range(3):
            for name, c in codecs.items():
                c.reserve_batch(w, h, b)
                for it in range(2):
                    c.profile(it == 1, ["huff_decode"] if it else None)
                    for _ in range(20 if it else 3):
                        c.decompress_batch_device(d_pay.data_ptr(), d_sz.data_ptr(), cap, b, w, h, q,
                                                  d_out.data_ptr(), sp)
                    rc, bad = c.sync_status(sp)
                    assert rc == 0, (name, rc, bad)
                ms, n = c.kernel_stats()["huff_decode"]
                res[name].append(ms / n * 1e3)
                c.profile(False)
                assert torch.equal(d_out[(b - 1) * fb: b * fb], want), name
        print(f"frames {b:3d} groups {b * groups:7d}  " +
              "  ".join(f"{name} us " + " ".join(f"{v:8.1f}" for v in vs) for name, vs in res.items()), flush=True)
    for c in codecs.values():
        c.close()


if __name__ == "__main__":
    main()

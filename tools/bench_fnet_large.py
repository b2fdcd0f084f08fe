"""The layer road of the float32 network (edison_fnet_load_ex) measured:

  arch   train.get_model's conv_model and low_latency_conv at 31x13x1, 10 classes, which only the layer road runs: utterances/s of
         edison_fnet_batch_dev at --utts utterances between device events, then each record's kernel time between hipEvents
         (edison_fnet_profile_dev) with the f32 FLOP/s it implies -- 2 x live rows x K x out_c per utterance and record -- and, for a
         dense record over the LDS, the weight bytes its workgroups read per second (every M block of 128 utterances reads B once)
  road   what the road costs where the one-launch kernel runs too: kws_conv (tests/golden/cube_kws.ednf) loaded plain and loaded
         layered, on two contexts in one process, the legs alternating after a warm-up of each

    python tools/bench_fnet_large.py [--utts 8192] [--steps 10] [--warmup 3] [--rounds 5]

One JSON line per figure. Every figure is a single run of one process; run it under a time limit of its own.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32 = 157.3e12           # MI355X f32-input MFMA peak (FLOP/s)
MB = 128                      # ED_FNET_LAYER_MB (csrc/fnet.h): a workgroup's rows


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / steps


def records(m):
    """Per conv / dense record of model dict m: (live rows per utterance, K, out_c, k_pad x n_pad)."""
    from edison_amd import cube_import
    out = []
    for L in m["layers"]:
        if L["type"] != cube_import.T_CONV:
            continue
        (ih, iw, ic), (kh, kw), (sh, sw), cp = L["inp"], L["k"], L["s"], L.get("cpad", (0, 0, 0, 0))
        ch, cw = (ih + cp[0] + cp[2] - kh) // sh + 1, (iw + cp[1] + cp[3] - kw) // sw + 1
        K, oc = kh * kw * ic, L["out"][2]
        out.append((ch * cw, K, oc, (K + 3) // 4 * 4 * ((oc + 15) // 16 * 16)))
    return out


def bench_arch(arch, n, steps, warmup, dev, board):
    import torch
    from edison_amd import cube_import, train
    from edison_amd.context import Context
    m = train.get_model(arch, (31, 13, 1), 10)
    c = Context(0, model_path=None)
    try:
        c.fnet_load(cube_import.build_blob(m), large=True)
        info = c.fnet_info()
        assert info["layered"]
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        x = torch.randn((n, 403), generator=gen, device=dev) * 200
        lg, pr = (torch.empty((n, 10), dtype=torch.float32, device=dev) for _ in range(2))
        am = torch.empty(n, dtype=torch.int32, device=dev)
        c.use_torch_stream()
        sec = timed(lambda: c.fnet_t(x, n, lg, pr, am), steps, warmup)
        ms = np.mean([c.fnet_profile_t(x, n) for _ in range(steps)], axis=0)
        c.use_own_stream()
        rec = records(m)
        flops = sum(2.0 * live * K * oc for live, K, oc, _ in rec)
        print(json.dumps(dict(board=board, what="arch", arch=arch, utts=n, seconds=round(sec, 6), utts_per_s=round(n / sec, 1),
                              mflop_per_utt=round(flops / 1e6, 2), net_tflops=round(flops * n / sec / 1e12, 2),
                              share_of_f32_peak=round(flops * n / sec / PEAK_F32, 4), lds_bytes=info["lds_bytes"])), flush=True)
        for i, ((live, K, oc, wfl), t) in enumerate(zip(rec, ms)):
            row = dict(board=board, what="record", arch=arch, record=i, live_rows=live, K=K, out_c=oc, kernel_ms=round(float(t), 4),
                       tflops=round(2.0 * live * K * oc * n / (float(t) * 1e-3) / 1e12, 2))
            if live == 1 and wfl > 40960:
                row["weight_GB_per_s"] = round(-(-n // MB) * wfl * 4 / (float(t) * 1e-3) / 1e9, 1)
            print(json.dumps(row), flush=True)
        print(json.dumps(dict(board=board, what="softmax", arch=arch, kernel_ms=round(float(ms[-1]), 4), kernels_ms=round(float(ms.sum()), 4))), flush=True)
    finally:
        c.close()


def bench_road(n, steps, warmup, rounds, dev, board):
    import torch
    from edison_amd.context import Context
    fixture = os.path.join(ROOT, "tests", "golden", "cube_kws.ednf")
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    x = torch.randn((n, 403), generator=gen, device=dev) * 200
    legs = {}
    for leg in ("plain", "layered"):
        c = Context(0, model_path=None)
        c.fnet_load(fixture, layered=leg == "layered")
        c.use_torch_stream()
        out = (torch.empty((n, 10), dtype=torch.float32, device=dev), torch.empty((n, 10), dtype=torch.float32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev))
        legs[leg] = (c, out)
    try:
        run = {leg: (lambda c=c, out=out: c.fnet_t(x, n, *out)) for leg, (c, out) in legs.items()}
        for leg in run:
            timed(run[leg], warmup, warmup)
        times = {leg: [] for leg in run}
        for _ in range(rounds):
            for leg in run:
                times[leg].append(timed(run[leg], steps, 0))
        torch.cuda.synchronize()
        same = all(bool((a == b).all()) for a, b in zip(legs["plain"][1], legs["layered"][1]))
        med = {leg: float(np.median(t)) for leg, t in times.items()}
        print(json.dumps(dict(board=board, what="road", network="kws_conv", utts=n, outputs_identical=same,
                              plain_ms=[round(t * 1e3, 4) for t in times["plain"]], layered_ms=[round(t * 1e3, 4) for t in times["layered"]],
                              plain_utts_per_s=round(n / med["plain"], 1), layered_utts_per_s=round(n / med["layered"], 1),
                              layered_over_plain=round(med["layered"] / med["plain"], 3))), flush=True)
    finally:
        for c, _ in legs.values():
            c.use_own_stream()
            c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    from edison_amd.context import Context
    dev = torch.device("cuda", 0)
    c = Context(0, model_path=None)
    board = c.device_info()["name"]
    c.close()
    for arch in ("conv_model", "low_latency_conv"):
        bench_arch(arch, args.utts, args.steps, args.warmup, dev, board)
    bench_road(args.utts, args.steps, args.warmup, args.rounds, dev, board)
    return 0


if __name__ == "__main__":
    sys.exit(main())

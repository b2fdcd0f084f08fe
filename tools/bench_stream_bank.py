"""Many microphones per hop: the stream bank (edison_stream_bank_*, stream.StreamBank) beside the same number of independent
GeomStream objects pushed one after another -- the existing stream code is the yardstick, the bank is never its own baseline.

Device pushes of one frame at the shipped geometry and graph, output filter on, for every --mics count. Per count, in ONE process:
both legs are fed the same samples first and their outputs compared (exact), then warmed up, then timed in regions of many hops that
alternate bank, streams, bank, streams ... (--repeats regions each). A region's time is a host clock around its pushes and the
device synchronise that ends it, so it holds the enqueue cost as well as the kernels: what a caller waits for. Reported: the median
over regions of the time per hop of ALL microphones, its minimum and maximum, and streams / bank.

    python tools/bench_stream_bank.py [--mics 1,16,256,2048] [--repeats 7] [--region-ms 250] [--out FILE.json]

One JSON line per count; --out also writes them as a list.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mics", default="1,16,256,2048")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--region-ms", type=float, default=250.0, help="hops per region are chosen so that a region lasts about this long")
    ap.add_argument("--max-hops", type=int, default=5000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from edison_amd.context import Context
    from edison_amd.stream import GeomStream, StreamBank
    from geom_sweep import geom, signals
    dev = torch.device("cuda", 0)
    c = Context(0)
    board = c.device_info()["name"]
    g = geom()
    hop, no = g.frame_step, c.net_info()["n_out"]
    c.use_torch_stream()
    rows = []
    for M in [int(v) for v in args.mics.split(",")]:
        # eight hops of samples, another stretch of the signal mix for every microphone
        tile = signals(16, g.n_samples, 1).ravel()
        starts = (np.arange(M) * 7919) % (tile.shape[0] - 8 * hop)
        x = np.stack([tile[s:s + 8 * hop] for s in starts])                                    # [M][8 * hop]
        X = [torch.from_numpy(np.ascontiguousarray(x[:, k * hop:(k + 1) * hop])).to(dev) for k in range(8)]
        out = lambda: dict(logits=torch.zeros((M, no), dtype=torch.int8, device=dev), softmax=torch.zeros((M, no), dtype=torch.int8, device=dev),
                           argmax=torch.zeros(M, dtype=torch.int32, device=dev))
        ob, os_ = out(), out()
        bank = StreamBank(c, g, M, chunk_frames=1, output_filter=True)
        streams = [GeomStream(c, g, chunk_frames=1, output_filter=True) for _ in range(M)]
        per_stream = [[dict(samples=X[k][m], logits=os_["logits"][m:m + 1], softmax=os_["softmax"][m:m + 1], argmax=os_["argmax"][m:m + 1])
                       for m in range(M)] for k in range(8)]

        def hop_bank(k):
            bank.push_t(X[k % 8], **ob)

        def hop_streams(k):
            for s, kw in zip(streams, per_stream[k % 8]):
                s.push_t(kw["samples"], logits=kw["logits"], softmax=kw["softmax"], argmax=kw["argmax"])

        def region(fn, hops):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for k in range(hops):
                fn(k)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) / hops

        # the same samples through both: the outputs must agree before a time means anything
        for k in range(12):
            hop_bank(k)
            hop_streams(k)
            torch.cuda.synchronize(dev)
            for key in ob:
                assert torch.equal(ob[key], os_[key]), (M, k, key)
        # warm-up, and from it the hops of a region
        hops = {}
        for name, fn in (("bank", hop_bank), ("streams", hop_streams)):
            t = region(fn, 20)
            hops[name] = int(min(args.max_hops, max(8, args.region_ms * 1e-3 / t)))
            region(fn, hops[name])
        t = dict(bank=[], streams=[])
        for _ in range(args.repeats):
            for name, fn in (("bank", hop_bank), ("streams", hop_streams)):
                t[name].append(region(fn, hops[name]))
        us = lambda v: round(float(v) * 1e6, 2)
        row = dict(board=board, geometry="shipped", chunk=1, filter=1, n_mics=M, repeats=args.repeats, hops_per_region=hops,
                   bank_us_per_hop=us(np.median(t["bank"])), bank_min_us=us(min(t["bank"])), bank_max_us=us(max(t["bank"])),
                   streams_us_per_hop=us(np.median(t["streams"])), streams_min_us=us(min(t["streams"])), streams_max_us=us(max(t["streams"])),
                   streams_over_bank=round(float(np.median(t["streams"]) / np.median(t["bank"])), 2),
                   launches_per_hop=dict(bank=3, streams=3 * M))
        print(json.dumps(row), flush=True)
        rows.append(row)
        bank.close()
        for s in streams:
            s.close()
    c.use_own_stream()
    c.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

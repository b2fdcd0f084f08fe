"""What a mask costs: the stream bank's push without a mask beside the same push with an all-present mask and with a half-absent mask
(edison_bank_push_present_n_dev, StreamBank.push_t(present=)) -- the mask-less push is the yardstick.

Device pushes of one frame at the shipped geometry and graph, output filter on, for every --mics count. Per count, in ONE process and
on ONE bank: a second bank first shows that an all-present mask puts out what no mask puts out (exact); then the three cases are warmed
up and timed in regions of many hops that alternate none, all present, half absent, none ... (--repeats regions each). A region's time is
a host clock around its pushes and the device synchronise that ends it, so it holds the enqueue cost as well as the kernels. Reported:
the median over regions of the time per hop of ALL microphones, its minimum and maximum, and each masked case over the mask-less one.

By construction a push with a mask launches one kernel more than one without, whatever n_mics: MFCC, network, filter without; MFCC,
network, hold, masked filter with (launches_per_push). --count-run pushes a fixed number of each case and nothing else, for a kernel
trace to count them.

    python tools/bench_bank_present.py [--mics 256] [--repeats 7] [--region-ms 250] [--out FILE.json]
    python tools/bench_bank_present.py --count-run [--mics 1,256]

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

CASES = ("none", "all_present", "half_absent")
COUNT_RUN = dict(none=5, all_present=7, half_absent=11)     # pushes of --count-run: three different numbers, to tell the cases apart
LAUNCHES = dict(none=3, all_present=4, half_absent=4)       # kernels per push of one frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mics", default="256")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--region-ms", type=float, default=250.0, help="hops per region are chosen so that a region lasts about this long")
    ap.add_argument("--max-hops", type=int, default=5000)
    ap.add_argument("--count-run", action="store_true", help="a fixed number of pushes per case and no timing: for a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from edison_amd.context import Context
    from edison_amd.stream import StreamBank
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
        ob = out()
        half = np.ones(M, np.uint8)
        half[::2] = 0                                                                          # one microphone: absent
        masks = dict(none=None, all_present=torch.ones(M, dtype=torch.uint8, device=dev), half_absent=torch.from_numpy(half).to(dev))
        bank = StreamBank(c, g, M, chunk_frames=1, output_filter=True)
        hop_fn = {name: (lambda k, p=masks[name]: bank.push_t(X[k % 8], present=p, **ob)) for name in CASES}

        if args.count_run:
            for name in CASES:
                for k in range(COUNT_RUN[name]):
                    hop_fn[name](k)
            torch.cuda.synchronize(dev)
            row = dict(n_mics=M, pushes=COUNT_RUN, launches_per_push=LAUNCHES, kernels=sum(COUNT_RUN[n] * LAUNCHES[n] for n in CASES),
                       hold_kernels=COUNT_RUN["all_present"] + COUNT_RUN["half_absent"])
            print(json.dumps(row), flush=True)
            rows.append(row)
            bank.close()
            continue

        def region(fn, hops):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for k in range(hops):
                fn(k)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) / hops

        # an all-present mask puts out what no mask puts out: a second bank, the same samples
        other, oo = StreamBank(c, g, M, chunk_frames=1, output_filter=True), out()
        for k in range(12):
            hop_fn["all_present"](k)
            other.push_t(X[k % 8], **oo)
            torch.cuda.synchronize(dev)
            for key in ob:
                assert torch.equal(ob[key], oo[key]), (M, k, key)
        other.close()
        # warm-up, and from it the hops of a region
        hops = {}
        for name in CASES:
            t = region(hop_fn[name], 20)
            hops[name] = int(min(args.max_hops, max(8, args.region_ms * 1e-3 / t)))
            region(hop_fn[name], hops[name])
        t = {name: [] for name in CASES}
        for _ in range(args.repeats):
            for name in CASES:
                t[name].append(region(hop_fn[name], hops[name]))
        us = lambda v: round(float(v) * 1e6, 2)
        row = dict(board=board, geometry="shipped", chunk=1, filter=1, n_mics=M, repeats=args.repeats, hops_per_region=hops)
        for name in CASES:
            row.update({name + "_us_per_hop": us(np.median(t[name])), name + "_min_us": us(min(t[name])), name + "_max_us": us(max(t[name]))})
        row.update(all_present_over_none=round(float(np.median(t["all_present"]) / np.median(t["none"])), 3),
                   half_absent_over_none=round(float(np.median(t["half_absent"]) / np.median(t["none"])), 3), launches_per_push=LAUNCHES)
        assert all(LAUNCHES[name] == LAUNCHES["none"] + 1 for name in CASES[1:])
        print(json.dumps(row), flush=True)
        rows.append(row)
        bank.close()
    c.use_own_stream()
    c.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

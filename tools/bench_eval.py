#!/usr/bin/env python
"""Report-only: what scoring a batch of network outputs costs on the device against the path it replaces. Prints ONE JSON line and
gates nothing.

    python tools/bench_eval.py [--n 262144] [--classes 10] [--iters 200] [--warmup 20]

At n x classes int8 softmax rows resident on the device (bench.py's batch, the shipped graph's width), in one process, alternating:

  eval_add_us    one edison_eval_add_i8_dev: `iters` adds enqueued back to back between two device events, total / iters
  host_count_us  the path it replaces: the device-to-host copy of the softmax (into pinned memory, synchronised) and the numpy count --
                 first-maximum argmax and np.add.at into the matrix (no top-k, no rank: the numpy side does less)
  d2h_us         the copy alone

The counters of the timed adds are compared with the numpy count of the same rows times the number of adds made.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from edison_amd.context import Context

    ctx = Context(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    logits = rng.normal(0, 2, (a.n, a.classes))
    p = np.exp(logits - logits.max(axis=1, keepdims=True))
    soft = np.clip(np.rint(127 * p / p.sum(axis=1, keepdims=True)), -128, 127).astype(np.int8)      # rows shaped like an int8 softmax
    labels = rng.integers(0, a.classes, a.n).astype(np.int32)
    d_soft, d_lab = torch.from_numpy(soft).to(dev), torch.from_numpy(labels).to(dev)
    pinned = torch.empty((a.n, a.classes), dtype=torch.int8).pin_memory()
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.use_torch_stream(stream)
    ev = ctx.evaluator(rule="nnom", n_classes=a.classes, top_k=2)

    def host_count():
        pinned.copy_(d_soft, non_blocking=True)
        stream.synchronize()
        t_copy = time.perf_counter()
        out = pinned.numpy()
        m = np.zeros((a.classes, a.classes), np.uint64)
        np.add.at(m, (labels, out.argmax(axis=1)), 1)
        return m, t_copy

    adds = 0
    for _ in range(a.warmup):
        ev.add_t(d_soft, d_lab)
        adds += 1
    want, _ = host_count()
    stream.synchronize()
    add_us, host_us, d2h_us = [], [], []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.iters):
            ev.add_t(d_soft, d_lab)
        e1.record(stream)
        e1.synchronize()
        adds += a.iters
        add_us.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        for _ in range(3):
            t0 = time.perf_counter()
            _, t_copy = host_count()
            t1 = time.perf_counter()
            host_us.append((t1 - t0) * 1e6)
            d2h_us.append((t_copy - t0) * 1e6)
    got = ev.result()
    ok = bool(np.array_equal(got.confusion, want * np.uint64(adds)) and got.count == adds * a.n)
    info = ctx.device_info()
    ev.close()
    ctx.use_own_stream()
    print(json.dumps(dict(tool="bench_eval", device=info["name"], n=a.n, classes=a.classes, iters=a.iters, rounds=a.rounds,
                          eval_add_us=round(float(np.median(add_us)), 2), eval_add_us_min=round(min(add_us), 2), eval_add_us_max=round(max(add_us), 2),
                          host_count_us=round(float(np.median(host_us)), 1), host_count_us_min=round(min(host_us), 1),
                          d2h_us=round(float(np.median(d2h_us)), 1), counts_match=ok)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Kernel timing of the 9-layer DS-CNN fixture graph (tests/golden/alt_models/dscnn_kws.h) on the GPU box: the fused kernel
(edison_net_batch_dev: DW_Conv2D / AvgPool on the VALU between the matrix-core layers, one launch) against the
layer-by-layer kernel (edison_net_layers_dev, which also writes every layer's output), interleaved in one process.
usage: bench_dscnn.py [--n 262144] [--rounds 7] [--reps 5]
Device events around `reps` back-to-back launches; the two routes alternate round by round, so that clock and thermal drift
hit both alike; the median round and the min..max spread of each route are printed, and one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("EDISON_NET_SPECIALIZE", "0")
import torch  # noqa: E402
from edison_amd.context import Context, _t_ptr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--header", default=os.path.join(ROOT, "tests", "golden", "alt_models", "dscnn_kws.h"))
ap.add_argument("--n", type=int, default=262144)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = Context(0, model_path=None)
ctx.load_weights_h(a.header)
st = torch.cuda.Stream()
torch.cuda.set_stream(st)
ctx.use_torch_stream(st)
info = ctx.net_info()
assert info["accelerated"] == 2, "the graph has no plan for the fused kernel"
n_in = info["in_h"] * info["in_w"] * info["in_c"]
x = torch.randint(-128, 128, (a.n, n_in), dtype=torch.int8, device=dev)
logits = torch.empty((a.n, info["n_out"]), dtype=torch.int8, device=dev)
am = torch.empty((a.n,), dtype=torch.int32, device=dev)
acts = torch.empty((a.n, info["acts_bytes"]), dtype=torch.int8, device=dev)
L = ctx._L
routes = {
    "fused": lambda: ctx._check(L.edison_net_batch_dev(ctx._h, _t_ptr(x), a.n, _t_ptr(logits), None, _t_ptr(am))),
    "layer_by_layer": lambda: ctx._check(L.edison_net_layers_dev(ctx._h, _t_ptr(x), a.n, _t_ptr(acts))),
}


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps


for fn in routes.values():      # warm-up: code objects, clocks
    for _ in range(3):
        fn()
torch.cuda.synchronize()
ms = {k: [] for k in routes}
for _ in range(a.rounds):
    for k, fn in routes.items():
        ms[k].append(once(fn))
# the layer-by-layer route's logits layer equals the fused kernel's logits
off = info["layers"][-2 if info["has_softmax"] else -1]["acts_offset"]
same = bool(torch.equal(acts[:, off:off + info["n_out"]], logits))
out = {"graph": os.path.basename(a.header), "n": a.n, "bit_identical": same}
for k, v in ms.items():
    med = statistics.median(v)
    out[k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "minputs_per_s": round(a.n / med / 1e3, 2)}
    print("%-16s median %.3f ms (min %.3f, max %.3f) / %d inputs = %.2f M inputs/s" % (k, med, min(v), max(v), a.n, a.n / med / 1e3))
out["fused_speedup"] = round(out["layer_by_layer"]["ms_median"] / out["fused"]["ms_median"], 3)
print(json.dumps(out))
ctx.close()

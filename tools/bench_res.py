#!/usr/bin/env python3
"""Kernel timing of the residual fixture graph (tests/golden/alt_models/res_kws.h) on the GPU box, in the style of bench_dscnn.py:
the fused kernel (edison_net_batch_dev: held skip tensors, Add on the VALU between the matrix-core layers, one launch) against the
layer-by-layer kernel (edison_net_layers_dev, which also writes every layer's output), and beside them the structurally nearest
sequential graph, dscnn_kws.h, on the fused kernel -- the figure to compare between two commits: its plan does not depend on
anything the branching graphs added. All three interleaved in one process.
usage: bench_res.py [--n 65536] [--rounds 7] [--reps 5]
Device events around `reps` back-to-back launches; the routes alternate round by round, so that clock and thermal drift hit all
alike; the median round and the min..max spread of each are printed, and one JSON line with inferences per second."""
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
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

dev = torch.device("cuda", 0)
st = torch.cuda.Stream()
torch.cuda.set_stream(st)
models = os.path.join(ROOT, "tests", "golden", "alt_models")
routes, keep, lds = {}, [], {}
for name in ("res_kws", "dscnn_kws"):
    ctx = Context(0, model_path=None)
    ctx.load_weights_h(os.path.join(models, name + ".h"))
    ctx.use_torch_stream(st)
    info = ctx.net_info()
    assert info["accelerated"] == 2, "%s has no plan for the fused kernel" % name
    n_in = info["in_h"] * info["in_w"] * info["in_c"]
    x = torch.randint(-128, 128, (a.n, n_in), dtype=torch.int8, device=dev)
    logits = torch.empty((a.n, info["n_out"]), dtype=torch.int8, device=dev)
    am = torch.empty((a.n,), dtype=torch.int32, device=dev)
    keep.append((ctx, x, logits, am))
    routes[name + "_fused"] = (lambda c=ctx, x=x, lg=logits, am=am: c._check(c._L.edison_net_batch_dev(c._h, _t_ptr(x), a.n, _t_ptr(lg), None, _t_ptr(am))))
    if name == "res_kws":
        acts = torch.empty((a.n, info["acts_bytes"]), dtype=torch.int8, device=dev)
        routes["res_kws_layer_by_layer"] = (lambda c=ctx, x=x, t=acts: c._check(c._L.edison_net_layers_dev(c._h, _t_ptr(x), a.n, _t_ptr(t))))
        res_info, res_logits = info, logits


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
off = res_info["layers"][-2]["acts_offset"]     # the Dense layer in front of the Softmax: the logits
out = {"n": a.n, "bit_identical": bool(torch.equal(acts[:, off:off + res_info["n_out"]], res_logits))}
for k, v in ms.items():
    med = statistics.median(v)
    out[k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "inferences_per_s": round(a.n / med * 1e3)}
    print("%-24s median %.3f ms (min %.3f, max %.3f) / %d inputs = %.2f M inferences/s" % (k, med, min(v), max(v), a.n, a.n / med / 1e3))
print(json.dumps(out))
for c, *_ in keep:
    c.close()

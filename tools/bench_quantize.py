"""Cost and effect of quantising the reference's float32 network (tests/golden/cube_kws.ednf) to an int8 NNoM graph (DESIGN.md section
18). Measured, not gated:

  calibration  edison_fcal_add_dev against edison_fnet_batch_dev on the same --utts inputs (default 262 144), in one process,
               alternating the two --rounds times; the median of each and their ratio. The calibrator does the float network's MFMA
               work plus an LDS atomic per output and writes no logits.
  int8_net     edison_net_batch_dev on the quantised graph against edison_fnet_batch_dev on the float network, same inputs, alternating
  agreement    how often the int8 graph's argmax equals the float network's on 4096 seeded inputs (scaled and perturbed copies of the
               five fixture rows) plus the fixture rows: for the graph calibrated on those inputs and for the one calibrated on the
               five fixture rows alone, with method max_min and with saturate 0.001

    python tools/bench_quantize.py [--utts 262144] [--steps 20] [--warmup 2] [--rounds 5]

One JSON line per figure, all from one process.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the general int8 kernel, not a kernel compiled for each of the four graphs loaded here
os.environ.setdefault("EDISON_NET_SPECIALIZE", "0")
sys.path.insert(0, ROOT)


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


def alternate(a, b, rounds, steps, warmup):
    ta, tb = [], []
    for r in range(rounds):
        ta.append(timed(a, steps, warmup if r == 0 else 1))
        tb.append(timed(b, steps, warmup if r == 0 else 1))
    return ta, tb


def seeded_inputs(rows, n, seed=18):
    rng = np.random.default_rng(seed)
    x = [rows[i % len(rows)] * rng.uniform(0.25, 2.0) + rng.normal(0, 8.0, rows.shape[1]) for i in range(n)]
    return np.concatenate([np.array(x), rows]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    from edison_amd import cube_import, quantize as qz
    from edison_amd.context import Context
    dev = torch.device("cuda", 0)
    fixture = os.path.join(ROOT, "tests", "golden", "cube_kws.ednf")
    golden = np.load(os.path.join(ROOT, "tests", "golden", "cube_golden.npz"))
    rows = np.stack([golden["net_in_" + str(s)] for s in golden["names"]])
    with open(fixture, "rb") as f:
        model = cube_import.read_blob(f.read())
    c = Context(0, model_path=None)
    c.fnet_load(fixture)
    board = c.device_info()["name"]

    # agreement
    x = seeded_inputs(rows, 4096)
    want = c.fnet(x)["argmax"]
    cal = c.calibrator()
    blobs = {}
    for name, data in (("seeded", x), ("fixture_rows", rows)):
        cal.reset()
        cal.add(data)
        stats = cal.result()
        for method, kw in (("max_min", {}), ("saturate_0.001", dict(method="saturate", saturate=0.001))):
            try:
                blob, rep = qz.quantize(model, stats, **kw)
            except qz.QuantizeError as e:
                print(json.dumps(dict(board=board, what="agreement", calibrated_on=name, method=method, refused=str(e))), flush=True)
                continue
            blobs[(name, method)] = (blob, rep)
            c.load_model_bytes(blob)
            got = c.net(qz.quantize_input(x, rep["input"]["dec"]))["argmax"]
            print(json.dumps(dict(board=board, what="agreement", calibrated_on=name, method=method, inputs=len(x), in_dec=rep["input"]["dec"],
                                  out_dec=[L["out_dec"] for L in rep["layers"]], same_argmax=int((got == want).sum()),
                                  share=round(float((got == want).mean()), 4))), flush=True)

    # timing, on copies of the seeded inputs
    n = args.utts
    xt = torch.from_numpy(x).to(dev).repeat((n + len(x) - 1) // len(x), 1)[:n].contiguous()
    blob, rep = blobs[("seeded", "max_min")]
    c.load_model_bytes(blob)
    xi = torch.from_numpy(qz.quantize_input(x, rep["input"]["dec"])).to(dev).repeat((n + len(x) - 1) // len(x), 1)[:n].contiguous()
    lg = torch.empty((n, 10), dtype=torch.float32, device=dev)
    pr = torch.empty((n, 10), dtype=torch.float32, device=dev)
    am = torch.empty(n, dtype=torch.int32, device=dev)
    lg8 = torch.empty((n, 10), dtype=torch.int8, device=dev)
    sm8 = torch.empty((n, 10), dtype=torch.int8, device=dev)
    am8 = torch.empty(n, dtype=torch.int32, device=dev)
    c.use_torch_stream()
    run_f = lambda: c.fnet_t(xt, n, lg, pr, am)
    tf, tc = alternate(run_f, lambda: cal.add_t(xt, n), args.rounds, args.steps, args.warmup)
    tf2, t8 = alternate(run_f, lambda: c.net_t(xi, n, lg8, sm8, am8), args.rounds, args.steps, args.warmup)
    c.use_own_stream()
    med = statistics.median
    print(json.dumps(dict(board=board, what="calibration", utts=n, fnet_batch=c.fnet_info()["batch"], fcal_batch=cal.batch, fnet_s=[round(t, 6) for t in tf],
                          fcal_s=[round(t, 6) for t in tc], fnet_utts_per_s=round(n / med(tf), 1), fcal_utts_per_s=round(n / med(tc), 1),
                          fcal_over_fnet=round(med(tc) / med(tf), 3))), flush=True)
    print(json.dumps(dict(board=board, what="int8_net", utts=n, fnet_s=[round(t, 6) for t in tf2], int8_s=[round(t, 6) for t in t8],
                          fnet_utts_per_s=round(n / med(tf2), 1), int8_utts_per_s=round(n / med(t8), 1), speedup=round(med(tf2) / med(t8), 2),
                          int8_argmax_equals_float=round(float((am8.cpu().numpy() == am.cpu().numpy()).mean()), 4))), flush=True)
    cal.close()
    c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Many microphones per hop on the float32 X-CUBE-AI network: the float bank (edison_float_bank_*, stream.FloatBank) beside the same
number of independent FloatStream objects pushed one after another -- the existing stream code is the yardstick, the bank is never its
own baseline -- and, for pushes of several frames, the bank's one network launch beside the same bank forced to one launch per frame.

Device pushes at the shipped geometry and network (tests/golden/cube_kws.ednf), output filter on. One process per run (a run = one
line of the table): both legs are fed the same samples first and their outputs compared (equal, bit for bit), then warmed up, then timed
in regions of many pushes that alternate leg A, leg B, leg A ... (--repeats regions each). A region's time is a host clock around its
pushes and the device synchronise that ends it, so it holds the enqueue cost as well as the kernels: what a caller waits for. Reported:
the median over regions of the time per hop (a push of `chunk` frames counts as `chunk` hops) of ALL microphones, its minimum and maximum.

    python tools/bench_float_bank.py                       every run of DESIGN.md section 15a, each in a child process of its own
    python tools/bench_float_bank.py --run streams --mics 256 [--q15]     chunk 1: the bank against n_mics FloatStreams
    python tools/bench_float_bank.py --run per-frame --mics 256 --chunk 8 [--q15]   one network launch against one per frame
    [--repeats 7] [--region-ms 250] [--out FILE.json]

One JSON line per run; --out also writes them as a list.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RUNS = [("streams", m, 1, q) for q in (0, 1) for m in (1, 16, 256, 2048)] + [("per-frame", 256, 8, q) for q in (0, 1)]


def one_run(args):
    import torch
    from edison_amd import _lib
    from edison_amd import config as cfg
    from edison_amd.context import Context
    from edison_amd.kws.geometry import KwsGeometry
    from edison_amd.stream import FloatBank, FloatStream
    from geom_sweep import signals
    dev = torch.device("cuda", 0)
    c = Context(0, model_path=None)
    c.fnet_load(os.path.join(ROOT, "tests", "golden", "cube_kws.ednf"))
    board = c.device_info()["name"]
    g = KwsGeometry.from_config(net_input_scale=cfg.net_input_scale)
    hop, no = g.frame_step, c.fnet_info()["n_out"]
    M, n, q15 = args.mics, args.chunk, bool(args.q15)
    c.use_torch_stream()
    # eight pushes of samples, another stretch of the signal mix for every microphone
    tile = signals(16 + n, g.n_samples, 1).ravel()
    starts = (np.arange(M) * 7919) % (tile.shape[0] - 8 * n * hop)
    x = np.stack([tile[s:s + 8 * n * hop] for s in starts])                                    # [M][8 * n * hop]
    X = [torch.from_numpy(np.ascontiguousarray(x[:, k * n * hop:(k + 1) * n * hop])).to(dev) for k in range(8)]
    out = lambda: dict(logits=torch.zeros((n, M, no), dtype=torch.float32, device=dev), probs=torch.zeros((n, M, no), dtype=torch.float32, device=dev),
                       argmax=torch.zeros((n, M), dtype=torch.int32, device=dev), filtered=torch.zeros((n, M, no), dtype=torch.float32, device=dev))
    oa, ob = out(), out()
    bank = FloatBank(c, M, g, q15=q15, chunk_frames=n, output_filter=True)

    def hop_bank(k):
        bank.push_t(X[k % 8], **oa)

    if args.run == "streams":
        assert n == 1
        streams = [FloatStream(c, g, q15=q15, chunk_frames=1, output_filter=True) for _ in range(M)]
        per_stream = [[dict(samples=X[k][m], logits=ob["logits"][0, m:m + 1], probs=ob["probs"][0, m:m + 1], argmax=ob["argmax"][0, m:m + 1],
                            filtered=ob["filtered"][0, m:m + 1]) for m in range(M)] for k in range(8)]

        def hop_other(k):
            for s, kw in zip(streams, per_stream[k % 8]):
                s.push_t(kw["samples"], logits=kw["logits"], probs=kw["probs"], argmax=kw["argmax"], filtered=kw["filtered"])
        other = "streams"
    else:
        # the same bank object class, its network stage forced to one ed_launch_fnet per frame of the push
        forced = FloatBank(c, M, g, q15=q15, chunk_frames=n, output_filter=True)
        tool = _lib.lib().ed_float_bank_tool_per_frame
        tool.restype, tool.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]
        assert tool(forced._h, 1) == 0
        streams = [forced]

        def hop_other(k):
            forced.push_t(X[k % 8], **ob)
        other = "per_frame"

    def region(fn, pushes):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for k in range(pushes):
            fn(k)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / (pushes * n)

    # the same samples through both: the outputs must agree before a time means anything
    for k in range(12):
        hop_bank(k)
        hop_other(k)
        torch.cuda.synchronize(dev)
        for key in oa:
            assert torch.equal(oa[key].view(torch.int32), ob[key].view(torch.int32)), (M, k, key)
    # warm-up, and from it the pushes of a region
    legs = (("bank", hop_bank), (other, hop_other))
    pushes = {}
    for name, fn in legs:
        t = region(fn, 20)
        pushes[name] = int(min(args.max_pushes, max(8, args.region_ms * 1e-3 / (t * n))))
        region(fn, pushes[name])
    t = {name: [] for name, _ in legs}
    for _ in range(args.repeats):
        for name, fn in legs:
            t[name].append(region(fn, pushes[name]))
    us = lambda v: round(float(v) * 1e6, 2)
    row = dict(board=board, run=args.run, network="cube_kws.ednf", geometry="shipped", q15=int(q15), chunk=n, filter=1, n_mics=M, repeats=args.repeats,
               pushes_per_region=pushes)
    for name, _ in legs:
        row.update({name + "_us_per_hop": us(np.median(t[name])), name + "_min_us": us(min(t[name])), name + "_max_us": us(max(t[name]))})
    row[other + "_over_bank"] = round(float(np.median(t[other]) / np.median(t["bank"])), 2)
    print(json.dumps(row), flush=True)
    bank.close()
    for s in streams:
        s.close()
    c.use_own_stream()
    c.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=("streams", "per-frame"), default=None, help="one run in this process; without it every run, a child process each")
    ap.add_argument("--mics", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=1)
    ap.add_argument("--q15", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--region-ms", type=float, default=250.0, help="pushes per region are chosen so that a region lasts about this long")
    ap.add_argument("--max-pushes", type=int, default=5000)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds a child run may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        rows = [one_run(args)]
    else:
        rows = []
        for run, mics, chunk, q15 in RUNS:
            cmd = [sys.executable, os.path.abspath(__file__), "--run", run, "--mics", str(mics), "--chunk", str(chunk), "--repeats", str(args.repeats),
                   "--region-ms", str(args.region_ms), "--max-pushes", str(args.max_pushes)] + (["--q15"] if q15 else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if r.returncode != 0:   # a run that failed ends the series: nothing more is started on the device
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                return 1
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

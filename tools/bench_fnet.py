"""Throughput and accuracy of the float32 X-CUBE-AI network path on the reference's own network
(tests/golden/cube_kws.ednf):

  fnet       the network alone, edison_fnet_batch_dev on device tensors
  kws_float  audio -> class, edison_kws_float_batch_dev, host flow (float64 MFCC -> float32 -> scale -> clip -> network)
  kws_q15    audio -> class, firmware flow (variant C -> (float) -> network)

timed with device events at --utts utterances (default 262 144; the audio is one long seeded recording read as 2 s windows one
frame apart), plus the numbers the GPU tests' bounds rest on: the largest per-layer
error over 1e-7 S (tests/test_gpu_fnet.py), the largest end-to-end logit and probability differences to the float64 restatement, and
the host-flow features that differ from the reference's float32 net input.

    python tools/bench_fnet.py [--utts 262144] [--steps 10] [--warmup 3]

One JSON line per figure. Every figure is a single run of one process.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MAC_PER_UTT = 798438          # kws.c ai_kws_get_info: n_macc
PEAK_F32 = 157.3e12           # MI355X f32-input MFMA peak (FLOP/s)


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


def accuracy(c, model, golden):
    import fnet_host
    from test_gpu_fnet import SOURCES, _audio, _inputs
    x = _inputs(golden)
    acts = c.fnet_layers(x).astype(np.float64)
    prev, off, worst = np.asarray(x, np.float64), 0, []
    for i, L in enumerate(fnet_host.conv_records(model)):
        n = int(np.prod(L["out"]))
        want, S = fnet_host.layer_from(model, i, prev)
        got = acts[:, off:off + n]
        worst.append(round(float((np.abs(got - want) / (1e-7 * S + 1e-300)).max()), 3))
        prev, off = got, off + n
    r = c.fnet(x)
    ref = fnet_host.run64(model, x)
    a = _audio(golden)
    h = c.kws_float(a)
    flips = [int((h["feat"][j] != golden["net_in_" + s]).sum()) for j, s in enumerate(SOURCES)]
    top = np.sort(ref["logits"], axis=1)
    return dict(layer_err_over_1e7S=worst, logits_vs_f64_chain=float(np.abs(r["logits"] - ref["logits"]).max()),
                probs_vs_f64_chain=float(np.abs(r["probs"] - ref["probs"]).max()),
                probs_vs_f64_softmax_of_logits=float(np.abs(r["probs"] - fnet_host.softmax(r["logits"].astype(np.float64))).max()),
                argmax_diff=int((r["argmax"] != ref["argmax"]).sum()), min_top2_margin=float((top[:, -1] - top[:, -2]).min()),
                host_feature_flips=flips, edison_p=float(h["probs"][0, 0]), edison_p_fixture=float(golden["probs_edison"][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import fnet_host
    from edison_amd.context import Context
    from edison_amd.kws.geometry import KwsGeometry
    dev = torch.device("cuda", 0)
    fixture = os.path.join(ROOT, "tests", "golden", "cube_kws.ednf")
    golden = np.load(os.path.join(ROOT, "tests", "golden", "cube_golden.npz"))
    c = Context(0, model_path=None)
    c.fnet_load(fixture)
    board = c.device_info()["name"]
    info = c.fnet_info()
    print(json.dumps(dict(board=board, what="accuracy", **accuracy(c, fnet_host.load(fixture), golden))), flush=True)

    n = args.utts
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    x = torch.randn((n, 403), generator=gen, device=dev) * 200
    # a long recording read as overlapping 2 s utterances one frame apart (utt_stride 1024): n distinct windows in 0.5 GB
    stride = 1024
    audio = (torch.randn(((n - 1) * stride + 32000,), generator=gen, device=dev) * 3000).clamp(-32768, 32767).to(torch.int16)
    lg = torch.empty((n, 10), dtype=torch.float32, device=dev)
    pr = torch.empty((n, 10), dtype=torch.float32, device=dev)
    am = torch.empty(n, dtype=torch.int32, device=dev)
    feat = torch.empty((n, 403), dtype=torch.float32, device=dev)
    g = KwsGeometry.from_config()
    c.use_torch_stream()
    rows = [("fnet", timed(lambda: c.fnet_t(x, n, lg, pr, am), args.steps, args.warmup)),
            ("kws_float", timed(lambda: c.kws_float_t(audio, g, n, stride, feat, lg, pr, am), args.steps, args.warmup)),
            ("kws_q15", timed(lambda: c.kws_float_t(audio, g, n, stride, feat, lg, pr, am, q15=True), args.steps, args.warmup))]
    c.use_own_stream()
    for route, sec in rows:
        flops = 2.0 * MAC_PER_UTT * n
        print(json.dumps(dict(board=board, what="throughput", route=route, utts=n, batch_per_workgroup=info["batch"], lds_bytes=info["lds_bytes"],
                              seconds=round(sec, 6), utts_per_s=round(n / sec, 1), net_tflops=round(flops / sec / 1e12, 2),
                              share_of_f32_peak=round(flops / sec / PEAK_F32, 4))), flush=True)
    c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

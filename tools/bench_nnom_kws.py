#!/usr/bin/env python3
"""Timing of the NNoM example's two GPU entry points against the routes that existed before them. One JSON line.

    python tools/bench_nnom_kws.py [--utt 65536] [--rounds 9] [--events 1,8,64]

Pair 1, audio to label for a batch: edison_kws_f32_batch_dev at --utt utterances laid hop x rows samples apart, against one flat
edison_mfcc_f32_batch_dev launch over the same frames followed by edison_net_batch_dev; and the feature launches of the two alone
(rows form against flat form: the same kernel, the same frames).
Pair 2, the continuous loop: edison_f32_stream_predict_dev at 1, 8 and 64 events per push (the graph reads its windows in place),
against edison_f32_stream_push_dev (which copies the windows out) followed by edison_net_batch_dev on the copies.

Device events around the timed calls on one HIP stream; the routes of a pair alternate round by round, the order swapping every round;
reported per route: the median over the rounds and the spread (minimum and maximum), in microseconds per call. Both routes' labels are
compared before anything is timed. The graph is tests/golden/alt_models/dscnn_kws.h (12 x 10 x 1), the extractor
mfcc_create(11, 1, 512, 8, 0.97); the audio is seeded noise made on the device.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utt", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--events", default="1,8,64")
    args = ap.parse_args()
    import numpy as np
    import torch
    from edison_amd.context import Context
    from edison_amd.mfcc.mfcc_f32 import MfccF32, NnomKwsFrontEnd

    c = Context(0, model_path=None)
    c.load_weights_h(os.path.join(ROOT, "tests", "golden", "alt_models", "dscnn_kws.h"))
    m = MfccF32(ctx=c, num_mfcc_features=11, feature_offset=1)
    info = c.net_info()
    rows, n_out, n_cls, hop = info["in_h"], info["in_w"], info["n_out"], 256
    dev = torch.device("cuda", c.device)
    c.use_torch_stream()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)

    def noise(n):
        return torch.randint(-3000, 3000, (n,), dtype=torch.int16, device=dev, generator=gen)

    def timed(fn, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / reps

    def pair(routes, reps):
        """routes: {name: fn}; alternate, swapping the order every round -> {name: dict(median_us, min_us, max_us)}"""
        names = list(routes)
        for k in names:                                                    # warm up every shape the timed window uses
            timed(routes[k], 2)
        got = {k: [] for k in names}
        for r in range(args.rounds):
            for k in (names if r % 2 == 0 else names[::-1]):
                got[k].append(timed(routes[k], reps))
        return {k: dict(median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in got.items()}

    res = dict(graph="dscnn_kws 12x10x1", extractor="mfcc_create(11,1,512,8,0.97)", rounds=args.rounds)

    # ---- pair 1
    n, stride = args.utt, rows * hop
    audio = noise((n - 1) * stride + (rows - 1) * hop + 512)
    feat_a, feat_b = (torch.empty((n, rows * n_out), dtype=torch.int8, device=dev) for _ in range(2))
    lg, sm = (torch.empty((n, n_cls), dtype=torch.int8, device=dev) for _ in range(2))
    label, am = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    prob = torch.empty(n, dtype=torch.float32, device=dev)

    def one_call():
        c.kws_f32_t(m, audio, n, stride, label, hop=hop, feat=feat_a, logits=lg, softmax=sm, prob=prob)

    def flat_then_net():
        m.compute_t(audio, n * rows, hop, feat_b)
        c.net_t(feat_b, n, lg, sm, am)

    one_call(); flat_then_net(); torch.cuda.synchronize()
    assert torch.equal(feat_a, feat_b) and torch.equal(label, am), "the two routes disagree"
    res["batch"] = dict(n_utt=n, frames=n * rows, **pair({"kws_f32_batch_dev": one_call, "flat_mfcc_then_net_batch_dev": flat_then_net}, 10))
    res["batch_features_only"] = pair({"rows_form": lambda: m.rows_t(audio, n, stride, rows, hop, feat_a),
                                       "flat_form": lambda: m.compute_t(audio, n * rows, hop, feat_b)}, 20)

    # ---- pair 2
    res["stream"] = {}
    for k in [int(v) for v in args.events.split(",")]:
        fe_a, fe_b = (NnomKwsFrontEnd(ctx=c, window_rows=rows, max_events=k, num_mfcc_features=11, feature_offset=1) for _ in range(2))
        x = noise(k * 512)
        win = torch.empty((k, rows * n_out), dtype=torch.int8, device=dev)
        la, lb = torch.empty(k, dtype=torch.int32, device=dev), torch.empty(k, dtype=torch.int32, device=dev)

        def in_place():
            fe_a.predict_t(x, k, la, logits=lg, softmax=sm, prob=prob)

        def copy_then_net():
            fe_b.push_t(x, k, win)
            c.net_t(win, k, lg, sm, lb)

        for _ in range(rows):                                              # the same history in both streams before the comparison
            in_place(); copy_then_net()
        torch.cuda.synchronize()
        assert torch.equal(la, lb), "the two stream routes disagree"
        res["stream"]["%d_events" % k] = pair({"stream_predict_dev": in_place, "stream_push_dev_then_net_batch_dev": copy_then_net}, 500)
        fe_a.close(); fe_b.close()
    c.use_own_stream()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

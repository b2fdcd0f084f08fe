"""Throughput of float64 MFCC at any geometry for a whole data set: the one call (edison_mfcc_geom_batch_dev on device tensors, timed with
device events) against the route kws.features.dataset_features takes without a geometry -- at the five geometries of
tests/test_gpu_kws_geom.py one edison_mfcc_generic call per utterance (float64 direct DFT, host pointers, tables rebuilt and a
synchronisation every call), at the shipped geometry one fp32 edison_mfcc_rows call -- and dataset_features(x, geometry=) itself
(host arrays in and out, wall clock).

    python tools/bench_mfcc_geom.py [--utts 16384] [--per-utt-utts 256] [--steps 10] [--warmup 3]

One JSON line per (geometry, route): utterances/s and frames/s. Every figure is a single run of one process.
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


def wall(fn):
    fn()
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=16384)
    ap.add_argument("--per-utt-utts", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from edison_amd.context import Context
    from edison_amd.kws.features import dataset_features
    from geom_sweep import GEOMS, geom, signals
    dev = torch.device("cuda", 0)
    cases = [("shipped", {})] + [(n, GEOMS[n]) for n in sorted(GEOMS)]
    for name, kw in cases:
        c = Context(0, model_path=None)
        board = c.device_info()["name"]
        g = geom(**kw)
        F, nu = g.frame_count, args.utts
        audio_h = np.tile(signals(64, g.n_samples, 1), (nu // 64, 1))
        audio = torch.from_numpy(audio_h).to(dev)
        out = torch.empty((nu, F, g.num_mfcc), dtype=torch.float64, device=dev)
        c.use_torch_stream()
        rows = [("mfcc_geom_t", nu, timed(lambda: c.mfcc_geom_t(audio, g, nu, g.n_samples, out), args.steps, args.warmup))]
        c.use_own_stream()
        rows.append(("dataset_features_geometry", nu, wall(lambda: dataset_features(audio_h, geometry=g, ctx=c))))
        # dataset_features without a geometry: the same geometry through its keywords
        kws = dict(fs=int(g.sample_rate), nSamples=g.n_samples, frame_length=g.frame_len, frame_step=g.frame_step, num_mel_bins=g.mel_nbins,
                   lower_edge_hertz=g.lower_edge_hertz, upper_edge_hertz=g.upper_edge_hertz, mel_mtx_scale=g.mel_mtx_scale,
                   use_mfcc_log=g.use_log, first_mfcc=g.first_mfcc, num_mfcc=g.num_mfcc, net_input_scale=g.net_input_scale)
        if g.variant == 1:   # dataset_features' own route computes variant B only
            n_old = nu if name == "shipped" else args.per_utt_utts
            route = "dataset_features_rows_fp32" if name == "shipped" else "dataset_features_per_utt"
            rows.append((route, n_old, wall(lambda: dataset_features(audio_h[:n_old], ctx=c, **kws))))
        for route, n, sec in rows:
            print(json.dumps(dict(board=board, geometry=name, route=route, frame_len=g.frame_len, mel_nbins=g.mel_nbins, frames_per_utt=F, utts=n,
                                  seconds=round(sec, 6), utts_per_s=round(n / sec, 1), frames_per_s=round(n * F / sec, 1))), flush=True)
        c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

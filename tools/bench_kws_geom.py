"""Throughput of keyword spotting at other MFCC geometries: the one-call path (edison_kws_geom_batch_dev, float64 FFT MFCC + the graph)
against the route a user had before it -- per utterance edison_mfcc_generic (float64 direct DFT, host-pointer call), quantisation on
the host, then edison_net_batch -- at the shipped geometry and at the five geometries of tests/test_gpu_kws_geom.py, plus, at the shipped
geometry, the fixed-shape kws in its default (fp32) and exact modes.

    python tools/bench_kws_geom.py [--utts 32768] [--composed-utts 256] [--steps 10] [--warmup 3]

One JSON line per (geometry, route): utterances/s and frames/s. The one-call and fixed-shape rows time device-tensor calls on torch's
stream with device events; the composed row times the host loop (it synchronises per utterance by construction).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32768)
    ap.add_argument("--composed-utts", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from edison_amd import _lib
    from edison_amd.context import Context
    from geom_sweep import GEOMS, geom, header, signals
    dev = torch.device("cuda", 0)
    cases = [("shipped", None, {})] + [(n, header(n), GEOMS[n]) for n in sorted(GEOMS)]
    for name, header, kw in cases:
        c = Context(0, model_path=None) if header else Context(0)
        if header:
            c.load_weights_h(header)
        info = c.net_info()
        board = c.device_info()["name"]
        g = geom(**kw)
        F, nu = g.frame_count, args.utts
        audio_h = signals(64, g.n_samples, 1)
        audio = torch.from_numpy(np.tile(audio_h, (nu // 64, 1))).to(dev)
        feat = torch.empty((nu, g.n_features), dtype=torch.int8, device=dev)
        logits = torch.empty((nu, info["n_out"]), dtype=torch.int8, device=dev)
        soft = torch.empty_like(logits) if info["has_softmax"] else None
        am = torch.empty((nu,), dtype=torch.int32, device=dev)
        c.use_torch_stream()
        rows = []
        s = timed(lambda: c.kws_geom_t(audio, g, nu, g.n_samples, feat, logits, soft, am), args.steps, args.warmup)
        rows.append(("kws_geom", nu, s))
        if name == "shipped":
            for exact in (False, True):
                s = timed(lambda: c.kws_t(audio, nu, g.n_samples, feat=feat, logits=logits, softmax=soft, argmax=am, exact=exact), args.steps, args.warmup)
                rows.append(("kws_exact" if exact else "kws_default", nu, s))
        c.use_own_stream()
        # the composed route: edison_mfcc_generic per utterance, host quantisation, edison_net_batch
        L, gc = c._L, g.to_ctypes()
        m = np.zeros((F, g.mel_nbins))
        ncu = args.composed_utts

        def composed():
            fs = np.zeros((ncu, g.n_features), np.int8)
            for u in range(ncu):
                x = np.ascontiguousarray(audio_h[u % 64])
                r = L.edison_mfcc_generic(c._h, x.ctypes.data, F, g.frame_len, g.frame_step, gc.variant, g.mel_nbins, g.sample_rate, g.lower_edge_hertz,
                                          g.upper_edge_hertz, g.mel_mtx_scale, None, None, None, None, m.ctypes.data, 0, None, 1.0)
                assert r == 0, L.edison_last_error(c._h)
                v = m[:, g.first_mfcc:g.first_mfcc + g.num_mfcc].astype(np.float32) * np.float32(g.net_input_scale)
                fs[u] = np.rint(np.clip(v, -128, 127)).astype(np.int8).reshape(-1)
            return c.net(fs)
        composed()
        t0 = time.perf_counter()
        composed()
        rows.append(("composed", ncu, time.perf_counter() - t0))
        for route, n, sec in rows:
            print(json.dumps(dict(board=board, geometry=name, route=route, frame_len=g.frame_len, mel_nbins=g.mel_nbins, frames_per_utt=F, utts=n,
                                  seconds=round(sec, 6), utts_per_s=round(n / sec, 1), frames_per_s=round(n * F / sec, 1))), flush=True)
        c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

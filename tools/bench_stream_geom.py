"""Continuous keyword spotting at other MFCC geometries (edison_stream_geom_*, stream.GeomStream), per geometry of
tests/test_gpu_kws_geom.py and the shipped one:

  * device-push throughput: one hour of audio pushed in --chunk-frame device pushes on torch's stream, in inferences/s, beside the
    kws_geom batch call over the same windows (utt_stride = frame_step) -- the same inferences in one call;
  * host-push latency at chunk 1: p50 / p99 over --pushes pushes after --warmup, for the shipped geometry and kws_small's (512-sample
    frames, 20 mel bins), beside the fixed stream's chunk-1 host push at the same hop on its default (mapped) route and, in a child
    process started with EDISON_STREAM_NO_MAPPED=1 (read once per process), on its staged route.

    python tools/bench_stream_geom.py [--hours 1] [--chunk 4096] [--pushes 2000] [--warmup 200]

One JSON line per (geometry, measurement). Every figure is one run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def latency(push, frames, args):
    for i in range(args.warmup):
        push(frames[i % len(frames)])
    t = np.zeros(args.pushes)
    for i in range(args.pushes):
        x = frames[i % len(frames)]
        t0 = time.perf_counter()
        push(x)
        t[i] = time.perf_counter() - t0
    return dict(pushes=args.pushes, p50_us=round(float(np.percentile(t, 50)) * 1e6, 1), p99_us=round(float(np.percentile(t, 99)) * 1e6, 1))


def fixed_latency(args, route):
    """the fixed stream's chunk-1 host push at hop 1024 (the hop of both latency geometries)"""
    from edison_amd.context import Context
    from edison_amd.stream import Stream
    c = Context(0)
    s = Stream(c, hop=1024, chunk_frames=1)
    rng = np.random.default_rng(1)
    frames = [np.clip(rng.normal(0, 2000, 1024), -32768, 32767).astype(np.int16) for _ in range(64)]
    emit(board=c.device_info()["name"], geometry="shipped", measure="fixed_stream_host_push", route=route, hop=1024, chunk=1, **latency(s.push, frames, args))
    s.close()
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--pushes", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--fixed-only", default=None, help=argparse.SUPPRESS)  # the child process: the fixed stream's host push only
    args = ap.parse_args()
    if args.fixed_only:
        fixed_latency(args, args.fixed_only)
        return 0
    import torch
    from edison_amd.context import Context
    from edison_amd.stream import GeomStream
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
        hop, F, ch = g.frame_step, g.frame_count, args.chunk
        K = int(args.hours * 3600 * g.sample_rate) // hop // ch * ch   # whole pushes of one hour
        tile = signals(16, g.n_samples, 1).ravel()
        x = torch.from_numpy(np.resize(tile, K * hop)).to(dev)
        lo = torch.empty((ch, info["n_out"]), dtype=torch.int8, device=dev)
        am = torch.empty(ch, dtype=torch.int32, device=dev)
        s = GeomStream(c, g, chunk_frames=ch)
        c.use_torch_stream()

        def stream_hour():
            for k0 in range(0, K, ch):
                s.push_t(x[k0 * hop:(k0 + ch) * hop], logits=lo, argmax=am)
        stream_hour()   # warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        stream_hour()
        e1.record()
        torch.cuda.synchronize()
        sec = e0.elapsed_time(e1) / 1e3
        emit(board=board, geometry=name, measure="device_push", frame_len=g.frame_len, hop=hop, mel_nbins=g.mel_nbins, window_rows=F, chunk=ch,
             inferences=K, seconds=round(sec, 6), inferences_per_s=round(K / sec, 1))
        # the batch call over the same windows: utterance u starts at u * hop, F frames each
        n_utt = (K * hop - g.frame_len) // hop + 1 - (F - 1)
        blo = torch.empty((n_utt, info["n_out"]), dtype=torch.int8, device=dev)
        bam = torch.empty(n_utt, dtype=torch.int32, device=dev)
        c.kws_geom_t(x, g, n_utt, hop, None, blo, None, bam)
        torch.cuda.synchronize()
        e0.record()
        c.kws_geom_t(x, g, n_utt, hop, None, blo, None, bam)
        e1.record()
        torch.cuda.synchronize()
        sec = e0.elapsed_time(e1) / 1e3
        emit(board=board, geometry=name, measure="kws_geom_batch", frame_len=g.frame_len, hop=hop, mel_nbins=g.mel_nbins, window_rows=F,
             inferences=n_utt, seconds=round(sec, 6), inferences_per_s=round(n_utt / sec, 1))
        c.use_own_stream()
        s.close()
        del x
        if name in ("shipped", "kws_small"):
            s1 = GeomStream(c, g, chunk_frames=1)
            frames = [tile[i * hop:(i + 1) * hop].copy() for i in range(64)]
            emit(board=board, geometry=name, measure="geom_stream_host_push", frame_len=g.frame_len, hop=hop, mel_nbins=g.mel_nbins, chunk=1,
                 **latency(s1.push, frames, args))
            s1.close()
        c.close()
    fixed_latency(args, "default (mapped)")
    env = dict(os.environ, EDISON_STREAM_NO_MAPPED="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--fixed-only", "staged", "--pushes", str(args.pushes), "--warmup", str(args.warmup)],
                       env=env, timeout=600)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())

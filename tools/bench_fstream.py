"""Continuous keyword spotting with the float32 X-CUBE-AI network (edison_stream_float_*, stream.FloatStream) on the reference's own
network (tests/golden/cube_kws.ednf), in the host flow (float64 MFCC -> float32 x scale -> clip) and in the firmware's flow (variant C):

  * device-push throughput: one hour of audio pushed in --chunk-frame device pushes on torch's stream (device events), in inferences/s,
    beside one kws_float batch call over the same windows (utt_stride = frame_step) -- the same inferences in one call;
  * host-push latency at chunk 1: p50 / p99 over --pushes pushes after --warmup.

    python tools/bench_fstream.py [--hours 1] [--chunk 4096] [--pushes 2000] [--warmup 200]
    python tools/bench_fstream.py --trace-pushes 64      # only a scripted sequence of device pushes (filter on), for a kernel trace

One JSON line per (flow, measurement). Every figure is one run.
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

FIXTURE = os.path.join(ROOT, "tests", "golden", "cube_kws.ednf")


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


def audio(n):
    from geom_sweep import signals
    return np.resize(signals(16, 32000, 1).ravel(), n)


def trace(c, g, args):
    """args.trace_pushes device pushes of 512 frames per flow, filter on: the sequence a kernel trace counts dispatches of."""
    import torch
    from edison_amd.stream import FloatStream
    dev = torch.device("cuda", 0)
    ch, hop = 512, g.frame_step
    x = torch.from_numpy(audio(args.trace_pushes * ch * hop)).to(dev)
    for q15 in (False, True):
        s = FloatStream(c, g, q15=q15, chunk_frames=ch, output_filter=True)
        pr = torch.empty((ch, s.n_out), dtype=torch.float32, device=dev)
        c.use_torch_stream()
        for k0 in range(0, args.trace_pushes * ch, ch):
            s.push_t(x[k0 * hop:(k0 + ch) * hop], probs=pr)
        torch.cuda.synchronize()
        c.use_own_stream()
        s.close()
        emit(measure="trace_sequence", flow="q15" if q15 else "host", pushes=args.trace_pushes, chunk=ch, filter=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--pushes", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--trace-pushes", type=int, default=0)
    args = ap.parse_args()
    import torch
    from edison_amd import config as cfg
    from edison_amd.context import Context
    from edison_amd.kws.geometry import KwsGeometry
    from edison_amd.stream import FloatStream
    dev = torch.device("cuda", 0)
    c = Context(0, model_path=None)
    c.fnet_load(FIXTURE)
    g = KwsGeometry.from_config(net_input_scale=cfg.net_input_scale)
    if args.trace_pushes:
        trace(c, g, args)
        c.close()
        return 0
    board = c.device_info()["name"]
    n_out = c.fnet_info()["n_out"]
    hop, F, ch = g.frame_step, g.frame_count, args.chunk
    K = int(args.hours * 3600 * g.sample_rate) // hop // ch * ch   # whole pushes of the hour
    xh = audio(K * hop)
    x = torch.from_numpy(xh).to(dev)
    for q15 in (False, True):
        flow = "q15" if q15 else "host"
        lo = torch.empty((ch, n_out), dtype=torch.float32, device=dev)
        pr = torch.empty((ch, n_out), dtype=torch.float32, device=dev)
        am = torch.empty(ch, dtype=torch.int32, device=dev)
        s = FloatStream(c, g, q15=q15, chunk_frames=ch)
        c.use_torch_stream()

        def stream_hour():
            for k0 in range(0, K, ch):
                s.push_t(x[k0 * hop:(k0 + ch) * hop], logits=lo, probs=pr, argmax=am)
        stream_hour()   # warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        stream_hour()
        e1.record()
        torch.cuda.synchronize()
        sec = e0.elapsed_time(e1) / 1e3
        emit(board=board, flow=flow, measure="device_push", chunk=ch, inferences=K, seconds=round(sec, 6), inferences_per_s=round(K / sec, 1))
        # the batch call over the same windows: utterance u starts at u * hop, F frames each
        n_utt = K - (F - 1)
        blo = torch.empty((n_utt, n_out), dtype=torch.float32, device=dev)
        bpr = torch.empty((n_utt, n_out), dtype=torch.float32, device=dev)
        bam = torch.empty(n_utt, dtype=torch.int32, device=dev)
        c.kws_float_t(x, g, n_utt, hop, None, blo, bpr, bam, q15=q15)
        torch.cuda.synchronize()
        e0.record()
        c.kws_float_t(x, g, n_utt, hop, None, blo, bpr, bam, q15=q15)
        e1.record()
        torch.cuda.synchronize()
        sec = e0.elapsed_time(e1) / 1e3
        emit(board=board, flow=flow, measure="kws_float_batch", inferences=n_utt, seconds=round(sec, 6), inferences_per_s=round(n_utt / sec, 1))
        c.use_own_stream()
        s.close()
        s1 = FloatStream(c, g, q15=q15, chunk_frames=1)
        frames = [xh[i * hop:(i + 1) * hop].copy() for i in range(64)]
        emit(board=board, flow=flow, measure="host_push", chunk=1, **latency(s1.push, frames, args))
        s1.close()
    c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

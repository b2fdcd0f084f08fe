"""Cost of the exact KWS mode at config-3 size: bench.py's utterance mix, 262 144 utterances per step, the default KWS step and the
exact one interleaved in one process (blocks of K steps each, medians of the blocks), plus the flagged fraction.

    python tools/bench_kws_exact.py [--utts 262144] [--steps 10] [--blocks 6]

The flagging MFCC kernel's own cost against the default MFCC kernel, and the recompute's, come from a kernel trace of this script:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_kws_exact.py --blocks 2
(ed_mfcc2_kernel vs ed_mfcc2_flag_kernel, ed_mfcc_exact_kernel, ed_cnn_mfma_kernel in the stats file).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=6)
    args = ap.parse_args()
    import torch
    from bench import synth_utterances
    from edison_amd.context import Context
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    ctx.use_torch_stream()
    nu = args.utts
    audio = synth_utterances(nu, 21, dev)
    feat = torch.empty((nu, 403), dtype=torch.int8, device=dev)
    logits = torch.empty((nu, 10), dtype=torch.int8, device=dev)
    soft = torch.empty_like(logits)
    am = torch.empty((nu,), dtype=torch.int32, device=dev)

    def step(exact):
        ctx.kws_t(audio, nu, 31 * 1024, feat=feat, logits=logits, softmax=soft, argmax=am, exact=exact)

    def block(exact):
        for _ in range(args.warmup):
            step(exact)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.steps):
            step(exact)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    ms = {False: [], True: []}
    for b in range(args.blocks):
        for exact in ((False, True) if b % 2 == 0 else (True, False)):
            ms[exact].append(block(exact))
    step(True)
    flagged, frames = ctx.kws_exact_stats()
    d, e = float(np.median(ms[False])), float(np.median(ms[True]))
    print(json.dumps(dict(utts=nu, frames=frames, default_ms_per_step=round(d, 4), exact_ms_per_step=round(e, 4), ratio=round(e / d, 4),
                          flagged=flagged, flagged_fraction=round(flagged / frames, 5),
                          default_blocks=[round(x, 4) for x in ms[False]], exact_blocks=[round(x, 4) for x in ms[True]])), flush=True)
    ctx.use_own_stream()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

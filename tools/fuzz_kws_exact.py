"""Fuzz of the exact KWS mode against the float64 host flow (oracle.mfcc, variant B), >= 1 M frames over signal classes.

    python tools/fuzz_kws_exact.py [--utts-per-class 4230] [--seed 1]

Per class it prints one JSON line:
  ratio_max     max over frames and in-range coefficients c < 13 of |v32 - v64| / (2^-24 rms(frame)): the fp32 kernel's own error
                in the unit the flag bound uses (delta = K 2^-24 rms |scale|, K = ED_EXACT_K in edison_internal.h)
  flagged       fraction of frames the flagging kernel listed for the float64 recompute (edison_kws_exact_stats)
  default_diff  int8 features of the default (fp32) KWS path that differ from the oracle's
  exact_diff    the same for the exact mode: must be 0
The oracle runs on the CPU (n_threads) between the GPU calls, never inside a timed region (nothing here is timed).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K_EXACT = 10.0  # ED_EXACT_K
CLASSES = ["bench", "speech", "quiet", "dc", "oob_tone", "square", "impulse", "silence"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts-per-class", type=int, default=4230)  # 8 classes x 4230 x 31 = 1 049 040 frames
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threads", type=int, default=max(1, min(32, os.cpu_count() or 1)))
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  (torch's HIP runtime first, see tests/conftest.py)
    except ImportError:
        pass
    from oracle import oracle
    from edison_amd.context import Context
    from test_gpu_kws_exact import _fill, UL
    oracle.build()
    ctx = Context(0)
    model = oracle.Model()
    total = dict(frames=0, exact_diff=0, ratio_max=0.0)
    for ci, kind in enumerate(CLASSES):
        rng = np.random.default_rng(args.seed * 1000 + ci)
        a = np.zeros((args.utts_per_class, UL), np.int16)
        _fill(a, kind, rng)
        x = a.reshape(-1)
        nf = x.size // 1024
        v32 = ctx.mfcc(x, n_frames=nf, n_coef=13)                                  # the fast fp32 kernel, variant B
        v64 = oracle.mfcc(x, 1, n_frames=nf, n_threads=args.threads)[:, :13]
        fr = x.reshape(nf, 1024)
        rms = np.concatenate([np.sqrt(np.square(fr[i:i + 8192], dtype=np.float64).mean(axis=1)) for i in range(0, nf, 8192)])
        inr = (v64 >= -128.0) & (v64 < 127.0)
        err = np.where(inr, np.abs(v32.astype(np.float64) - v64), 0.0).max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(rms > 0, err / (2.0 ** -24 * rms), np.where(err > 0, np.inf, 0.0))
        ref = oracle.net_input(v64).reshape(-1, 403)
        d = ctx.kws(x, n_utt=a.shape[0], utt_stride=UL, exact=False)
        e = ctx.kws(x, n_utt=a.shape[0], utt_stride=UL, exact=True)
        flagged, frames = ctx.kws_exact_stats()
        ro = oracle.cnn(model, ref, n_threads=args.threads)
        line = dict(cls=kind, frames=int(nf), ratio_max=round(float(ratio.max()), 4),
                    ratio_p999=round(float(np.quantile(ratio, 0.999)), 4), flagged=round(flagged / frames, 5),
                    default_diff=int((d["feat"] != ref).sum()), exact_diff=int((e["feat"] != ref).sum()),
                    exact_argmax_diff=int((e["argmax"] != ro["argmax"]).sum()), default_argmax_diff=int((d["argmax"] != ro["argmax"]).sum()))
        print(json.dumps(line), flush=True)
        total["frames"] += int(nf)
        total["exact_diff"] += line["exact_diff"] + line["exact_argmax_diff"]
        total["ratio_max"] = max(total["ratio_max"], line["ratio_max"])
    total["K"] = K_EXACT
    total["margin"] = round(K_EXACT / total["ratio_max"], 2) if total["ratio_max"] > 0 else None
    print(json.dumps(dict(summary=total)), flush=True)
    ctx.close()
    return 0 if total["exact_diff"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

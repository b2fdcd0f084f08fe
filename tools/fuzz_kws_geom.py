"""Fuzz of the any-geometry KWS features (edison_kws_geom_batch) against the reference host flow restated (oracle.mfcc_numpy, float64,
then oracle.net_input), >= 1 M frames over the five geometries of tests/test_gpu_kws_geom.py and its signal mix -- or, with --sweep,
over the rows of tests/geom_sweep.py (every code path of the kernel; each row at the sensitive net_input_scale and with the one-Dense
graph of tests/test_gpu_geom_sweep.py, its level-normalised signal mix).

    python tools/fuzz_kws_geom.py [--sweep] [--frames-per-geometry N] [--seed 1] [--jobs 8]

--frames-per-geometry defaults to 210 000 for the five geometries and to max(20 000, 1.05 M / rows) with --sweep.

One JSON line per geometry: frames, features compared, differences. A difference is listed with its utterance, frame and coefficient,
the two int8 values and the distance of the oracle's float32 value (mfcc * scale) to the nearest rounding boundary x.5 -- it is a
finding to explain, not a tolerance to widen. The oracle runs on the CPU in worker processes before the GPU is opened.
"""
import argparse
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _oracle_chunk(job):
    g, lo, audio = job
    from oracle import oracle
    import geom_sweep as gs
    return lo, gs.oracle_feat(oracle, gs.oracle_mfcc(oracle, audio, g), g)


def _cases(args):
    """name -> (geometry, audio [n_utt][n_samples], a function that loads the row's graph into a context)."""
    from geom_sweep import GEOMS, geom, header, signals
    out = {}
    if not args.sweep:
        for name in sorted(GEOMS):
            g = geom(**GEOMS[name])
            n_utt = -(-args.frames_per_geometry // g.frame_count)
            out[name] = (g, signals(n_utt, g.n_samples, args.seed), lambda c, name=name: c.load_weights_h(header(name)))
        return out
    from dataclasses import replace
    from oracle import oracle
    import geom_sweep as gs
    for name in sorted(gs.ROWS):
        g = gs.geometry(name)
        # the scale of tests/test_gpu_geom_sweep.py: from the oracle's coefficients over the test's own audio of the row
        g = replace(g, net_input_scale=gs.sensitive_scale(gs.oracle_mfcc(oracle, gs.row_signals(name, g, gs.min_frames(name)), g)))
        out[name] = (g, gs.row_signals(name, g, args.frames_per_geometry, seed=args.seed),
                     lambda c, name=name, g=g: c.load_model_bytes(gs.dense_graph(g, seed=sorted(gs.ROWS).index(name))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true", help="the rows of tests/geom_sweep.py instead of the five geometries")
    ap.add_argument("--frames-per-geometry", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--jobs", type=int, default=max(1, min(16, os.cpu_count() or 1)))
    args = ap.parse_args()
    from oracle import oracle
    oracle.build()
    if not args.frames_per_geometry:
        if args.sweep:
            import geom_sweep as gs
            args.frames_per_geometry = max(20000, -(-1050000 // len(gs.ROWS)))
        else:
            args.frames_per_geometry = 210000
    cases = _cases(args)
    plan, want = {}, {}
    for name, (g, audio, _) in cases.items():
        n_utt = audio.shape[0]
        plan[name] = n_utt
        step = -(-n_utt // (4 * args.jobs))
        jobs = [(g, lo, audio[lo:lo + step]) for lo in range(0, n_utt, step)]
        want[name] = np.zeros((n_utt, g.n_features), np.int8)
        with ProcessPoolExecutor(args.jobs) as ex:
            for lo, f in ex.map(_oracle_chunk, jobs):
                want[name][lo:lo + f.shape[0]] = f
    from edison_amd.context import Context
    total = 0
    for name, (g, audio, load) in cases.items():
        c = Context(0, model_path=None)
        load(c)
        got = c.kws_geom(audio, g)["feat"]
        bad = np.argwhere(got != want[name])
        finds = []
        for u, i in bad[:20]:
            f, k = divmod(int(i), g.num_mfcc)
            span = (g.frame_count - 1) * g.frame_step + g.frame_len
            m = oracle.mfcc_numpy(audio[u, :span], oracle.VARIANT_A if g.variant == 0 else oracle.VARIANT_B, g.frame_len, g.frame_step,
                                  n_frames=g.frame_count, num_mel_bins=g.mel_nbins, sample_rate=g.sample_rate, lower_edge_hertz=g.lower_edge_hertz,
                                  upper_edge_hertz=g.upper_edge_hertz, mel_mtx_scale=g.mel_mtx_scale, use_log=g.use_log)
            v = float(np.float32(m[f, g.first_mfcc + k]) * np.float32(g.net_input_scale))
            finds.append(dict(utt=int(u), frame=f, coef=g.first_mfcc + k, got=int(got[u, i]), oracle=int(want[name][u, i]), value=v,
                              to_boundary=abs(abs(v - np.floor(v)) - 0.5)))
        frames = plan[name] * g.frame_count
        total += frames
        print(json.dumps(dict(geometry=name, frame_len=g.frame_len, mel_nbins=g.mel_nbins, net_input_scale=g.net_input_scale, utts=plan[name],
                              frames=frames, features=int(got.size),
                              differences=int(bad.shape[0]), findings=finds)), flush=True)
        c.close()
    print(json.dumps(dict(total_frames=total)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

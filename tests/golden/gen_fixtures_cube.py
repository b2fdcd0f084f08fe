#!/usr/bin/env python3
"""The reference's X-CUBE-AI float network as a data fixture, and golden vectors for it. Build container only (needs the reference).

cube_kws.ednf: edison_amd/cube_import.py on firmware/src/ai/cube/kws/kws.c + kws_data.c + keywords.txt (171 944 bytes of float32
  weights, BatchNorms folded in by X-CUBE-AI).
cube_golden.npz, for both reference wavs (edge-padded to 2 s, kws_on_mcu.py:330-334) and seeded noise:
  audio_<s>      int16 [32000]
  net_in_<s>     float32 [403]: the host flow's net input -- the reference's own mfcc_mcu (variant B, first 13 coefficients) cast to
                 float32, times net_input_scale, clipped to [-2^15, 2^15 - 1] (kws_on_mcu.py:343-347, audio/config.py:46-48), never rounded
  logits_<s>, probs_<s>   float64 [10]: tests/fnet_host.py (the float64 restatement) on net_in_<s>
  q15_<s>        int16 [31][13]: variant C (the firmware's audioCalcMFCCs, this repo's oracle, bit-exact to the firmware) on the first
                 31 744 samples; the firmware flow casts them to float with no scale and no clip (app.c:675-683)
  q15_logits_<s>, q15_probs_<s>  float64 [10]: the restatement on (float)q15_<s>
Re-run:  python3 tests/golden/gen_fixtures_cube.py
"""
import os
import sys

import numpy as np
import scipy.io.wavfile as wavfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
CUBE = os.path.join(REF, "firmware/src/ai/cube/kws")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "audio"))

import config as refcfg                      # noqa: E402  (reference audio/config.py)
import edison.mfcc.mfcc_utils as mfu         # noqa: E402  (reference implementation of variant B)
import fnet_host  # noqa: E402
from edison_amd import cube_import           # noqa: E402
from oracle import oracle                    # noqa: E402


def host_net_input(data):
    n = refcfg.nSamples
    o = mfu.mfcc_mcu(data, refcfg.fs, n, refcfg.frame_len, refcfg.frame_step, refcfg.frame_count, refcfg.fft_len,
                     refcfg.num_mel_bins, refcfg.lower_edge_hertz, refcfg.upper_edge_hertz, refcfg.mel_mtx_scale)
    m = np.array([f["mfcc"][:refcfg.num_mfcc] for f in o])
    x = np.array(m.reshape([1, 31, 13, 1]), dtype="float32") * refcfg.net_input_scale
    return np.clip(x, refcfg.net_input_clip_min, refcfg.net_input_clip_max).reshape(-1)


def main():
    blob = cube_import.import_files(os.path.join(CUBE, "kws.c"), os.path.join(CUBE, "kws_data.c"), os.path.join(CUBE, "keywords.txt"))
    with open(os.path.join(HERE, "cube_kws.ednf"), "wb") as f:
        f.write(blob)
    model = fnet_host.load(blob)
    oracle.build()
    n = refcfg.nSamples
    sources = {}
    for name, wav in (("edison", "edison_16k_16b.wav"), ("hey", "hey_short_16k.wav")):
        fs, x = wavfile.read(os.path.join(REF, "audio/data", wav))
        assert fs == 16000 and x.dtype == np.int16
        sources[name] = (np.pad(x, (0, n - x.shape[0]), mode="edge") if x.shape[0] < n else x[:n]).astype(np.int16)
    rng = np.random.default_rng(1405)
    for i in range(3):
        sources["noise%d" % i] = np.clip(rng.normal(0, 1000 * (i + 1), n), -32768, 32767).astype(np.int16)
    out = dict(names=np.array(sorted(sources)))
    for name, data in sources.items():
        out["audio_" + name] = data
        x = host_net_input(data)
        out["net_in_" + name] = x
        r = fnet_host.run64(model, x[None])
        out["logits_" + name], out["probs_" + name] = r["logits"][0], r["probs"][0]
        q = oracle.mfcc_q15(data[:31 * 1024])[:, :13].astype(np.int16)
        out["q15_" + name] = q
        rq = fnet_host.run64(model, q.astype(np.float32).reshape(1, -1))
        out["q15_logits_" + name], out["q15_probs_" + name] = rq["logits"][0], rq["probs"][0]
        print("%-8s host %-8s p=%.4f | firmware %-8s p=%.4f" % (name, model["keywords"][r["argmax"][0]], r["probs"][0].max(),
                                                             model["keywords"][rq["argmax"][0]], rq["probs"][0].max()))
    np.savez_compressed(os.path.join(HERE, "cube_golden.npz"), **out)


if __name__ == "__main__":
    main()

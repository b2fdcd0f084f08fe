"""``kws quantize <net.ednf> <audio.npy> <out.ednn>`` -- quantise a float32 X-CUBE-AI network to an int8 NNoM graph, calibrated on the
GPU over a set of utterances (``Context.quantize``, edison_amd/calibrate.py and quantize.py): what the reference
does with ``generate_model(model, x, name=.../weights.h)`` (kws_nnom.py:305).

    audio.npy       int16 [n, samples] or a flat stream of utterances: the calibration set
    --weights-h f   also write the NNoM model header of the graph, for the firmware
    --saturate s    let the share s of each activation's values saturate (method "saturate") instead of covering the maximum
    --geometry      the MFCC geometry of the float network's features, as in ``kws eval``      --chunk N   utterances per launch

Prints the report (every dec and shift, the quantisation RMS error of each tensor, the net_input_scale the int8 graph's features need)
and how often the int8 graph's class equals the float network's on the calibration set.
"""
import sys

import numpy as np

USAGE = "usage: kws quantize <net.ednf> <audio.npy> <out.ednn> [--weights-h <out.h>] [--saturate <share>] [--geometry k=v,...] [--chunk N]"


def run(net, audio_path, out_path, weights_h=None, saturate=None, geometry=None, chunk=16384, ctx=None, out=None):
    from .. import config as cfg, quantize as qz
    from ..context import default_context
    from .kws_eval import parse_geometry
    out = out or sys.stdout
    ctx = ctx or default_context()
    audio = np.load(audio_path)
    ctx.fnet_load(net)
    g = parse_geometry(geometry, net_input_scale=cfg.net_input_scale) if geometry else None
    method = dict(method="saturate", saturate=float(saturate)) if saturate is not None else dict(method="max_min")
    blob, rep = ctx.quantize(audio, geometry=g, chunk=chunk, return_features=True, **method)
    with open(out_path, "wb") as f:
        f.write(blob)
    if weights_h:
        with open(weights_h, "w") as f:
            f.write(qz.write_weights_h(rep["graph"], rep["in_shape"], rep["input"]["dec"]))
    out.write(qz.format_report(rep) + "\n")
    # the int8 graph on the calibration set's own features against the float network
    n = len(rep["float_argmax"])
    if n:
        ctx.load_model_bytes(blob)
        q = ctx.net(qz.quantize_input(rep["features"], rep["input"]["dec"]))["argmax"]
        same = int((q == rep["float_argmax"]).sum())
        out.write("int8 argmax equals the float argmax on %d of %d calibration utterances (%.2f %%)\n" % (same, n, 100.0 * same / n))
        rep["agreement"] = same / n
    out.write("wrote %s: %d bytes%s\n" % (out_path, len(blob), ", and %s" % weights_h if weights_h else ""))
    return blob, rep


def main(argv):
    opts = {"--weights-h": None, "--saturate": None, "--geometry": None, "--chunk": "16384"}
    rest = []
    i = 1
    while i < len(argv):
        if argv[i] in opts:
            if i + 1 >= len(argv):
                print("%s needs a value" % argv[i])
                return 1
            opts[argv[i]] = argv[i + 1]
            i += 2
        else:
            rest.append(argv[i])
            i += 1
    if len(rest) != 3:
        print(USAGE)
        return 1
    try:
        chunk = int(opts["--chunk"])
        saturate = None if opts["--saturate"] is None else float(opts["--saturate"])
    except ValueError:
        print(USAGE)
        return 1
    from ..quantize import QuantizeError
    try:
        run(rest[0], rest[1], rest[2], weights_h=opts["--weights-h"], saturate=saturate, geometry=opts["--geometry"], chunk=chunk)
    except QuantizeError as e:
        print("kws quantize: %s" % e)
        return 1
    return 0

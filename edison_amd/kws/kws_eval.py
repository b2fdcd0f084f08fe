"""``kws eval <audio.npy> <labels.npy>`` -- the confusion matrix and top-k accuracy of a network on a labelled data set, counted on
the GPU (``Context.evaluate``, edison_amd/evaluate.py): what the reference prints with NNoM's prediction_summary for the quantised
graph (nnom_utils.c:178-254) and with predictWithConfMatrix for the float model (kws_nnom.py:327-333).

    audio.npy    int16 [n, samples] (the reference's cached x_*.npy before feature extraction) or a flat stream of utterances
    labels.npy   [n] class indices, or the reference's one-hot y_*.npy [n, classes]; -1 marks an unlabelled utterance
    --graph f    an int8 graph (.ednn, or an NNoM weights.h) instead of the shipped one
    --net f      a float32 X-CUBE-AI network (.ednf): scored with the float model's rule (first class above 0.5)
    --geometry   the MFCC geometry the network was trained at, as name=value pairs of kws.geometry.KwsGeometry separated by commas,
                 e.g. frame_len=640,frame_step=320,num_mfcc=10 (default: audio/config.py's, on the shipped fast path)
    --top-k K    ranks to report (default 2)      --chunk N    utterances per launch (default 16384)
"""
import sys

import numpy as np

USAGE = "usage: kws eval <audio.npy> <labels.npy> [--graph <file.ednn|weights.h> | --net <file.ednf>] [--geometry k=v,...] [--top-k K] [--chunk N]"


def parse_geometry(text, **base):
    from .geometry import KwsGeometry
    fields = KwsGeometry.__dataclass_fields__
    changes = dict(base)
    for item in text.split(","):
        k, _, v = item.partition("=")
        k = k.strip()
        if k == "frame_count":
            k = "frame_count_"
        if k not in fields:
            raise ValueError("unknown geometry field %r" % k)
        kind = fields[k].type
        changes[k] = (v.strip().lower() in ("1", "true", "yes")) if kind is bool else (int(v) if kind is int else float(v))
    return KwsGeometry.from_config(**changes)


def run(audio_path, labels_path, graph=None, net=None, geometry=None, top_k=2, chunk=16384, ctx=None, out=None):
    from .. import config as cfg
    from ..context import default_context
    out = out or sys.stdout
    ctx = ctx or default_context()
    audio, labels = np.load(audio_path), np.load(labels_path)
    if net is not None:
        ctx.fnet_load(net, large=True)   # a network that exceeds the LDS runs layer by layer; one that fits loads as ever
        g = parse_geometry(geometry, net_input_scale=cfg.net_input_scale) if geometry else None
        res = ctx.evaluate(audio, labels, flow="kws_float", chunk=chunk, top_k=top_k, geometry=g)
    else:
        if graph is not None:
            (ctx.load_weights_h if str(graph).endswith(".h") else ctx.load_model)(graph)
        if geometry:
            res = ctx.evaluate(audio, labels, flow="kws_geom", chunk=chunk, top_k=top_k, geometry=parse_geometry(geometry))
        else:
            res = ctx.evaluate(audio, labels, flow="kws", chunk=chunk, top_k=top_k)
    out.write(res.summary())
    if res.skipped:
        out.write("Unlabelled: %d\n" % res.skipped)
    return res


def main(argv):
    opts = {"--graph": None, "--net": None, "--geometry": None, "--top-k": "2", "--chunk": "16384"}
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
    if len(rest) != 2 or (opts["--graph"] and opts["--net"]):
        print(USAGE)
        return 1
    try:
        top_k, chunk = int(opts["--top-k"]), int(opts["--chunk"])
    except ValueError:
        print(USAGE)
        return 1
    run(rest[0], rest[1], graph=opts["--graph"], net=opts["--net"], geometry=opts["--geometry"], top_k=top_k, chunk=chunk)
    return 0

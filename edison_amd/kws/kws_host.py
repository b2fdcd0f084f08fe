"""Host keyword-spotting flow on the MI355X -- the counterpart of the *host* leg of the reference's
``audio/edison/kws/kws_on_mcu.py`` (``fileInference`` :273-308, ``frameInference`` :310-401) and of
``audio/edison/train/kws_nnom.py testfile`` (:335-361), with the board leg (UART) replaced by the GPU:

    wav -> int16 -> pad/cut to 32000 samples -> MFCC variant B -> first 13 coefficients
        -> clip(x*1, -128, 127).round() -> int8 [31][13] -> int8 CNN -> softmax int8[10] -> argmax -> keyword

Everything after the pad/cut runs in ONE C-ABI call (``edison_kws_batch``): the features never visit the host
unless asked for.
"""
import sys

import numpy as np

from .. import config as cfg
from ..context import KEYWORDS, default_context


def read_wav(path):
    """16 kHz wav -> int16 samples; float wavs are scaled like kws_on_mcu.py:328-329."""
    import scipy.io.wavfile as wavfile
    in_fs, data = wavfile.read(path)
    if in_fs != cfg.fs:
        raise ValueError("Sample rate of file %d doesn't match %d" % (in_fs, cfg.fs))
    if data.ndim > 1:
        data = data[:, 0]
    if data.dtype == np.float32 or data.dtype == np.float64:
        data = ((2 ** 15 - 1) * data).astype('int16')
    return np.asarray(data, dtype=np.int16)


def pad_or_cut(data, n=cfg.nSamples, mode="zero"):
    """kws_on_mcu.py:287-290 (zero pad, ``fileInference``) / :331-334 (edge pad, ``frameInference``)."""
    if data.shape[0] < n:
        if mode == "edge":
            return np.pad(data, (0, n - data.shape[0]), mode='edge')
        return np.pad(data, (0, n - data.shape[0]))
    return data[:n]


def infer_utterances(audio, ctx=None, exact=None, geometry=None):
    """audio: int16 [n_utt, >=31744] (or 1-D single utterance). Returns the dict of ``Context.kws``. exact: True gives the
    features, logits and argmax of the reference's float64 host flow (``Context.kws_exact``); None keeps the context's mode.
    geometry: a ``kws.geometry.KwsGeometry`` for a graph trained at another MFCC geometry -- each utterance is zero-padded or cut to
    geometry.n_samples and goes through ``Context.kws_geom`` (float64 features already; `exact` does not apply)."""
    ctx = ctx or default_context()
    a = np.atleast_2d(np.asarray(audio, dtype=np.int16))
    if geometry is not None:
        a = np.stack([pad_or_cut(row, geometry.n_samples) for row in a])
        return ctx.kws_geom(np.ascontiguousarray(a), geometry, n_utt=a.shape[0], utt_stride=geometry.n_samples)
    return ctx.kws(np.ascontiguousarray(a), n_utt=a.shape[0], utt_stride=a.shape[1], exact=exact)


def report(res, i=0, out=None):
    """Prediction line in the spirit of kws_on_mcu.report (:148-157): int8 softmax / 127 and the class."""
    out = out or sys.stdout  # looked up per call: a default bound at import time may be a stream that is closed by now
    np.set_printoptions(precision=3, suppress=True)
    probs = res["softmax"][i].astype(np.float32) / 127.0
    k = int(res["argmax"][i])
    print('gpu prediction:', probs, KEYWORDS[k], file=out)
    print('dense logits  :', res["logits"][i], file=out)
    return KEYWORDS[k]


def file_inference(path, pad_mode="zero", ctx=None, verbose=True, exact=None, geometry=None):
    """One wav through the host flow. geometry: the MFCC geometry of a graph trained at another one (``kws.geometry.KwsGeometry``);
    the wav is then padded or cut to geometry.n_samples and runs through ``Context.kws_geom``. None: audio/config.py's, as before."""
    if geometry is not None:
        data = pad_or_cut(read_wav(path), n=geometry.n_samples, mode=pad_mode)
        res = infer_utterances(data, ctx, geometry=geometry)
        k = int(res["argmax"][0])
        res["keyword"] = KEYWORDS[k] if res["logits"].shape[1] == len(KEYWORDS) else str(k)
        if verbose:
            print('net input (int8, %dx%d):' % (geometry.frame_count, geometry.num_mfcc))
            print(res["feat"].reshape(geometry.frame_count, geometry.num_mfcc))
            if res["softmax"] is not None and res["softmax"].shape[1] == len(KEYWORDS):
                report(res)
        return res
    data = pad_or_cut(read_wav(path), mode=pad_mode)
    res = infer_utterances(data, ctx, exact=exact)
    res["keyword"] = KEYWORDS[int(res["argmax"][0])]
    if verbose:
        print('net input (int8, 31x13):')
        print(res["feat"].reshape(cfg.n_frames, cfg.num_mfcc))
        report(res)
    return res


def rmse(a, b):
    return np.sqrt(np.mean((a - b) ** 2))


def compare(data_a, data_b, name, out=None):
    """The comparison block of kws_on_mcu.compare (:159-168), same wording and number formats."""
    dev = 100.0 * (1.0 - (data_b.ravel() + 1e-9) / (data_a.ravel() + 1e-9))
    out = out or sys.stdout
    print('_________________________________________________________________', file=out)
    print('Comparing: %s' % (name), file=out)
    print("Deviation: max %.3f%% min %.3f%% avg %.3f%% \nrmse %.3f" % (
        dev.max(), dev.min(), np.mean(dev), rmse(data_b.ravel(), data_a.ravel())), file=out)
    print('scale %.3f=1/%.3f' % (data_b.max() / data_a.max(), data_a.max() / data_b.max()), file=out)
    print('correlation coeff %.3f' % (np.corrcoef(data_a.ravel(), data_b.ravel())[0, 1]), file=out)
    print('_________________________________________________________________', file=out)


def frame_inference(path, ctx=None, out=None, exact=None):
    """`kws mcu file <wav>` = kws_on_mcu.frameInference (:310-401): the wav (edge-padded to 2 s) through the host
    leg (MFCC variant B) and through the board's leg -- here the GPU's variant C, i.e. the firmware's own Q15
    arithmetic -- each followed by the int8 network, then the two comparison blocks the reference prints
    (README.md:121-139 shows them for data/edison_16k_16b.wav)."""
    out = out or sys.stdout
    from .. import _lib
    ctx = ctx or default_context()
    data = pad_or_cut(read_wav(path), mode="edge")
    np.set_printoptions(precision=3, suppress=True)
    host = ctx.kws(data, n_utt=1, utt_stride=data.shape[0], exact=exact)
    mcu = ctx.kws(data, n_utt=1, utt_stride=data.shape[0], q15=True)
    host_pred = host["softmax"][0].astype(np.float32) / 127.0
    mcu_pred = mcu["softmax"][0].astype(np.float32) / 127.0
    print('keywords:', list(KEYWORDS), file=out)
    print('host prediction:', host_pred, KEYWORDS[int(host["argmax"][0])], file=out)
    print('mcu prediction: ', mcu_pred, KEYWORDS[int(mcu["argmax"][0])], file=out)
    print('rmse:', rmse(host_pred, mcu_pred), file=out)
    compare(host_pred, mcu_pred, 'predictions', out)
    # the MFCC block compares the unclipped coefficients, float32 like the reference's arrays (:346, app.c:212)
    host_mfcc = ctx.mfcc(data, variant=_lib.MFCC_B, n_coef=cfg.num_mfcc).astype(np.float32)
    mcu_mfcc = ctx.mfcc_q15(data, n_coef=cfg.num_mfcc).astype(np.float32)
    compare(host_mfcc, mcu_mfcc, 'MFCC=net input', out)
    return dict(host=host, mcu=mcu, host_mfcc=host_mfcc, mcu_mfcc=mcu_mfcc)


def single_inference(repeat=1, ctx=None, out=None):
    """`kws mcu single [n]` = kws_on_mcu.singleInference (:236-270), nnom branch: the all-zero int8 net input."""
    out = out or sys.stdout
    ctx = ctx or default_context()
    res = None
    for _ in range(max(1, int(repeat))):
        res = ctx.cnn(np.zeros((1, cfg.n_frames * cfg.num_mfcc), np.int8))
        report(res, 0, out)
    return res


def _float_keywords(net):
    from ..cube_import import read_blob
    with open(net, "rb") as f:
        kw = read_blob(f.read())["keywords"]
    return kw or list(KEYWORDS)


def float_report(host_pred, mcu_pred=None, keywords=KEYWORDS, out=None):
    """kws_on_mcu.report (:148-157) for the float network's probabilities; without an MCU leg only the host line."""
    out = out or sys.stdout
    np.set_printoptions(precision=3, suppress=True)
    print('keywords:', list(keywords), file=out)
    print('host prediction:', host_pred, keywords[int(host_pred.argmax())], file=out)
    if mcu_pred is not None:
        print('mcu prediction: ', mcu_pred, keywords[int(mcu_pred.argmax())], file=out)
        print('rmse:', rmse(host_pred, mcu_pred), file=out)


def float_file_inference(path, net, pad_mode="zero", ctx=None, out=None):
    """`kws mcu fileinf|frame <wav> --net <file.ednf>`: the wav through the X-CUBE-AI float network's host flow (kws_on_mcu.py:343-348,
    net_type 'cube'): float64 MFCC variant B -> first 13 -> float32 x net_input_scale -> clip(-32768, 32767) -> the network."""
    ctx = ctx or default_context()
    ctx.fnet_load(net, large=True)   # a network that exceeds the LDS runs layer by layer; one that fits loads as ever
    data = pad_or_cut(read_wav(path), mode=pad_mode)
    res = ctx.kws_float(data, n_utt=1)
    kw = _float_keywords(net)
    float_report(res["probs"][0], keywords=kw, out=out)
    res["keyword"] = kw[int(res["argmax"][0])] if int(res["argmax"][0]) < len(kw) else str(int(res["argmax"][0]))
    return res


def float_frame_inference(path, net, ctx=None, out=None):
    """`kws mcu file <wav> --net <file.ednf>`: the host flow and the firmware's (variant C -> (float), app.c:675-683) through the float
    network, printed as kws_on_mcu.report (:148-157) prints them, then the comparison block of the predictions."""
    out = out or sys.stdout
    ctx = ctx or default_context()
    ctx.fnet_load(net, large=True)   # a network that exceeds the LDS runs layer by layer; one that fits loads as ever
    data = pad_or_cut(read_wav(path), mode="edge")
    host = ctx.kws_float(data, n_utt=1)
    mcu = ctx.kws_float(data, n_utt=1, q15=True)
    float_report(host["probs"][0], mcu["probs"][0], _float_keywords(net), out)
    compare(host["probs"][0], mcu["probs"][0], 'predictions', out)
    return dict(host=host, mcu=mcu)


def nnom_example(path, graph, labels=None, feature_offset=1, dec_bits=8, preemph=0.97, ctx=None, out=None):
    """`kws mcu nnom <wav> --graph <weights.h | file.ednn> [--labels <file>]`: the firmware's NNoM keyword-spotting example
    (appNnomKwsRun, app.c:545-623) over a wav file on the GPU. The graph's input rows x n x 1 gives the window and the extractor,
    mfcc_create(n + feature_offset, feature_offset, 512, dec_bits, preemph); every 512 samples are one audio event (the last one
    padded with zeros), and every event prints `label : pct%` as app.c:620 does. labels: one class name per line."""
    from ..context import Context
    from ..mfcc.mfcc_f32 import NnomKwsFrontEnd
    out = out or sys.stdout
    ctx = ctx or Context(model_path=None)
    if str(graph).endswith(".h"):
        ctx.load_weights_h(graph)
    else:
        ctx.load_model(graph)
    info = ctx.net_info()
    names = None
    if labels is not None:
        with open(labels) as f:
            names = [line.strip() for line in f if line.strip()]
    data = np.asarray(read_wav(path), dtype=np.int16).ravel()
    data = np.concatenate([data, np.zeros(-data.size % 512, np.int16)])
    fe = NnomKwsFrontEnd(ctx=ctx, window_rows=info["in_h"], num_mfcc_features=info["in_w"] + int(feature_offset), feature_offset=int(feature_offset),
                         mfcc_dec_bits=int(dec_bits), preemph=float(preemph))
    try:
        res = fe.predict(data, labels=names)
    finally:
        fe.close()
    for i, (lb, pr) in enumerate(zip(res["label"], res["prob"])):
        print("%s : %d%%" % (res["names"][i] if names else int(lb), int(pr * 100)), file=out)
    return res


# the reference's own function names and call conventions (kws_on_mcu.py:243,273,310: `args` = the CLI's remaining
# arguments, args[0] = the wav file)
def singleInference(repeat=1):
    return single_inference(repeat)


def fileInference(args):
    return file_inference(args[0])


def frameInference(args):
    return frame_inference(args[0])


def main(argv):
    """``kws mcu <mode> [file]`` of the reference's CLI (main.py:146-165, kws_on_mcu.py:650-690). The modes that record
    from a microphone (mic, host, hostcont, hostsingle, miccont) are not part of this port."""
    net = None
    if "--net" in argv:
        i = argv.index("--net")
        if i + 1 >= len(argv):
            print('--net needs an .ednf file')
            return 1
        net = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    opts = {}
    for flag in ("--graph", "--labels"):
        if flag in argv:
            i = argv.index(flag)
            if i + 1 >= len(argv):
                print('%s needs a file' % flag)
                return 1
            opts[flag] = argv[i + 1]
            argv = argv[:i] + argv[i + 2:]
    if len(argv) < 2:
        print('usage: kws mcu <single [n] | fileinf <wav> | file <wav> | frame <wav>> [--net <file.ednf>]\n'
              '       kws mcu nnom <wav> --graph <weights.h | file.ednn> [--labels <file>]')
        return 1
    mode = argv[1]
    print('Running mode', mode, 'with args', argv[2:])
    if mode == "nnom":
        if len(argv) < 3 or "--graph" not in opts:
            print('need a wav file and --graph <weights.h | file.ednn>')
            return 1
        nnom_example(argv[2], opts["--graph"], labels=opts.get("--labels"))
        return 0
    if mode == "single":
        single_inference(int(argv[2]) if len(argv) > 2 else 1)
        return 0
    if mode in ("file", "fileinf", "frame", "host"):
        if len(argv) < 3:
            print('need a wav file')
            return 1
        if net is not None and mode != "host":
            if mode == "file":
                float_frame_inference(argv[2], net)
            else:
                float_file_inference(argv[2], net, pad_mode="edge" if mode == "frame" else "zero")
            return 0
        if mode == "file":
            frame_inference(argv[2])
        else:
            file_inference(argv[2], pad_mode="edge" if mode == "frame" else "zero")
        return 0
    print('mode %r records from a microphone, which this port does not drive' % mode)
    return 1

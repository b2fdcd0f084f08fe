"""``kws live <host|mcu> <wav>`` -- the firmware's continuous mode (firmware/src/app.c:288-371) replayed on a wav file.

The reference's ``audio/edison/kws/kws_live.py`` listens to a microphone; the signal path behind the microphone is
what this module runs, frame by frame, on the GPU: 1024-sample frames -> MFCC -> 31-row sliding window -> int8 network
-> moving average over the outputs -> maximum / threshold -> wake-word state machine. ``host`` uses the host float
model of the features (variant B), ``mcu`` the firmware's own Q15 arithmetic (variant C). The printed lines follow the
firmware's UART log (app.c:330-353). ``--net <file.ednf>`` runs the float32 X-CUBE-AI network instead of the int8 graph: the
firmware's default build (NET_TYPE_CUBE), whose moving average uses alpha 0.5 (app.c:35-36). With ``--net``, several wav files run as
the microphones of one bank (``stream.FloatBank``): ``kws live <host|mcu> a.wav b.wav ... --net <file.ednf>``.
"""
import sys

import numpy as np

from .. import config as cfg
from ..context import KEYWORDS, default_context
from ..stream import FloatBank, FloatStream, Fsm, GeomStream, Stream, StreamBank
from .kws_host import read_wav


def netOutFilt(net_outs, alpha):
    """The host-side moving average of the reference's live view (kws_live.py:139-152): row 0 is all zeros, row i+1 =
    alpha * row i + (1 - alpha) * net_outs[i], in float64 like the reference's Python floats. (The firmware's own
    filter -- float32 state, double arithmetic, app.c:332-356 -- is the stream's `output_filter` option.)"""
    x = np.asarray(net_outs, dtype=np.float64)
    flt = np.zeros((x.shape[0] + 1, x.shape[1]), dtype=np.float64)
    for i in range(x.shape[0]):
        flt[i + 1] = alpha * flt[i] + (1.0 - alpha) * x[i]
    return flt


def run(path, q15=False, ctx=None, out=None, alpha=None, threshold=0.5, geometry=None, net=None):
    """geometry (kws.geometry.KwsGeometry): a graph trained at that MFCC geometry, on a GeomStream whose hop is geometry.frame_step
    (float64 features, q15 does not apply); the state machine runs, and its lines are printed, only for a graph with 10 outputs.
    net (an .ednf path or its bytes): the float32 X-CUBE-AI network, loaded on ctx, on a FloatStream (host flow at `geometry`, default
    audio/config.py's; q15: the firmware's flow); class names from the .ednf. alpha: the moving average's, default 0.9 for the int8
    graph (app.c:38) and 0.5 for the float network (app.c:35-36).
    path may be a list of wav files, with geometry or net: the microphones of one StreamBank or FloatBank (run_bank)."""
    if not isinstance(path, (str, bytes)) and hasattr(path, "__len__"):
        if len(path) != 1:
            return run_bank(path, ctx=ctx, out=out, alpha=alpha, threshold=threshold, geometry=geometry, net=net, q15=q15)
        path = path[0]
    out = out or sys.stdout
    ctx = ctx or default_context()
    if alpha is None:
        alpha = 0.9 if net is None else 0.5
    data = read_wav(path)
    if net is not None:
        ctx.fnet_load(net)
        if geometry is None:
            from ..kws.geometry import KwsGeometry
            geometry = KwsGeometry.from_config(net_input_scale=cfg.net_input_scale)
    hop = cfg.frame_length if geometry is None else int(geometry.frame_step)
    n = -(-data.shape[0] // hop)
    data = np.pad(data, (0, n * hop - data.shape[0]))
    # the firmware's loop body behind the network (app.c:341-371) is part of the push: moving average, maximum, threshold and
    # edisonFSM run as the last GPU stages (Stream(fsm=True)); what comes back is the state after every inference
    if net is not None:
        with_fsm = ctx.fnet_info()["n_out"] == len(KEYWORDS)
        st = FloatStream(ctx, geometry, q15=q15, chunk_frames=n, output_filter=True, alpha=alpha, threshold=threshold, fsm=with_fsm)
        names = st.keywords or (list(KEYWORDS) if with_fsm else [])
        name = lambda i: names[i] if i < len(names) else "class %d" % i
    elif geometry is None:
        st = Stream(ctx, hop=hop, chunk_frames=n, q15=q15, output_filter=True, alpha=alpha, threshold=threshold, fsm=True)
        with_fsm, name = True, lambda i: KEYWORDS[i]
    else:
        with_fsm = ctx.net_info()["n_out"] == len(KEYWORDS)
        st = GeomStream(ctx, geometry, chunk_frames=n, output_filter=True, alpha=alpha, threshold=threshold, fsm=with_fsm)
        name = (lambda i: KEYWORDS[i]) if with_fsm else (lambda i: "class %d" % i)
    res = st.push(data)
    st.close()
    if net is not None:
        shown = res["probs"]
    else:
        shown = res["softmax"] if res["softmax"] is not None else res["logits"]   # what the filter averaged
    events, before = _print_hops(out, n, shown, res["likely"], res["spotted"], res["fsm_states"] if with_fsm else None, name)
    if with_fsm:
        assert len(events) == res["fsm"]["commands"]
    return dict(result=res, commands=events, state=before if with_fsm else None)


def _print_hops(out, n, shown, likelies, spotteds, fsm_states, name):
    """One line per hop, the firmware's UART log (app.c:330-353); fsm_states None: no state machine. Returns (commands, last state)."""
    events = []
    before, loc, val = "RESET", -1, -1
    for i in range(n):
        likely, spotted = int(likelies[i]), int(spotteds[i])
        line = "pred: [ " + " ".join("%2.2f" % float(v) for v in shown[i]) + " ] likely: %s" % name(likely)
        if spotted >= 0:
            line += " spotted %s" % name(spotted)
        if fsm_states is not None:
            after = Fsm.STATES[int(fsm_states[i])]
            if after != before:
                line += "   [FSM %s -> %s]" % (before, after)
            if before == "HOT" and after == "LOC":
                loc = likely                                          # the location that was spotted (app.c:812-816)
            if before == "LOC" and after == "SET":
                val = likely                                          # ... and the value (app.c:836-840)
            if before == "SET":                                       # the step that executes the command (app.c:850-872)
                line += "   [%s %s]" % (KEYWORDS[loc], KEYWORDS[val])
                events.append((KEYWORDS[loc], KEYWORDS[val]))
            before = after
        print(line, file=out)
    return events, before


def run_bank(paths, ctx=None, out=None, alpha=None, threshold=0.5, geometry=None, net=None, q15=False):
    """Several wav files as the microphones of one bank: the shorter recordings are padded with silence to the longest, all advance in
    one push. Without net: a StreamBank at `geometry` on the int8 graph. With net (an .ednf path or its bytes): a FloatBank on the
    float32 X-CUBE-AI network, loaded on ctx (host flow at `geometry`, default audio/config.py's; q15: the firmware's flow), as run()
    with net. Per microphone a heading line ``mic <m>: <path>`` and then the lines run() prints for that file alone, for the hops of
    its own recording. Returns dict(result, mics=[dict(commands, state)])."""
    if net is None and (geometry is None or q15):
        raise ValueError("several recordings run as one bank: the int8 graph at a geometry (geometry=..., no q15), or a float network (net=...)")
    out = out or sys.stdout
    ctx = ctx or default_context()
    if net is not None:
        ctx.fnet_load(net)
        if geometry is None:
            from ..kws.geometry import KwsGeometry
            geometry = KwsGeometry.from_config(net_input_scale=cfg.net_input_scale)
    hop = int(geometry.frame_step)
    datas = [read_wav(p) for p in paths]
    hops = [-(-d.shape[0] // hop) for d in datas]
    n = max(hops)
    x = np.stack([np.pad(d, (0, n * hop - d.shape[0])) for d in datas])
    if net is not None:
        with_fsm = ctx.fnet_info()["n_out"] == len(KEYWORDS)
        bank = FloatBank(ctx, len(paths), geometry, q15=q15, chunk_frames=n, output_filter=True, alpha=0.5 if alpha is None else alpha,
                         threshold=threshold, fsm=with_fsm)
        names = bank.keywords or (list(KEYWORDS) if with_fsm else [])
        name = lambda i: names[i] if i < len(names) else "class %d" % i
    else:
        with_fsm = ctx.net_info()["n_out"] == len(KEYWORDS)
        bank = StreamBank(ctx, geometry, len(paths), chunk_frames=n, output_filter=True, alpha=0.9 if alpha is None else alpha,
                          threshold=threshold, fsm=with_fsm)
        name = (lambda i: KEYWORDS[i]) if with_fsm else (lambda i: "class %d" % i)
    res = bank.push(x)
    bank.close()
    if net is not None:
        shown = res["probs"]
    else:
        shown = res["softmax"] if res["softmax"] is not None else res["logits"]
    mics = []
    for m, p in enumerate(paths):
        print("mic %d: %s" % (m, p), file=out)
        events, before = _print_hops(out, hops[m], shown[:, m], res["likely"][:, m], res["spotted"][:, m],
                                     res["fsm_states"][:, m] if with_fsm else None, name)
        mics.append(dict(commands=events, state=before if with_fsm else None))
    return dict(result=res, mics=mics)


def main(argv):
    net = None
    if "--net" in argv:
        i = argv.index("--net")
        if i + 1 >= len(argv):
            print("--net needs an .ednf file")
            return 1
        net = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    if len(argv) < 3 or argv[1] not in ("host", "mcu") or (len(argv) > 3 and net is None):
        print("usage: kws live <host|mcu> <wav> [<wav> ...] [--net <file.ednf>]   (--net: the float32 X-CUBE-AI network instead of the int8 "
              "graph; several wavs with --net: the microphones of one bank; the microphone front end of the reference is not part of this port)")
        return 0 if len(argv) == 2 and argv[1] in ("host", "mcu") else 1
    run(argv[2:] if len(argv) > 3 else argv[2], q15=(argv[1] == "mcu"), net=net)
    return 0

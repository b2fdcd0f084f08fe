"""Scoring a labelled data set on the GPU: NNoM's evaluation API (prediction_create / prediction_run / prediction_matrix /
prediction_top_k / prediction_summary, nnom_utils.c:20-254) and the float model's predictWithConfMatrix (kws_keras.py:503-517) behind
``edison_eval_*`` (include/edison_hip.h). The counters live in device memory; an ``Evaluator`` adds chunks of
network outputs to them where they lie and ``result()`` brings back only the counts. ``Context.evaluate`` runs a whole flow this way.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import EVAL_ARGMAX, EVAL_KERAS, EVAL_NNOM, EdisonError

RULES = {"nnom": EVAL_NNOM, "keras": EVAL_KERAS, "argmax": EVAL_ARGMAX}
FLOWS = ("kws", "kws_geom", "kws_f32", "kws_float")


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _t_ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def label_vector(labels):
    """int32 labels from a vector or from a one-hot matrix (the reference's cached y_*.npy), taken with argmax(axis=1)"""
    y = np.asarray(labels)
    if y.ndim == 2:
        y = np.argmax(y, axis=1)
    if y.ndim != 1:
        raise ValueError("labels must be a vector or a one-hot matrix")
    return np.ascontiguousarray(y, dtype=np.int32)


class EvalResult:
    """confusion uint64 [n, n] (rows = actual label, columns = predicted), top_k uint64 [top_k] (top_k[r]: true label ranked r), count
    (labelled outputs), skipped (label out of range), correct (the trace); pred / prob / rank per utterance when they were asked for."""

    def __init__(self, confusion, top_k, count, skipped, correct, pred=None, prob=None, rank=None):
        self.confusion, self.top_k = confusion, top_k
        self.count, self.skipped, self.correct = int(count), int(skipped), int(correct)
        self.pred, self.prob, self.rank = pred, prob, rank

    @property
    def accuracy(self):
        return self.correct / self.count if self.count else float("nan")

    def top_k_accuracy(self, k=None):
        """Share of counted outputs whose true label ranks among the first k (default: all recorded ranks)"""
        k = len(self.top_k) if k is None else int(k)
        if not 0 <= k <= len(self.top_k):
            raise ValueError("k must be 0 .. %d, the evaluator's top_k" % len(self.top_k))
        return int(self.top_k[:k].sum()) / self.count if self.count else float("nan")

    def summary(self):
        """Text laid out like prediction_top_k + prediction_matrix (nnom_utils.c:178-224) with the same integer arithmetic:
        (top * 100) / count and ((top * 100 * 100) / count) % 100, "100%" when all are right, cell * 100 / row_total per row. A row
        whose total is 0 prints its cells and no percentage (the reference divides by zero there). Exact integers throughout: the
        reference's uint32 products wrap above 429 496 frames."""
        n = self.confusion.shape[0]
        lines = ["", "Prediction summary:", "Test frames: %d" % self.count]
        if n > 1:
            top = 0
            for i, v in enumerate(self.top_k):
                top += int(v)
                if top != self.count:
                    lines.append("Top %d Accuracy: %d.%02d%% " % (i + 1, (top * 100) // self.count, ((top * 100 * 100) // self.count) % 100))
                else:
                    lines.append("Top %d Accuracy: 100%% " % (i + 1))
            lines += ["", "Confusion matrix:", "predict" + "".join("%6d" % j for j in range(n)), "actual"]
            for i in range(n):
                row = [int(v) for v in self.confusion[i]]
                total = sum(row)
                lines.append(" %3d | " % i + "".join("%6d" % v for v in row) + "   |" + ("%4d%%" % (row[i] * 100 // total) if total else ""))
            lines.append("")
        return "\n".join(lines) + "\n"


class Evaluator:
    """edison_eval: device counters on `ctx`. rule: "nnom" (int8 outputs), "keras" or "argmax" (float32), or an _lib.EVAL_* value."""

    def __init__(self, ctx, rule, n_classes, top_k=2, max_blocks=0):
        self._ctx, self._L = ctx, ctx._L
        o = _lib.EvalOpts()
        self._L.edison_eval_default_opts(ctypes.byref(o))
        o.rule = RULES[rule] if isinstance(rule, str) else int(rule)
        o.n_classes, o.top_k, o.max_blocks = int(n_classes), int(top_k), int(max_blocks)
        h = ctypes.c_void_p()
        ctx._check(self._L.edison_eval_create(ctx._h, ctypes.byref(o), ctypes.byref(h)))
        self._h = h
        self.rule, self.n_classes, self.top_k = o.rule, o.n_classes, o.top_k
        self.is_float = o.rule != EVAL_NNOM

    def close(self):
        if getattr(self, "_h", None):
            self._L.edison_eval_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        self._ctx._check(self._L.edison_eval_reset(self._h))

    def add(self, outputs, labels, return_pred=False):
        """Host arrays: outputs [n, n_classes] (int8 for "nnom", float32 otherwise), labels a vector or one-hot. With return_pred the
        per-utterance dict(pred uint32, prob float32, rank int32) comes back."""
        x = np.ascontiguousarray(outputs, dtype=np.float32 if self.is_float else np.int8).reshape(-1, self.n_classes)
        y = label_vector(labels)
        if y.shape[0] != x.shape[0]:
            raise ValueError("%d outputs, %d labels" % (x.shape[0], y.shape[0]))
        n = x.shape[0]
        pred = np.zeros(n, np.uint32) if return_pred else None
        prob = np.zeros(n, np.float32) if return_pred else None
        rank = np.zeros(n, np.int32) if return_pred else None
        fn = self._L.edison_eval_add_f32 if self.is_float else self._L.edison_eval_add_i8
        self._ctx._check(fn(self._h, _np_ptr(x), _np_ptr(y), n, _np_ptr(pred), _np_ptr(prob), _np_ptr(rank)))
        return dict(pred=pred, prob=prob, rank=rank) if return_pred else None

    def add_t(self, outputs, labels, n=None, pred=None, prob=None, rank=None):
        """edison_eval_add_*_dev on torch device tensors (outputs [n, n_classes] int8 / float32 contiguous, labels int32 [n]; pred uint32
        -- or int32 -- , prob float32, rank int32 optional), enqueued on the context's stream: no copy, no host synchronisation."""
        n = int(labels.shape[0] if n is None else n)
        fn = self._L.edison_eval_add_f32_dev if self.is_float else self._L.edison_eval_add_i8_dev
        self._ctx._check(fn(self._h, _t_ptr(outputs), _t_ptr(labels), n, _t_ptr(pred), _t_ptr(prob), _t_ptr(rank)))

    def result(self):
        """Synchronise and fetch the counters (the evaluator goes on counting afterwards)"""
        t = _lib.EvalTotals()
        conf = np.zeros((self.n_classes, self.n_classes), np.uint64)
        top = np.zeros(self.top_k, np.uint64)
        self._ctx._check(self._L.edison_eval_result(self._h, ctypes.byref(t), _np_ptr(conf), _np_ptr(top)))
        return EvalResult(conf, top, t.count, t.skipped, t.correct)


def host_eval(rule, outputs, labels, top_k=2):
    """The same rules on the host alone, no GPU (edison_nnom_prediction_run / edison_eval_f32_host): an EvalResult with pred, prob, rank."""
    rule = RULES[rule] if isinstance(rule, str) else int(rule)
    x = np.ascontiguousarray(outputs, dtype=np.int8 if rule == EVAL_NNOM else np.float32)
    if x.ndim != 2:
        raise ValueError("outputs must be [n, n_out]")
    y = label_vector(labels)
    if y.shape[0] != x.shape[0]:
        raise ValueError("%d outputs, %d labels" % (x.shape[0], y.shape[0]))
    n, n_out = x.shape
    conf, top = np.zeros((n_out, n_out), np.uint64), np.zeros(max(int(top_k), 0), np.uint64)
    pred, prob, rank = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    t = _lib.EvalTotals()
    L = _lib.lib()
    tail = (_np_ptr(x), _np_ptr(y), n, n_out, int(top_k), _np_ptr(conf), _np_ptr(top), _np_ptr(pred), _np_ptr(prob), _np_ptr(rank), ctypes.byref(t))
    r = L.edison_nnom_prediction_run(*tail) if rule == EVAL_NNOM else L.edison_eval_f32_host(rule, *tail)
    if r != _lib.OK:
        raise EdisonError(r, "host evaluation: bad arguments")
    return EvalResult(conf, top, t.count, t.skipped, t.correct, pred, prob, rank)


def evaluate(ctx, audio, labels, flow="kws", chunk=16384, rule=None, top_k=2, return_pred=False, max_blocks=0, **flow_args):
    """Context.evaluate: score a labelled data set with one of the audio-to-class flows, chunk by chunk. Per chunk the flow's device
    form (kws_t, kws_geom_t, kws_f32_t, kws_float_t; their arguments in flow_args) writes its outputs to device buffers and add_t counts
    them behind it on the context's stream; nothing but the final counters comes back, unless return_pred asks for the per-utterance
    pred / prob / rank. audio: int16, a numpy array (uploaded chunk by chunk) or a torch device tensor (read in place); utterance u starts
    at u * utt_stride (flow_args; default: the row length of a 2-D audio, else the flow's own default). labels: one per utterance, a
    vector or one-hot; -1 (any value out of range) marks an unlabelled utterance. The last chunk may be short."""
    import torch
    if flow not in FLOWS:
        raise ValueError("flow must be one of %s" % (FLOWS,))
    y = label_vector(labels)
    n = int(y.shape[0])
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    args = dict(flow_args)
    stride = args.pop("utt_stride", None)
    on_device = isinstance(audio, torch.Tensor)
    if not on_device:
        audio = np.ascontiguousarray(audio, dtype=np.int16)
    if stride is None and audio.ndim == 2:
        stride = int(audio.shape[1])
    flat = audio.reshape(-1)
    dev = torch.device("cuda", ctx.device)

    # the flow: samples one utterance reads, the default stride, which output the rule reads, and the chunk's launch
    if flow in ("kws", "kws_geom", "kws_f32"):
        info = ctx.net_info()
        n_out, dtype, last = info["n_out"], torch.int8, ("softmax" if info["has_softmax"] else "logits")
        rule = EVAL_NNOM if rule is None else rule
    else:
        info = ctx.fnet_info()
        n_out, dtype, last = info["n_out"], torch.float32, "probs"
        rule = EVAL_KERAS if rule is None else rule
    if flow == "kws":
        used, stride = _lib.UTT_FRAMES * _lib.FRAME_LEN, 32000 if stride is None else int(stride)
        run = lambda a, m, o, lb: ctx.kws_t(a, m, stride, **{last: o}, **args)
    elif flow == "kws_f32":
        mfcc, hop = args.pop("mfcc"), int(args.pop("hop", 0))
        used = (info["in_h"] - 1) * (hop if hop else mfcc.frame_len // 2) + mfcc.frame_len
        stride = used if stride is None else int(stride)
        run = lambda a, m, o, lb: ctx.kws_f32_t(mfcc, a, m, stride, lb, hop=hop, **{last: o}, **args)
    else:
        g = args.pop("geometry", None)
        if g is None:
            if flow == "kws_geom":
                raise ValueError("flow kws_geom needs geometry=")
            from . import config as cfg
            from .kws.geometry import KwsGeometry
            g = KwsGeometry.from_config(net_input_scale=cfg.net_input_scale)
        used, stride = (g.frame_count - 1) * g.frame_step + g.frame_len, int(g.n_samples if stride is None else stride)
        if flow == "kws_geom":
            run = lambda a, m, o, lb: ctx.kws_geom_t(a, g, m, stride, **{last: o}, **args)
        else:
            run = lambda a, m, o, lb: ctx.kws_float_t(a, g, m, stride, **{last: o}, **args)
    if n and (n - 1) * stride + used > flat.shape[0]:
        raise ValueError("audio too short for %d utterances" % n)

    ev = Evaluator(ctx, rule, n_out, top_k=top_k, max_blocks=max_blocks)
    try:
        m_max = min(chunk, max(n, 1))
        outs = torch.zeros((m_max, n_out), dtype=dtype, device=dev)
        f32_label = torch.zeros(m_max, dtype=torch.int32, device=dev) if flow == "kws_f32" else None   # nnom_predict's label: required there
        y_d = torch.from_numpy(y).to(dev)
        pred = torch.zeros(n, dtype=torch.int32, device=dev) if return_pred else None
        prob = torch.zeros(n, dtype=torch.float32, device=dev) if return_pred else None
        rank = torch.zeros(n, dtype=torch.int32, device=dev) if return_pred else None
        a_d = None
        for u0 in range(0, n, chunk):
            m = min(chunk, n - u0)
            lo, hi = u0 * stride, (u0 + m - 1) * stride + used
            if on_device:
                a_d = flat[lo:hi]
            else:
                ctx.sync()                       # the previous chunk still reads the audio buffer this upload replaces
                a_d = torch.from_numpy(flat[lo:hi]).to(dev)
            torch.cuda.current_stream(dev).synchronize()   # torch's allocations and uploads, before the context's stream reads them
            run(a_d, m, outs, f32_label)
            ev.add_t(outs, y_d[u0:u0 + m], m, None if pred is None else pred[u0:u0 + m], None if prob is None else prob[u0:u0 + m],
                     None if rank is None else rank[u0:u0 + m])
        res = ev.result()
        if return_pred:
            res.pred, res.prob, res.rank = pred.cpu().numpy().view(np.uint32), prob.cpu().numpy(), rank.cpu().numpy()
        return res
    finally:
        ev.close()

"""Numpy restatement of the three evaluation rules, written from the reference's lines (not from csrc/nnom_eval_core.h):

  * ``nnom``   -- prediction_run, firmware/src/ai/nnom/src/core/nnom_utils.c:88-164, on int8 outputs;
  * ``keras``  -- predictWithConfMatrix, kws_keras.py:503-517 / kws_nnom.py:150-165: argmax of 1.0 * (y_pred > 0.5) into a confusion matrix;
  * ``argmax`` -- the first maximum of float32 outputs.

Every function takes outputs [n, n_out] and int32 labels [n] and returns a dict: confusion uint64 [n_out, n_out] (rows = actual), top_k
uint64 [top_k], count, skipped, correct, and the per-row pred uint32, prob float32, rank int32. A label outside 0 .. n_out - 1 is skipped:
it moves only `skipped`; its pred / prob are still given, its rank is -1. Plain loops over rows: the point is to be easy to hold against
the reference, not to be fast. The reference's own compiled prediction_run is driven by ``run_reference`` (ctypes, oracle/_ref).
"""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libnnom_ref.so")
NNOM, KERAS, ARGMAX = 0, 1, 2


def _rank(row, t):
    """nnom_utils.c:112-121: how many outputs come before the true one; an equal output counts only from a lower index"""
    rank = 0
    for j in range(len(row)):
        if j == t:
            continue
        if row[t] < row[j]:
            rank += 1
        elif row[t] == row[j] and j < t:
            rank += 1
    return rank


def _empty(n, n_out, top_k):
    return dict(confusion=np.zeros((n_out, n_out), np.uint64), top_k=np.zeros(top_k, np.uint64), count=0, skipped=0, correct=0,
                pred=np.zeros(n, np.uint32), prob=np.zeros(n, np.float32), rank=np.full(n, -1, np.int32))


def _finish(r):
    r["correct"] = int(np.trace(r["confusion"]))
    return r


def nnom(out, labels, top_k):
    out = np.asarray(out, np.int8)
    n, n_out = out.shape
    r = _empty(n, n_out, top_k)
    for i in range(n):
        row = [int(v) for v in out[i]]
        t = int(labels[i])
        ok = 0 <= t < n_out
        if n_out > 1:
            max_val, max_index, total = row[0], 0, 0          # :128-138: `sum` starts at 0 and the loop starts at j = 1
            for j in range(1, n_out):
                if row[j] > max_val:
                    max_val, max_index = row[j], j
                total = (total + row[j]) & 0xFFFFFFFF             # uint32 += int8: sign-extended, modulo 2^32
            r["pred"][i] = max_index
            # :140-143: (float)int / (float)uint32, one correctly rounded float32 division
            r["prob"][i] = np.float32(max_val) / np.float32(total) if total != 0 else np.float32(0)
            if ok:
                rank = _rank(row, t)
                r["rank"][i] = rank
                if rank < top_k:
                    r["top_k"][rank] += 1
                r["confusion"][t, max_index] += 1
        else:
            p = np.float32(row[0]) / np.float32(127.0)            # :152-156
            r["prob"][i] = p
            r["pred"][i] = 1 if p >= np.float32(0.5) else 0
        if ok:
            r["count"] += 1
        else:
            r["skipped"] += 1
    return _finish(r)


def floats(rule, probs, labels, top_k):
    probs = np.asarray(probs, np.float32)
    n, n_out = probs.shape
    r = _empty(n, n_out, top_k)
    for i in range(n):
        row = probs[i]
        t = int(labels[i])
        if rule == KERAS:
            pred = int(np.argmax(1.0 * (row > 0.5)))              # kws_keras.py:508
        else:
            pred, best = 0, row[0]
            for j in range(1, n_out):
                if row[j] > best:
                    pred, best = j, row[j]
        r["pred"][i] = pred
        r["prob"][i] = row[pred]
        if 0 <= t < n_out:
            rank = _rank(row, t)
            r["rank"][i] = rank
            if rank < top_k:
                r["top_k"][rank] += 1
            r["confusion"][t, pred] += 1
            r["count"] += 1
        else:
            r["skipped"] += 1
    return _finish(r)


def keras(probs, labels, top_k):
    return floats(KERAS, probs, labels, top_k)


def argmax(probs, labels, top_k):
    return floats(ARGMAX, probs, labels, top_k)


def confusion_matrix(y_true, y_pred, n_out):
    """sklearn.metrics.confusion_matrix(y_true, y_pred, labels=range(n_out)): cell [i, j] = samples of class i predicted as j"""
    m = np.zeros((n_out, n_out), np.uint64)
    np.add.at(m, (np.asarray(y_true, np.int64), np.asarray(y_pred, np.int64)), 1)
    return m


# ---------------------------------------------------------------------------------------------------------------- the reference itself
class _NnomPredict(ctypes.Structure):
    """nnom_predict_t, nnom/inc/nnom_utils.h:22-40"""
    _fields_ = [("confusion_mat", ctypes.POINTER(ctypes.c_uint16)), ("top_k", ctypes.POINTER(ctypes.c_uint32)), ("model", ctypes.c_void_p),
                ("buf_prediction", ctypes.POINTER(ctypes.c_int8)), ("label_num", ctypes.c_uint32), ("top_k_size", ctypes.c_uint32),
                ("predict_count", ctypes.c_uint32), ("t_run_total", ctypes.c_uint32), ("t_predict_start", ctypes.c_uint32),
                ("t_predict_total", ctypes.c_uint32)]


def have_reference():
    return os.path.exists(REF_SO)


def run_reference(out, labels, top_k):
    """The reference's compiled prediction_run on a hand-built nnom_predict_t: model = NULL (model_run(NULL) returns an error that
    prediction_run ignores, after printing "Error: NULL object." to stdout), buf_prediction pointed at each row in turn. Labels must be
    in range (the reference indexes with them). Returns the dict of ``nnom`` (cells are the reference's uint16, widened)."""
    out = np.ascontiguousarray(out, np.int8)
    n, n_out = out.shape
    L = ctypes.CDLL(REF_SO)
    L.prediction_run.restype = ctypes.c_int
    L.prediction_run.argtypes = [ctypes.POINTER(_NnomPredict), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)]
    mat = np.zeros(n_out * n_out, np.uint16)
    top = np.zeros(max(top_k, 1), np.uint32)
    pre = _NnomPredict()
    pre.confusion_mat = mat.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
    pre.top_k = top.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    pre.model = None
    pre.label_num, pre.top_k_size, pre.predict_count = n_out, top_k, 0
    r = _empty(n, n_out, top_k)
    label, prob = ctypes.c_uint32(), ctypes.c_float()
    # the reference prints one line per call: keep it off the test log (file descriptor 1, the C library's stdout)
    import sys
    sys.stdout.flush()
    saved = os.dup(1)
    devnull = os.open(os.devnull, os.O_WRONLY)
    os.dup2(devnull, 1)
    try:
        for i in range(n):
            pre.buf_prediction = out[i].ctypes.data_as(ctypes.POINTER(ctypes.c_int8))
            status = L.prediction_run(ctypes.byref(pre), int(labels[i]), ctypes.byref(label), ctypes.byref(prob))
            assert status == 0, status
            r["pred"][i], r["prob"][i] = label.value, prob.value
        libc = ctypes.CDLL(None)
        libc.fflush(None)
    finally:
        os.dup2(saved, 1)
        os.close(saved)
        os.close(devnull)
    r["confusion"] = mat.reshape(n_out, n_out).astype(np.uint64)
    r["top_k"] = top[:top_k].astype(np.uint64)
    r["count"] = int(pre.predict_count)
    r.pop("rank")                                   # the reference does not return the rank; top_k carries it
    return _finish(r)

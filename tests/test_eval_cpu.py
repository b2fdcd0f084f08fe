"""CPU tests of the evaluation rules (csrc/nnom_eval_core.h through edison_nnom_prediction_run / edison_eval_f32_host in legacy.c) and
of EvalResult.summary: no GPU.

  * the pin: the reference's own compiled prediction_run (oracle/_ref/libnnom_ref.so through tests/nnom_eval_ref.run_reference) where it
    is built, and always its recording tests/golden/eval_golden.npz (tests/golden/gen_fixtures_eval.py) -- about 1 500 rows for 2, 3, 10
    and 64 outputs: random rows, all-equal rows, the maximum at element 0, a sum of exactly 0, wrapping sums, labels at every tie
    position. The numpy restatement (tests/nnom_eval_ref.py), the host function and the reference agree exactly: counts equal, prob bit
    for bit;
  * a single output, the Keras rule against confusion_matrix-style numpy, the first-maximum rule, labels out of range, top_k of 0, 1,
    n_out and n_out + 3, refusals, and summary() against a literal string.
"""
import ctypes
import os

import numpy as np
import pytest

import nnom_eval_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_golden.npz")
N_OUTS = (2, 3, 10, 64)
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def ev(built_lib):
    from edison_amd import evaluate
    return evaluate


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what, per_row=True):
    """got: an EvalResult (or a dict of the restatement), want: a dict of the restatement / the reference"""
    g = got if isinstance(got, dict) else dict(confusion=got.confusion, top_k=got.top_k, count=got.count, skipped=got.skipped, correct=got.correct,
                                               pred=got.pred, prob=got.prob, rank=got.rank)
    for k in ("count", "skipped", "correct"):
        if k in want:
            assert int(g[k]) == int(want[k]), (what, k, g[k], want[k])
    assert np.array_equal(g["confusion"], want["confusion"]), what + ": confusion matrix"
    assert np.array_equal(g["top_k"], want["top_k"]), what + ": top-k histogram"
    if per_row:
        assert np.array_equal(g["pred"], want["pred"]), what + ": pred"
        assert np.array_equal(_bits(g["prob"]), _bits(want["prob"])), what + ": prob, bit for bit"
        if "rank" in want:
            assert np.array_equal(g["rank"], want["rank"]), what + ": rank"


@pytest.mark.parametrize("n_out", N_OUTS)
def test_prediction_run_pinned_on_the_reference(ev, golden, n_out):
    """restatement == edison_nnom_prediction_run == the recording of the reference's prediction_run, and the live reference where built"""
    out, labels = golden["out_%d" % n_out], golden["labels_%d" % n_out]
    assert 1400 <= out.shape[0] <= 1600 and out.shape[1] == n_out and set(np.unique(labels)) == set(range(n_out))
    recorded = dict(confusion=golden["confusion_%d" % n_out], top_k=golden["top_k_%d" % n_out], count=int(golden["count_%d" % n_out]), skipped=0,
                    correct=int(np.trace(golden["confusion_%d" % n_out])),
                    pred=golden["pred_%d" % n_out], prob=golden["prob_%d" % n_out])
    assert int(recorded["confusion"].max()) < 65536 and recorded["count"] == out.shape[0]
    want = ref.nnom(out, labels, n_out)
    same(want, recorded, "restatement vs the recorded reference, %d outputs" % n_out)
    got = ev.host_eval("nnom", out, labels, top_k=n_out)
    same(got, want, "edison_nnom_prediction_run vs the restatement, %d outputs" % n_out)
    same(got, recorded, "edison_nnom_prediction_run vs the recorded reference, %d outputs" % n_out)
    if ref.have_reference():
        live = ref.run_reference(out, labels, n_out)
        same(recorded, live, "the recording vs the live reference, %d outputs" % n_out)
        same(got, live, "edison_nnom_prediction_run vs the live reference, %d outputs" % n_out)
    # the cases the rows are there for do occur
    sums = (out[:, 1:].astype(np.int64).sum(axis=1)) & 0xFFFFFFFF
    assert (sums == 0).sum() >= 50 and (sums > 2 ** 31).sum() >= 100
    assert (out.argmax(axis=1) == 0).sum() >= 100 and (out == out[:, :1]).all(axis=1).sum() >= 5 * n_out


def test_the_quotients_read_off_the_reference(ev):
    """The three rows of the issue: element 0 is not in the sum; a wrapping sum gives a tiny quotient"""
    rows = np.array([[-7, 3, 65, 115, -120, -92, 82, 114, -65, -49], [5, 5, 0, 0, 0, 0, 0, 0, 0, 5]], np.int8)
    r = ev.host_eval("nnom", rows, [3, 0], top_k=1)
    assert r.prob[0] == np.float32(115) / np.float32(53) and abs(float(r.prob[0]) - 2.1698112) < 1e-6 and r.prob[1] == np.float32(0.5)
    assert list(r.pred) == [3, 0] and list(r.rank) == [0, 0]
    wrap = np.full((1, 10), -128, np.int8)                       # sum = 2^32 - 9 * 128
    r = ev.host_eval("nnom", wrap, [9], top_k=10)
    assert r.prob[0] == np.float32(-128) / np.float32(2 ** 32 - 1152) and r.rank[0] == 9 and r.top_k[9] == 1


def test_one_output(ev):
    out = np.arange(-128, 128, dtype=np.int64).astype(np.int8).reshape(-1, 1)
    labels = np.array([0, 1, -1, 0] * 64, np.int32)
    want = ref.nnom(out, labels, 3)
    got = ev.host_eval("nnom", out, labels, top_k=3)
    same(got, want, "one output")
    assert got.count == 128 and got.skipped == 128 and got.correct == 0 and not got.confusion.any() and not got.top_k.any()
    assert (got.rank == -1).all() and got.pred[128 + 63] == 0 and got.pred[128 + 64] == 1    # 63 / 127 < 0.5 <= 64 / 127


def _float_rows(n_out, rng):
    rows = [rng.random(n_out).astype(np.float32) for _ in range(300)]
    rows += [rng.dirichlet(np.ones(n_out) * 0.3).astype(np.float32) for _ in range(300)]    # softmax-like: often one class above 0.5
    special = [np.full(n_out, 0.5), np.full(n_out, 0.1), np.full(n_out, 0.9), np.zeros(n_out)]
    if n_out >= 3:
        special += [np.r_[0.2, 0.7, 0.6, np.zeros(n_out - 3)], np.r_[0.5, 0.5, np.float32(0.5) + np.float32(2.0 ** -24), np.zeros(n_out - 3)],
                    np.r_[np.nan, 0.3, 0.8, np.zeros(n_out - 3)], np.r_[0.1, np.nan, np.nan, np.zeros(n_out - 3)]]
    rows += [np.asarray(s, np.float32) for s in special for _ in range(n_out)]
    out = np.stack(rows)
    labels = (np.arange(out.shape[0]) % n_out).astype(np.int32)
    return out, labels


@pytest.mark.parametrize("n_out", [1, 2, 3, 10, 64])
def test_keras_rule_against_confusion_matrix(ev, n_out):
    """p == 0.5 exactly is not above 0.5; no class above 0.5 gives class 0; of two classes above 0.5 the first wins"""
    out, labels = _float_rows(n_out, np.random.default_rng(n_out))
    got = ev.host_eval("keras", out, labels, top_k=n_out)
    y_pred = np.argmax(1.0 * (out > 0.5), axis=1)                                    # kws_keras.py:508
    assert np.array_equal(got.pred, y_pred)
    assert np.array_equal(got.confusion, ref.confusion_matrix(labels, y_pred, n_out))
    assert np.array_equal(_bits(got.prob), _bits(out[np.arange(out.shape[0]), y_pred]))
    same(got, ref.keras(out, labels, n_out), "keras rule, %d outputs" % n_out)
    assert got.count == out.shape[0] and got.correct == int((y_pred == labels).sum()) and int(got.top_k.sum()) == got.count
    if n_out >= 3:
        k = 600 + 4 * n_out                                                          # the rows [0.2, 0.7, 0.6, 0 ...], then the 0.5 rows
        assert got.pred[k] == 1 and got.pred[k + n_out] == 2 and got.pred[600] == 0 and got.pred[600 + n_out] == 0


@pytest.mark.parametrize("n_out", [1, 2, 3, 10, 64])
def test_first_maximum_rule(ev, n_out):
    out, labels = _float_rows(n_out, np.random.default_rng(100 + n_out))
    got = ev.host_eval("argmax", out, labels, top_k=n_out + 3)
    same(got, ref.argmax(out, labels, n_out + 3), "first maximum, %d outputs" % n_out)
    clean = ~np.isnan(out).any(axis=1)
    assert np.array_equal(got.pred[clean], out[clean].argmax(axis=1))
    assert not got.top_k[n_out:].any()


@pytest.mark.parametrize("rule", ["nnom", "keras", "argmax"])
def test_labels_out_of_range_are_skipped(ev, rule):
    rng = np.random.default_rng(5)
    n_out = 10
    out = rng.integers(-128, 128, (60, n_out)).astype(np.int8) if rule == "nnom" else rng.random((60, n_out)).astype(np.float32)
    labels = rng.integers(0, n_out, 60).astype(np.int32)
    labels[::4], labels[1::4], labels[2::8] = -1, n_out, INT32_MAX
    labels[58], labels[59] = -(2 ** 31), 256
    want = (ref.nnom if rule == "nnom" else ref.keras if rule == "keras" else ref.argmax)(out, labels, 2)
    got = ev.host_eval(rule, out, labels, top_k=2)
    same(got, want, rule + " with labels out of range")
    bad = (labels < 0) | (labels >= n_out)
    assert got.skipped == int(bad.sum()) > 30 and got.count == 60 - got.skipped and int(got.confusion.sum()) == got.count
    assert (got.rank[bad] == -1).all() and (got.rank[~bad] >= 0).all()
    everything = (ref.nnom if rule == "nnom" else ref.keras if rule == "keras" else ref.argmax)(out, np.zeros(60, np.int32), 2)
    assert np.array_equal(got.pred, everything["pred"]) and np.array_equal(_bits(got.prob), _bits(everything["prob"]))   # still written


@pytest.mark.parametrize("n_out", [2, 10])
def test_top_k_sizes(ev, golden, n_out):
    out, labels = golden["out_%d" % n_out][:400], golden["labels_%d" % n_out][:400]
    full = ref.nnom(out, labels, n_out)
    for k in (0, 1, n_out, n_out + 3):
        got = ev.host_eval("nnom", out, labels, top_k=k)
        same(got, ref.nnom(out, labels, k), "top_k = %d" % k)
        assert got.top_k.shape == (k,) and np.array_equal(got.top_k[:n_out], full["top_k"][:k]) and not got.top_k[n_out:].any()
    assert int(full["top_k"].sum()) == 400


def test_one_hot_labels_and_accumulation(ev, built_lib):
    """labels may be one-hot; the host functions ADD to what the caller hands them"""
    from edison_amd import _lib
    out = np.random.default_rng(9).integers(-128, 128, (50, 3)).astype(np.int8)
    labels = (np.arange(50) % 3).astype(np.int32)
    a = ev.host_eval("nnom", out, np.eye(3)[labels], top_k=2)
    same(a, ref.nnom(out, labels, 2), "one-hot labels")
    conf, top, t = np.zeros((3, 3), np.uint64), np.zeros(2, np.uint64), _lib.EvalTotals()
    for part in (slice(0, 20), slice(20, 50)):
        o, l = np.ascontiguousarray(out[part]), np.ascontiguousarray(labels[part])
        assert built_lib.edison_nnom_prediction_run(o.ctypes.data, l.ctypes.data, o.shape[0], 3, 2, conf.ctypes.data, top.ctypes.data, None, None, None,
                                                    ctypes.byref(t)) == 0
    assert np.array_equal(conf, a.confusion) and np.array_equal(top, a.top_k) and (t.count, t.skipped, t.correct) == (50, 0, a.correct)
    assert a.accuracy == a.correct / 50 and a.top_k_accuracy(1) == int(a.top_k[0]) / 50 and a.top_k_accuracy() == int(a.top_k.sum()) / 50


def test_host_refusals(built_lib):
    from edison_amd import _lib
    L = built_lib
    one, lab, f = np.zeros(300, np.int8), np.zeros(1, np.int32), np.zeros(300, np.float32)
    run = lambda n, n_out, k, o=one, l=lab: L.edison_nnom_prediction_run(None if o is None else o.ctypes.data, None if l is None else l.ctypes.data, n,
                                                                         n_out, k, None, None, None, None, None, None)
    assert run(1, 10, 2) == 0 and run(0, 10, 2, None, None) == 0 and run(1, 256, 0) == 0
    for bad in (run(1, 0, 2), run(1, 257, 2), run(1, 10, -1), run(-1, 10, 2), run(1, 10, 2, None), run(1, 10, 2, one, None)):
        assert bad == _lib.E_ARGUMENT
    fl = lambda rule, n_out=10: L.edison_eval_f32_host(rule, f.ctypes.data, lab.ctypes.data, 1, n_out, 2, None, None, None, None, None, None)
    assert fl(_lib.EVAL_KERAS) == 0 and fl(_lib.EVAL_ARGMAX) == 0
    assert fl(_lib.EVAL_NNOM) == _lib.E_ARGUMENT and fl(7) == _lib.E_ARGUMENT and fl(_lib.EVAL_KERAS, 0) == _lib.E_ARGUMENT


SUMMARY = "".join(line + "\n" for line in (
    "",
    "Prediction summary:",
    "Test frames: 7",
    "Top 1 Accuracy: 57.14% ",          # the reference's format ends in "% \n"
    "Top 2 Accuracy: 85.71% ",
    "Top 3 Accuracy: 100% ",
    "",
    "Confusion matrix:",
    "predict     0     1     2",
    "actual",
    "   0 |      3     1     0   |  75%",
    "   1 |      0     0     0   |",
    "   2 |      1     1     1   |  33%",
    "",
))


def test_summary_against_a_literal(ev):
    """prediction_top_k + prediction_matrix (nnom_utils.c:178-224): integer percentages, "100%" when all are right, a row without frames
    prints no percentage"""
    conf = np.array([[3, 1, 0], [0, 0, 0], [1, 1, 1]], np.uint64)
    r = ev.EvalResult(conf, np.array([4, 2, 1], np.uint64), 7, 2, 4)
    assert r.summary() == SUMMARY
    assert ev.EvalResult(np.zeros((1, 1), np.uint64), np.zeros(0, np.uint64), 5, 0, 0).summary() == "\nPrediction summary:\nTest frames: 5\n"
    exact = ev.EvalResult(np.array([[655, 0], [0, 345]], np.uint64), np.array([1000], np.uint64), 1000, 0, 1000)
    assert "Top 1 Accuracy: 100% \n" in exact.summary() and "   | 100%\n" in exact.summary()
    assert "Top 1 Accuracy: 0.09% \n" in ev.EvalResult(np.array([[1, 0], [1099, 0]], np.uint64), np.array([1], np.uint64), 1100, 0, 1).summary()


def test_wired_into_the_build_and_the_binding(built_lib):
    """The header, the binding and the build list the new pieces; the core header holds each rule once and leaves nnom_predict's alone"""
    from edison_amd import _lib, build, main
    for name in ("edison_eval.hip", "eval_kernels.hip"):
        assert name in build.HIP_SOURCES and os.path.exists(os.path.join(build.CSRC, name))
    assert "nnom_eval_core.h" in build.HEADERS
    want = {"edison_eval_default_opts", "edison_eval_create", "edison_eval_destroy", "edison_eval_reset", "edison_eval_add_i8_dev", "edison_eval_add_f32_dev",
            "edison_eval_add_i8", "edison_eval_add_f32", "edison_eval_result", "edison_nnom_prediction_run", "edison_eval_f32_host"}
    assert want <= set(_lib.SIGNATURES) and all(hasattr(built_lib, n) for n in want)
    core = open(os.path.join(build.CSRC, "nnom_eval_core.h")).read()
    assert "ed_nnom_predict_one(" not in core.split("*/", 1)[1] and "nnom_predict_core.h" not in core.split("*/", 1)[1]
    for src in ("legacy.c", "eval_kernels.hip"):
        assert '#include "nnom_eval_core.h"' in open(os.path.join(build.CSRC, src)).read()
    assert "atomicAdd(float" not in open(os.path.join(build.CSRC, "eval_kernels.hip")).read()
    assert main.COMMANDS["kws"]["eval"][0] == "edison_amd.kws.kws_eval"
    assert main.main(["main.py", "kws", "eval"]) == 1 and main.main(["main.py", "kws", "eval", "a.npy", "b.npy", "--graph", "x", "--net", "y"]) == 1

#!/usr/bin/env python
"""Writes tests/golden/eval_golden.npz: labelled int8 output rows and what the REFERENCE's own compiled prediction_run
(nnom_utils.c:88-164, oracle/_ref/libnnom_ref.so, driven by tests/nnom_eval_ref.run_reference) made of them. Inputs and recorded
results only. Needs oracle/_ref (built by oracle/Makefile where the reference sources are present):

    python tests/golden/gen_fixtures_eval.py

Per n_out in N_OUTS: out_<n> int8 [rows, n], labels_<n> int32 [rows] (all in range: the reference indexes with them), and the
reference's pred_<n> uint32, prob_<n> float32, confusion_<n> uint64 [n, n] (widened from its uint16 cells, all far below 65 536),
top_k_<n> uint64 [n] (top_k_size = n) and count_<n>.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import nnom_eval_ref as ref  # noqa: E402

N_OUTS = (2, 3, 10, 64)
OUT = os.path.join(HERE, "eval_golden.npz")


def rows_for(n_out, rng):
    """About 1 500 rows: random ones, then the cases a restatement gets wrong first. Returns (out int8 [rows, n_out], labels int32)."""
    out, lab = [], []

    def add(row, t):
        out.append(np.asarray(row, np.int64).astype(np.int8))
        lab.append(int(t))

    for _ in range(960 - 5 * n_out):                               # random rows, random labels (about 1 500 rows in all)
        add(rng.integers(-128, 128, n_out), rng.integers(0, n_out))
    for _ in range(240):                                           # few distinct values: ties at every position of the label
        row = rng.integers(-1, 2, n_out) * int(rng.integers(1, 128))
        add(row, len(out) % n_out)
    for v in (-128, -1, 0, 1, 127):                                # all equal (all -128 / -1: the uint32 sum wraps), every label
        for t in range(n_out):
            add(np.full(n_out, v), t)
    for _ in range(100):                                           # the maximum is element 0, which the sum leaves out
        row = rng.integers(-128, 100, n_out)
        row[0] = 127 if len(out) % 2 else int(row.max())           # a strict maximum, or tied with a later one
        add(row, rng.integers(0, n_out))
    for _ in range(100):                                           # sum over elements 1 .. n_out - 1 is exactly 0
        row = np.zeros(n_out, np.int64)
        row[0] = rng.integers(-128, 128)
        if n_out >= 3:
            a, b = rng.choice(np.arange(1, n_out), 2, replace=False)
            v = int(rng.integers(1, 128))
            row[a], row[b] = v, -v
        add(row, rng.integers(0, n_out))
    for _ in range(100):                                           # negative sums: a uint32 near 2^32 under the float conversion
        add(rng.integers(-128, 0, n_out), rng.integers(0, n_out))
    if n_out == 10:                                                # three rows whose quotient was read off the reference by hand
        add([-7, 3, 65, 115, -120, -92, 82, 114, -65, -49], 3)      # 2.1698112
        add([5, 5, 0, 0, 0, 0, 0, 0, 0, 5], 0)                      # 0.5: element 0 is not in the sum
        add([5, 5, 0, 0, 0, 0, 0, 0, 0, 5], 9)
    return np.stack(out), np.asarray(lab, np.int32)


def main():
    if not ref.have_reference():
        sys.exit("oracle/_ref/libnnom_ref.so is missing: build it with `make -C oracle ref` where the reference sources are present")
    rng = np.random.default_rng(20261019)
    data = {}
    for n in N_OUTS:
        out, labels = rows_for(n, rng)
        r = ref.run_reference(out, labels, n)
        assert r["count"] == out.shape[0] and int(r["confusion"].max()) < 65536
        data.update({"out_%d" % n: out, "labels_%d" % n: labels, "pred_%d" % n: r["pred"], "prob_%d" % n: r["prob"],
                     "confusion_%d" % n: r["confusion"], "top_k_%d" % n: r["top_k"], "count_%d" % n: np.int64(r["count"])})
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

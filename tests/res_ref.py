"""tests/res_ref.py -- TEST INFRASTRUCTURE: numpy restatement of NNoM 0.3.0's merge layers (CMSIS-NN on, rounding build: neither
ARM_NN_TRUNCATE nor NNOM_TRUNCATE is defined) and of the graph wiring of model.merge / model.mergex, written from the
reference's sources and independent of the product's kernels and planners. The single-input layers are run by the
restatements that exist (tests/dscnn_ref.py, oracle/net_ref.py), one layer at a time, each as a one-record blob over the
tensor its source list names. Pinned by tests/golden/res_golden.npz (gen_fixtures_res.py).

  Add   shift 0: arm_add_q7, sat8(a + b); otherwise local_add_q7 (nnom_local.c:1109-1126): sat8((a + b + (1 << (s - 1))) >> s)
        a third and later input is combined with the OUTPUT so far: out = add(in_k, out) (nnom_matrix.c:123-137)
  Sub   shift 0: arm_sub_q7, sat8(a - b); otherwise local_sub_q7 (:1128-1145): sat8((a - b + (1 << (s - 1))) >> s); two inputs
  Mult  shift 0: arm_mult_q7, sat8((a * b) >> 7); otherwise local_mult_q7 (:1090-1107): sat8((a * b + (1 << (s - 1))) >> s); two inputs
  Concat over the channel axis of inputs of ONE shape: per pixel, the inputs' channels side by side (nnom_concat.c:197-214)
  a ReLU tail activation (model.active on the merge layer) clamps the result at 0 afterwards (nnom.c:986-989)

`wrong` names one deliberate mis-reading, for the tests that show the fixture tells them apart:
  truncate      the local_*_q7 routines without their rounding term (the NNOM_TRUNCATE build)
  mult_no_q7    Mult at shift 0 without arm_mult_q7's >> 7
  add_wide      a three-input Add summed in one go and saturated once
  sub_swapped   b - a
  concat_planar the inputs one whole tensor after the other instead of interleaved per pixel
"""
import struct

import numpy as np

import dscnn_ref
from oracle import net_ref

T_SOFTMAX = 4
T_ADD, T_SUB, T_MULT, T_CONCAT = 7, 8, 9, 10


def _sat8(v):
    return np.clip(v, -128, 127)


def merge2(kind, shift, a, b, wrong=None):
    a = a.astype(np.int32)
    b = b.astype(np.int32)
    if kind == T_SUB and wrong == "sub_swapped":
        a, b = b, a
    r = a + b if kind == T_ADD else a - b if kind == T_SUB else a * b
    if shift == 0:
        if kind == T_MULT and wrong != "mult_no_q7":
            r = r >> 7
    else:
        r = (r + (0 if wrong == "truncate" else 1 << (shift - 1))) >> shift
    return _sat8(r)


def sources(blob):
    """Per record the records it reads (-1: the network input): the blob's source table (header word 6), or the predecessor."""
    head = struct.unpack_from("<8i", blob, 8)
    n, off = head[3], head[6]
    if off == 0:
        return [[i - 1] for i in range(n)]
    at = 40 + 48 * n + off
    out = []
    for _ in range(n):
        cnt = struct.unpack_from("<i", blob, at)[0]
        out.append(list(struct.unpack_from("<%di" % cnt, blob, at + 4)))
        at += 4 * (cnt + 1)
    return out


def _one(recs, payload, shape, x, wrong):
    """Records `recs` (a chain) as a graph of their own over x."""
    sub = (b"EDNNOM1\0" + struct.pack("<8i", shape[0], shape[1], shape[2], len(recs), payload.size, 1, 0, 0) +
           b"".join(struct.pack("<12i", *r) for r in recs) + payload.tobytes())
    return dscnn_ref.run(sub, x, wrong if wrong in ("floor_div", "count_area", "no_round", "chw_weights", "cmsis_always", "local_always") else None)["acts"]


def _out_shape(v, shape):
    h, w, c = shape
    if v[0] in (net_ref.T_CONV, net_ref.T_POOL, dscnn_ref.T_DWCONV, dscnn_ref.T_AVGPOOL):
        same = (v[8] >> 1) & 1
        od = lambda n, k, s: -(-n // s) if same else -(-(n - k + 1) // s)   # noqa: E731
        return od(h, v[2], v[4]), od(w, v[3], v[5]), (v[1] if v[0] == net_ref.T_CONV else c)
    if v[0] == net_ref.T_DENSE:
        return 1, 1, v[1]
    return shape


def run(blob, x, wrong=None, corrupt=None):
    """As oracle.net_ref.run: dict(acts=[per-record (n, out_n) int8], logits, softmax (or None), argmax). corrupt = (record, f): that
    record's result is replaced by f(result) before anything reads it -- for the tests that show a record reaches the output."""
    in_shape, recs, payload = net_ref.parse_blob(blob)
    src = sources(blob)
    x = np.ascontiguousarray(x, dtype=np.int8).reshape(-1, in_shape[0] * in_shape[1] * in_shape[2])
    n = x.shape[0]
    acts, shapes = [], []
    tensor = lambda r: x if r < 0 else acts[r]            # noqa: E731
    shape = lambda r: tuple(in_shape) if r < 0 else shapes[r]  # noqa: E731
    has_softmax = False
    for i, v in enumerate(recs):
        s = src[i]
        assert all(-1 <= r < i for r in s), "record %d reads forward" % i
        if v[0] in (T_ADD, T_SUB, T_MULT):
            assert len(s) >= 2 and (v[0] == T_ADD or len(s) == 2) and all(shape(r) == shape(s[0]) for r in s)
            ins = [tensor(r) for r in s]
            if v[0] == T_ADD and wrong == "add_wide":
                out = _sat8((sum(t.astype(np.int32) for t in ins) + ((1 << v[7]) >> 1)) >> v[7])
            else:
                out = merge2(v[0], v[7], ins[0], ins[1], wrong)
                for t in ins[2:]:
                    out = merge2(v[0], v[7], t, out, wrong)
            shapes.append(shape(s[0]))
        elif v[0] == T_CONCAT:
            assert len(s) >= 2 and all(shape(r) == shape(s[0]) for r in s)
            h, w, c = shape(s[0])
            ins = [tensor(r).reshape(n, h * w, c) for r in s]
            out = np.concatenate(ins, axis=1 if wrong == "concat_planar" else 2).reshape(n, -1).astype(np.int32)
            shapes.append((h, w, c * len(s)))
        elif v[0] == T_SOFTMAX:
            # net_ref restates Softmax behind the layer that feeds it: rerun that layer with it
            assert len(s) == 1 and s[0] >= 0 and len(src[s[0]]) == 1 and i == len(recs) - 1
            p = src[s[0]][0]
            out = _one([recs[s[0]], v], payload, shape(p), tensor(p), wrong)[1].astype(np.int32)
            shapes.append(shape(s[0]))
            has_softmax = True
        else:
            assert len(s) == 1
            out = _one([v], payload, shape(s[0]), tensor(s[0]), wrong)[0].astype(np.int32)
            shapes.append(_out_shape(v, shape(s[0])))
        if v[0] in (T_ADD, T_SUB, T_MULT, T_CONCAT) and v[8] & 1:
            out = np.maximum(out, 0)
        if corrupt is not None and corrupt[0] == i:
            out = np.asarray(corrupt[1](out.reshape(n, -1)))
        acts.append(out.reshape(n, -1).astype(np.int8))
    last = acts[-1]
    logits = acts[src[-1][0]] if has_softmax else last
    return dict(acts=acts, logits=logits, softmax=last if has_softmax else None, argmax=np.argmax(last, axis=1).astype(np.int32))

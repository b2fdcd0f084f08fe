#!/usr/bin/env python3
"""Random sequential int8 graphs through the general network kernel against oracle/net_ref.py (which is pinned to
the reference's NNoM on six graphs): shapes, kernels, strides, paddings and channel counts the fixtures do not hold.
Graphs the planner refuses (reference quirks, LDS budget) are counted and skipped.   usage (box): tools/fuzz_net.py [n_graphs [seed [own | branching]]]
With a third argument every graph that has a matrix-core plan is ALSO run on its own kernel (edison_net_specialize: ~1 s of
compilation per graph) and compared again. 67 inputs per graph: ragged against every per-wave batch the planner picks.
With the word `branching` behind the seed the graphs come from random_branching_graph instead -- DW_Conv2D, AvgPool, skip connections
closed by Add / Sub / Mult, Concat of agreeing branches, even and odd channel counts -- and are compared with tests/res_ref.py.
random_graph draws what it always drew: its stream does not depend on the new generator."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (loads torch's HIP runtime first)
from edison_amd import _lib, nnom_import  # noqa: E402
from edison_amd.context import Context  # noqa: E402
from oracle import net_ref  # noqa: E402

T_CONV, T_POOL, T_DENSE, T_SOFTMAX = 1, 2, 3, 4
T_DWCONV, T_AVGPOOL, T_ADD, T_SUB, T_MULT, T_CONCAT = 5, 6, 7, 8, 9, 10


def out_dim(n, k, s, same):
    return -(-n // s) if same else -(-(n - k + 1) // s)


def random_graph(rng):
    h, w, c = int(rng.integers(3, 25)), int(rng.integers(3, 25)), int(rng.choice([1, 1, 2, 3, 4, 8]))
    shape, layers = (h, w, c), []
    for _ in range(int(rng.integers(1, 5))):
        kind = rng.choice(["conv", "conv", "pool"])
        kh, kw = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        sh, sw = int(rng.integers(1, 3)), int(rng.integers(1, 3))
        same = int(rng.integers(0, 2))
        oh, ow = out_dim(h, kh, sh, same), out_dim(w, kw, sw, same)
        if oh < 1 or ow < 1:
            continue
        if kind == "conv":
            oc = int(rng.choice([1, 2, 3, 4, 5, 8, 12, 16]))
            layers.append(dict(type=T_CONV, out_ch=oc, kh=kh, kw=kw, sh=sh, sw=sw, w=rng.integers(-100, 101, oc * kh * kw * c).astype(np.int8),
                               b=rng.integers(-100, 101, oc).astype(np.int8), out_rshift=int(rng.integers(5, 11)),
                               bias_lshift=int(rng.integers(0, 7)), relu=int(rng.integers(0, 2)), same=same))
            h, w, c = oh, ow, oc
        else:
            layers.append(dict(type=T_POOL, kh=kh, kw=kw, sh=sh, sw=sw, same=same))
            h, w = oh, ow
    for _ in range(int(rng.integers(0, 3))):
        no = int(rng.integers(1, 40))
        layers.append(dict(type=T_DENSE, out=no, w=rng.integers(-100, 101, no * h * w * c).astype(np.int8), b=rng.integers(-100, 101, no).astype(np.int8),
                           out_rshift=int(rng.integers(5, 12)), bias_lshift=int(rng.integers(0, 7)), relu=int(rng.integers(0, 2))))
        h, w, c = 1, 1, no
    if not layers:
        return None
    if rng.integers(0, 2):
        layers.append(dict(type=T_SOFTMAX))
    return shape, layers


def random_branching_graph(rng):
    """(shape, layers with explicit `src`): a stem convolution, then one to four blocks -- a DW_Conv2D, an AvgPool, a plain
    convolution, a skip connection (one or two shape-keeping layers, then Add / Sub / Mult with the tensor they started from) or a
    Concat of two 1x1 convolutions of one width -- and sometimes a Dense and a Softmax. Every record is read by a later one."""
    h, w, c = int(rng.integers(4, 13)), int(rng.integers(4, 11)), int(rng.choice([1, 2, 3]))
    shape, layers = (h, w, c), []

    def conv(src, c_in, oc, k, s, same):
        layers.append(dict(type=T_CONV, src=[src], out_ch=oc, kh=k, kw=k, sh=s, sw=s, w=rng.integers(-100, 101, oc * k * k * c_in).astype(np.int8),
                           b=rng.integers(-100, 101, oc).astype(np.int8), out_rshift=int(rng.integers(6, 11)), bias_lshift=int(rng.integers(0, 7)),
                           relu=int(rng.integers(0, 2)), same=same))
        return len(layers) - 1

    def dwconv(src, ch, kh, kw, same):
        layers.append(dict(type=T_DWCONV, src=[src], kh=kh, kw=kw, sh=1, sw=1, w=rng.integers(-100, 101, kh * kw * ch).astype(np.int8),
                           b=rng.integers(-100, 101, ch).astype(np.int8), out_rshift=int(rng.integers(5, 10)), bias_lshift=int(rng.integers(0, 7)),
                           relu=int(rng.integers(0, 2)), same=same))
        return len(layers) - 1

    s = int(rng.integers(1, 3))
    c = int(rng.choice([4, 5, 6, 8, 10, 16]))
    cur = conv(-1, shape[2], c, 3, s, 1)
    h, w = out_dim(h, 3, s, 1), out_dim(w, 3, s, 1)
    for _ in range(int(rng.integers(1, 5))):
        kind = rng.choice(["dw", "avg", "conv", "skip", "skip", "cat"])
        if kind == "dw" and c % 2 == 0:
            kh, kw = [(3, 3), (3, 1), (1, 3), (2, 2)][int(rng.integers(0, 4))]
            same = int(rng.integers(0, 2))
            if out_dim(h, kh, 1, same) < 1 or out_dim(w, kw, 1, same) < 1:
                continue
            cur = dwconv(cur, c, kh, kw, same)
            h, w = out_dim(h, kh, 1, same), out_dim(w, kw, 1, same)
        elif kind == "avg":
            k, st, same = int(rng.integers(2, 4)), int(rng.integers(1, 3)), int(rng.integers(0, 2))
            if out_dim(h, k, st, same) < 1 or out_dim(w, k, st, same) < 1:
                continue
            layers.append(dict(type=T_AVGPOOL, src=[cur], kh=k, kw=k, sh=st, sw=st, same=same))
            cur = len(layers) - 1
            h, w = out_dim(h, k, st, same), out_dim(w, k, st, same)
        elif kind == "conv":
            oc = int(rng.choice([4, 5, 6, 8, 10, 16]))
            cur = conv(cur, c, oc, int(rng.choice([1, 3])), 1, 1)
            c = oc
        elif kind == "skip":
            skip = cur
            for _ in range(int(rng.integers(1, 3))):
                if c % 2 == 0 and rng.integers(0, 2):
                    cur = dwconv(cur, c, 3, 3, 1)
                else:
                    cur = conv(cur, c, c, int(rng.choice([1, 1, 3])), 1, 1)
            op = int(rng.choice([T_ADD, T_ADD, T_SUB, T_MULT]))
            shift = int(rng.choice([0, 5, 6, 7])) if op == T_MULT else int(rng.integers(0, 3))
            layers.append(dict(type=op, src=[cur, skip], out_shift=shift, relu=int(rng.integers(0, 2))))
            cur = len(layers) - 1
        else:
            oc = int(rng.choice([3, 4, 5, 8]))
            a, b = conv(cur, c, oc, 1, 1, 1), conv(cur, c, oc, 1, 1, 1)
            layers.append(dict(type=T_CONCAT, src=[a, b], out_shift=0, relu=int(rng.integers(0, 2))))
            cur, c = len(layers) - 1, 2 * oc
    if rng.integers(0, 2):
        no = int(rng.integers(2, 30))
        layers.append(dict(type=T_DENSE, src=[cur], out=no, w=rng.integers(-100, 101, no * h * w * c).astype(np.int8), b=rng.integers(-100, 101, no).astype(np.int8),
                           out_rshift=int(rng.integers(6, 12)), bias_lshift=int(rng.integers(0, 7)), relu=int(rng.integers(0, 2))))
        cur = len(layers) - 1
        if rng.integers(0, 2):
            layers.append(dict(type=T_SOFTMAX, src=[cur]))
    return shape, layers


def main():
    n_graphs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 77)
    branching = "branching" in sys.argv[3:]
    own = any(a != "branching" for a in sys.argv[3:]) and not branching   # a branching graph has no kernel of its own
    if branching:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import res_ref
    os.environ["EDISON_NET_SPECIALIZE"] = "0"   # loads leave the graph on the general kernel; `own` asks for the own kernel explicitly
    if own:
        os.environ["EDISON_JIT_CACHE"] = "off"
    ctx = Context(0, model_path=None)
    ran = refused = on_mfma = on_own = 0
    while ran + refused < n_graphs:
        g = random_branching_graph(rng) if branching else random_graph(rng)
        if g is None:
            continue
        shape, layers = g
        plain = [dict(L) for L in layers]
        try:
            # Dense weights are random anyway: whatever matrix the importer's de-interleave makes of the stream is the model
            blob = nnom_import.build_blob(shape, [dict(L) for L in layers])
            ctx.load_model_bytes(blob)
        except _lib.EdisonError as e:
            assert e.code in (_lib.E_SIZE, _lib.E_NO_IMPL), str(e)
            refused += 1
            continue
        x = rng.integers(-128, 128, (67, shape[0] * shape[1] * shape[2])).astype(np.int8)
        x[:8] = rng.integers(-10, 11, (8, x.shape[1]))
        ref = res_ref.run(blob, x) if branching else net_ref.run(blob, x)
        got = ctx.net_layers(x)
        want = np.concatenate(ref["acts"], axis=1)
        if not np.array_equal(got, want):
            first = int(np.argwhere(got != want)[0][1])
            raise SystemExit("MISMATCH on graph %s %s at activation byte %d" % (shape, [(L["type"], {k: v for k, v in L.items() if k not in ("w", "b")}) for L in plain], first))
        out = ctx.net(x)
        if not (np.array_equal(out["argmax"], ref["argmax"]) and np.array_equal(out["logits"], ref["logits"])):
            bad = np.argwhere(out["logits"] != ref["logits"])
            raise SystemExit("MISMATCH (batch path, accelerated=%s) on graph %s %s: %d logits differ, first at %s; argmax equal: %s" % (
                ctx.net_info().get("accelerated"), shape, [(L["type"], {k: v for k, v in L.items() if k not in ("w", "b")}) for L in plain],
                len(bad), bad[:1].tolist(), np.array_equal(out["argmax"], ref["argmax"])))
        ran += 1
        on_mfma += 1 if ctx.net_info().get("accelerated") == 2 else 0
        if own and ctx.net_info().get("accelerated") == 2:
            ctx.net_specialize()
            out2 = ctx.net(x)
            if not (np.array_equal(out2["argmax"], ref["argmax"]) and np.array_equal(out2["logits"], ref["logits"])):
                raise SystemExit("MISMATCH (the graph's OWN kernel) on graph %s %s" % (shape, [(L["type"], {k: v for k, v in L.items() if k not in ("w", "b")}) for L in plain]))
            on_own += 1
    print("general network kernel: %d random graphs bit-exact against the restatement (%d of them on the matrix-core kernel, the rest layer by layer%s), %d refused by the planner" % (
        ran, on_mfma, "; %d of them again on their own run-time-compiled kernel" % on_own if own else "", refused))


if __name__ == "__main__":
    main()

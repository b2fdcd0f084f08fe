"""The branching sweep: named graphs chosen so that together they take every path of the passes the fused network kernel
(ed_net_mfma_kernel, csrc/cnn_net_mfma_kernels.hip) grew behind tests/net_sweep.py -- DW_Conv2D and AvgPool on the VALU (ED_RUN_DW,
ED_RUN_AVG), Add / Sub / Mult (ED_RUN_MERGE), Concat (ED_RUN_CAT) -- and every placement the planner (csrc/model_net_mm.c) gives
their tensors: the ping-pong region or a held area, compact, zero-bordered or gapped.

Test infrastructure, not a test: tests/test_branch_sweep_cpu.py checks that the rows reach every item of the restated dispatch
(paths() below) but those in EXCLUDED, that each row is needed, that each note agrees with the plan and that the plan walk
(tests/plan_emulator.py) equals tests/res_ref.py; tests/test_gpu_branch_sweep.py runs every row on the GPU bit for bit against
tests/res_ref.py.

A row is (spec, note). spec: shape (h, w, c) and layers, each a dict made by conv / dw / avg / pool / dense / add / sub / mult / cat
below; `src` names the records a layer reads (default: the one in front). Weights are seeded and scaled layer by layer with
net_sweep._weights so that a layer's outputs spread over about `spread` (net_sweep.TARGET unless the row says otherwise: the merge
rows ask for more, so that their inputs meet at the rails). The note starts with the plan facts it claims, "key=v" tokens before the
';': batch, frag_mode, accelerated, and for a declined graph why=<reason> (decline_reasons below)."""
import functools
import math

import numpy as np

from edison_amd import nnom_import

import net_sweep as ns
import plan_emulator as pe
import res_ref

T_CONV, T_POOL, T_DENSE, T_SOFTMAX, T_DW, T_AVG, T_ADD, T_SUB, T_MULT, T_CAT = range(1, 11)
MAX_MSRC = 64      # ED_MM_MAX_MSRC, edison_internal.h
MAX_LAYERS = 32    # ED_NET_MAX_LAYERS
KIND = {pe.RUN_DW: "DW", pe.RUN_AVG: "AVG", pe.RUN_MERGE: "MERGE", pe.RUN_CAT: "CAT"}
OPS = {T_ADD: "add", T_SUB: "sub", T_MULT: "mult"}


def _2(v):
    return v if isinstance(v, tuple) else (v, v)


def conv(oc, k=1, s=1, same=1, relu=0, rs=9, spread=ns.TARGET, src=None, rails=()):
    return dict(op="conv", oc=oc, k=_2(k), s=_2(s), same=same, relu=relu, rs=rs, spread=spread, src=src, rails=rails)


def dw(k=3, s=1, same=1, relu=0, rs=8, spread=ns.TARGET, src=None, rails=()):
    return dict(op="dw", k=_2(k), s=_2(s), same=same, relu=relu, rs=rs, spread=spread, src=src, rails=rails)


def avg(k, s=None, same=0, src=None):
    return dict(op="avg", k=_2(k), s=_2(k if s is None else s), same=same, src=src)


def pool(k, s=None, same=0, src=None):
    return dict(op="pool", k=_2(k), s=_2(k if s is None else s), same=same, src=src)


def dense(n, relu=0, rs=9, spread=ns.TARGET, src=None):
    return dict(op="dense", n=n, relu=relu, rs=rs, spread=spread, src=src)


def add(*src, shift=0, relu=0):
    return dict(op="add", src=list(src), shift=shift, relu=relu)


def sub(*src, shift=0, relu=0):
    return dict(op="sub", src=list(src), shift=shift, relu=relu)


def mult(*src, shift=0, relu=0):
    return dict(op="mult", src=list(src), shift=shift, relu=relu)


def cat(*src, relu=0):
    return dict(op="cat", src=list(src), relu=relu)


SM = dict(op="softmax", src=None)
PP, PN, NN = (1, -1), (-1, 1), (-1, -1)   # pinned channels (see _bias)
TAIL = [dense(10), SM]


def _heavy():
    """net_sweep._heavy(): more than 96 KB of fragments, so the whole graph streams them from L2 (frag_mode 0)."""
    return [dense(L[1], relu=L[2], rs=L[3]) for L in ns._heavy()] + [SM]


ROWS = {}


def _row(name, shape, layers, note):
    assert len(layers) <= MAX_LAYERS and shape[0] <= 12 and shape[1] <= 10
    ROWS[name] = (dict(shape=shape, layers=layers), note)


IN = (12, 10, 1)
# ---- sequential graphs: the two VALU layers into every layout a consumer can ask for
_row("dw_gap", (9, 10, 1), [conv(32, 3, relu=1), dw(3, relu=1), conv(16, 1), pool((3, 5))] + TAIL,
     "batch=2 frag_mode=2; DW over 32 channels (dwords) into the 48-byte pixel pitch of a 1x1 convolution; SAME: border taps skipped; ReLU")
_row("avg_gap", IN, [conv(64, 3), avg((2, 1)), conv(16, 1), pool((3, 5))] + TAIL,
     "batch=1 frag_mode=2; AvgPool over 64 channels into an 80-byte pixel pitch; every window inside the image")
_row("dw_border_half", IN, [conv(6, 3, 2), dw((3, 1), rs=6, spread=100), conv(8, 3)] + TAIL,
     "batch=4 frag_mode=2; DW over 6 channels (16-bit words and a tail group), a 3 x 1 kernel, no ReLU, accumulators at both clamps, "
     "into the zero border of a SAME 3 x 3 convolution")
_row("avg_border_half", IN, [conv(10, 3, 2), avg(3, 1, same=1), conv(8, 3)] + TAIL,
     "batch=4 frag_mode=2; AvgPool over 10 channels, SAME: 4, 6 or 9 taps; 90 groups per image; into a zero border")
_row("dw_l2_valid", IN, [conv(8, 3, 2), dw((2, 3), (2, 1), same=0, relu=1)] + _heavy(),
     "batch=4 frag_mode=0; DW weights from L2, VALID: no tap skipped, stride 2 along y only")
_row("avg_whole_square", (10, 10, 1), [conv(8, 3, 2), avg(5)] + TAIL,
     "batch=4 frag_mode=2; the 5 x 5 AvgPool over a whole square 5 x 5 map")
_row("x64", IN, [conv(16, 3, 3), dw(3, rails=PP), avg(3, 1, same=1), add(2, 1, shift=1)] + TAIL,
     "batch=4 frag_mode=2; 4 x 4 pixels x 4 groups: every VALU and merge pass has exactly 64 lanes of work per image; the DW output held")
# ---- residual graphs: the merge passes, their sources and the held areas
_row("add_padded_held", IN, [conv(8, 3, 2, rails=PP), conv(8, 3, relu=1, src=[0]), conv(8, 1, rails=PP), add(2, 0, relu=1)] + TAIL,
     "batch=4 frag_mode=2; Add at shift 0 with a ReLU tail; the skip tensor is held in the zero-bordered layout of the SAME 3 x 3 "
     "convolution that also reads it, the other input compact in the region")
_row("alive_reuse", IN, [conv(6, 3, 2, spread=80, rails=PN), conv(6, 1, spread=80, rails=PN), conv(6, 1, spread=80, rails=PP), sub(2, 0, shift=1),
                         conv(6, 1, spread=80, src=[3], rails=NN), mult(4, 1), conv(6, 1, spread=80, rails=PN), mult(6, 4, shift=6)] + TAIL,
     "batch=4 frag_mode=2; 6 channels (a tail group); records 0 and 1 held at once, record 4 takes record 0's offset after its last reader; "
     "Sub at shift 1, Mult at shift 0 and at shift 6")
_row("add3", IN, [conv(8, 3, 2, spread=60, rails=PP), conv(8, 1, spread=60, rails=PP), conv(8, 1, spread=60, rails=PP), add(2, 1, 0), conv(8, 1, rails=PP), add(4, 3, 1, shift=1, relu=1)] + TAIL,
     "batch=4 frag_mode=2; Add over three inputs at shift 0 and at shift 1; the first Add's output is held")
_row("pool_held", IN, [conv(16, 3), conv(8, 1, rails=PP), pool(2), conv(8, 3, src=[2]), conv(8, 1, rails=PP), add(4, 2, shift=1)] + TAIL,
     "batch=4 frag_mode=2; the output of a MaxPool fused into its convolution is held, in the layout of the SAME 3 x 3 convolution behind it")
_row("avg_held", IN, [conv(6, 3, 2, rails=PN), avg(3, 1, same=1), conv(6, 1, rails=PP), sub(2, 1)] + TAIL,
     "batch=4 frag_mode=2; an AvgPool output held; Sub at shift 0 over 6 channels")
_row("merge_border", IN, [conv(8, 3, 2, rails=PN), conv(8, 1, rails=PP), sub(1, 0, shift=1, relu=1), conv(8, 3)] + TAIL,
     "batch=4 frag_mode=2; a merge pass stores into the zero border of a SAME 3 x 3 convolution")
# ---- Concat
_row("cat2_odd", IN, [conv(5, 3, (4, 5)), conv(5, 1, src=[0], rails=PP), conv(5, 1, src=[0]), cat(1, 2, relu=1), conv(10, 1, rails=PN), sub(4, 3)] + TAIL,
     "batch=4 frag_mode=2; Concat of two 5-channel inputs of 3 x 2 pixels with a ReLU tail, its output held for the Sub behind it")
_row("cat3_mixed", IN, [conv(4, 3, 2), conv(4, 1, src=[0]), conv(4, 1, src=[0]), conv(4, 3, src=[1]), cat(1, 2, 3), conv(8, 3)] + TAIL,
     "batch=4 frag_mode=2; Concat of three 4-channel inputs: the first in the zero-bordered layout of the 3 x 3 convolution that reads it "
     "too, the others compact; the output into a zero border")
# ---- fragments streamed from L2 behind the branch: the FRAG_LDS = false instance of every pass
_row("branch_l2", IN, [conv(8, 3, 2), dw(3, rails=PP), avg(3, 1, same=1), add(2, 1, shift=1), cat(3, 1)] + _heavy(),
     "batch=4 frag_mode=0; DW, AvgPool, Add and Concat in the kernel instance that streams fragments from L2")
# ---- declined by the fused planner: the layer-by-layer kernel runs them
_row("no_odd_merge", IN, [conv(5, 3, 2, rails=PP), conv(5, 1, rails=PP), add(1, 0)] + TAIL,
     "accelerated=0 why=odd_merge; Add over 5 channels")
_row("no_odd_avg", IN, [conv(5, 3, 2), avg(3, 1, same=1)] + TAIL,
     "accelerated=0 why=pitch; AvgPool over 5 channels: no 16-bit words")
_row("no_layouts", IN, [conv(8, 3, 2), conv(8, 1, src=[0], rails=PP), conv(8, 3, src=[0], rails=PP), add(1, 2)] + TAIL,
     "accelerated=0 why=layouts; a 1x1 and a zero-padded 3x3 convolution read one tensor")
_row("no_msrc", IN, [conv(8, 3, 2, spread=6, rails=(1, -1, 1)), conv(8, 1, spread=6, rails=(1, -1, -1))] + [add(i + 1, 0, 1, 0, 1, 0, 1, 0) for i in range(9)] + TAIL,
     "accelerated=0 why=msrc; nine Adds over eight inputs each (the one in front and the two stems in turn): 72 merge inputs")


# ---- building ---------------------------------------------------------------------------------------------------------------
def _srcs(spec):
    return [list(L["src"]) if L.get("src") is not None else [i - 1] for i, L in enumerate(spec["layers"])]


def _record(L, wt=None, b=None, bl=0):
    op = L["op"]
    if op in ("conv", "dw"):
        d = dict(type=T_CONV if op == "conv" else T_DW, kh=L["k"][0], kw=L["k"][1], sh=L["s"][0], sw=L["s"][1], same=L["same"], relu=L["relu"],
                 w=wt, b=b, out_rshift=L["rs"], bias_lshift=bl)
        if op == "conv":
            d["out_ch"] = L["oc"]
        return d
    if op == "dense":
        return dict(type=T_DENSE, out=L["n"], w=wt, b=b, out_rshift=L["rs"], bias_lshift=bl, relu=L["relu"])
    if op in ("avg", "pool"):
        return dict(type=T_AVG if op == "avg" else T_POOL, kh=L["k"][0], kw=L["k"][1], sh=L["s"][0], sw=L["s"][1], same=L["same"])
    if op == "softmax":
        return dict(type=T_SOFTMAX)
    return dict(type={"add": T_ADD, "sub": T_SUB, "mult": T_MULT, "cat": T_CAT}[op], out_shift=L.get("shift", 0), relu=L["relu"])


def _bias(rng, mean, rs, spread, rails=()):
    """The bias centres every output channel, give or take a quarter of the spread (net_sweep._layers). `rails`: the first channels
    are pinned instead, channel j at 127 (rails[j] > 0) or -128 whatever the input -- the caller zeroes their weights, and the
    layer's bias shift grows to rs + 3 so that a bias byte reaches past the clamp -- so that two tensors meet at chosen corners of a
    merge layer behind them: PP = (1, -1) against PP gives (127, 127) and (-128, -128), against PN = (-1, 1) the mixed corners."""
    bl = rs + 3 if rails else max(rs - 1, 0)
    b = np.clip(np.round((-mean + rng.normal(0, spread / 4 * 2.0 ** rs, mean.shape)) / 2.0 ** bl), -128, 127).astype(np.int8)
    for j, sign in enumerate(rails):
        b[j] = 127 if sign > 0 else -128
    return b, bl


@functools.lru_cache(maxsize=None)
def _layers(name):
    spec = ROWS[name][0]
    shape, srcs = spec["shape"], _srcs(spec)
    rng = np.random.default_rng(sum(map(ord, name)) * 7919)
    x = ns.inputs(name, 40, shape[0] * shape[1] * shape[2])
    acts, shapes, out = [], [], []
    for i, L in enumerate(spec["layers"]):
        s0 = srcs[i][0]
        h, w, c = shape if s0 < 0 else shapes[s0]
        cur = (x if s0 < 0 else acts[s0]).reshape(len(x), h, w, c)
        op = L["op"]
        if op in ("conv", "dense", "dw"):
            rs_eff = L["rs"] + math.log2(L["spread"] / ns.TARGET)       # net_sweep._weights scales to TARGET << rs
            f = cur.astype(np.float64)
            if op == "conv":
                P = ns._patches(f, L["k"][0], L["k"][1], L["s"][0], L["s"][1], L["same"])
                wt, mean = ns._weights(rng, P, L["oc"], rs_eff, 127)
                wt[:len(L["rails"])] = 0
                wt = wt.reshape(-1)
            elif op == "dense":
                wt, mean = ns._weights(rng, f.reshape(len(x), -1), L["n"], rs_eff, 127)
                wt = ns.interleave_dense_opt(wt)
            else:                                                        # per channel its own taps; weights [ky][kx][ch]
                P = ns._patches(f, L["k"][0], L["k"][1], L["s"][0], L["s"][1], L["same"]).reshape(-1, L["k"][0] * L["k"][1], c)
                cols = [ns._weights(rng, P[:, :, ch], 1, rs_eff, 127) for ch in range(c)]
                wt = np.stack([q[0][0] for q in cols], axis=1)
                wt[:, :len(L["rails"])] = 0
                wt = wt.reshape(-1)
                mean = np.array([q[1][0] for q in cols])
            b, bl = _bias(rng, mean, L["rs"], L["spread"], L.get("rails", ()))
            d = _record(L, wt, b, bl)
        else:
            d = _record(L)
        d["src"] = srcs[i]
        out.append(d)
        # this record's output over the 40 inputs, for the scaling of the layers behind it (the expected values of the tests are
        # res_ref.run's over the whole graph, not these)
        if op == "softmax":
            acts.append(None)
            shapes.append((h, w, c))
        elif op == "cat":
            acts.append(np.concatenate([acts[t].reshape(len(x), h * w, c) for t in srcs[i]], axis=2).reshape(len(x), -1).clip(0 if L["relu"] else -128))
            shapes.append((h, w, c * len(srcs[i])))
        elif op in ("add", "sub", "mult"):
            ins = [acts[t] for t in srcs[i]]
            r = res_ref.merge2(d["type"], L["shift"], ins[0], ins[1])
            for t in ins[2:]:
                r = res_ref.merge2(d["type"], L["shift"], t, r)
            acts.append(np.maximum(r, 0 if L["relu"] else -128).astype(np.int8))
            shapes.append((h, w, c))
        else:
            one = nnom_import.build_blob((h, w, c), [{k: v for k, v in d.items() if k != "src"}])
            acts.append(res_ref.run(one, cur.reshape(len(x), -1))["acts"][0])
            shapes.append(res_ref._out_shape(res_ref.net_ref.parse_blob(one)[1][0], (h, w, c)))
    return shape, out


def layers(name):
    """Row `name` -> (shape, nnom_import.build_blob layer list) with seeded, scaled weights."""
    shape, lay = _layers(name)
    return shape, [dict(L) for L in lay]


@functools.lru_cache(maxsize=None)
def blob(name):
    shape, lay = layers(name)
    return nnom_import.build_blob(shape, lay)


def inputs(name, n, in_n=None):
    shape = ROWS[name][0]["shape"]
    return ns.inputs(name, n, shape[0] * shape[1] * shape[2] if in_n is None else in_n)


def cuts(name):
    """[(li, blob)]: row `name` cut behind record li wherever the cut is a graph of its own -- every record in front of li is read
    inside the cut (nnom_import.build_blob refuses an unread tensor) and a fusable MaxPool stays with its convolution -- so that the
    record's own output is the logits the batch path returns."""
    shape, lay = layers(name)
    out = []
    for li in range(len(lay) - 1):
        if lay[li]["type"] == T_SOFTMAX:
            continue
        nxt = lay[li + 1]
        if lay[li]["type"] == T_CONV and nxt["type"] == T_POOL and nxt["src"] == [li]:
            continue                                     # cut behind the pool instead
        read = {t for L in lay[:li + 1] for t in L["src"]}
        if all(t in read for t in range(li)):
            out.append((li, nnom_import.build_blob(shape, [dict(L) for L in lay[:li + 1]])))
    return out


# ---- the kernel's and the planner's choices, restated -------------------------------------------------------------------------
def band(work):
    """The lane loop `for (i = lane; i < work; i += 64)` of a VALU / merge pass: less than one sweep, whole sweeps, or a ragged last one."""
    return "<64" if work < 64 else ("x64" if work % 64 == 0 else ">64+")


def _held(plan):
    """{tensor: (first byte, end, storing pass, last reading pass)} of the tensors the plan keeps in held areas."""
    M = plan.M
    hold0 = 2 * M.buf_bytes + M.x_bytes
    out = {}
    for li, R in enumerate(plan.R):
        if R.kind != pe.RUN_SKIP and R.o_off >= hold0:
            t = R.li_out
            out[t] = (R.o_off, R.o_off + M.batch * R.o_img, li, max(j for j in range(plan.P.n_layers) if t in plan.src[j]))
    return out


def paths(plan, nb):
    """What the fused kernel runs for the VALU, merge and Concat passes of a plan at a per-wave fill nb (1 .. batch), and where the
    planner put what they read and store: dict(batch, frag_mode, runs = one dict per such pass, held = set of held-area facts).
    cnn_net_mfma_kernels.hip:1095-1218, model_net_mm.c:196-241, 518-659."""
    M = plan.M
    fl = M.frag_mode == 2
    hold0 = 2 * M.buf_bytes + M.x_bytes
    place = lambda off: "held" if off >= hold0 else "region"       # noqa: E731
    runs = []
    for li, R in enumerate(plan.R):
        if R.kind not in KIND:
            continue
        L = plan.PL[li]
        kind = KIND[R.kind]
        c_out = R.out_c if kind in ("MERGE", "CAT") else L.in_c
        d = dict(kind=kind, frag_lds=fl, out_place=place(R.o_off), relu=R.lo_clamp == 0, border=bool(R.zero_border), gap=R.oc_pitch != c_out)
        if kind in ("DW", "AVG"):
            c4n = (L.in_c + 3) // 4
            d.update(group="dword" if L.in_c % 4 == 0 else "half", band=band(nb * L.out_h * L.out_w * c4n), skipped=bool(L.check_taps))
            if kind == "DW":
                d.update(stride="1" if (L.sh, L.sw) == (1, 1) else ("one axis" if 1 in (L.sh, L.sw) else "both"), square=L.kh == L.kw)
            else:
                d["whole_square"] = L.in_h == L.in_w and (L.kh, L.kw) == (L.in_h, L.in_w) and not L.check_taps
        else:
            h, w = R.pix_per_img // R.col_w, R.col_w
            c = R.pitch_x if kind == "CAT" else R.out_c
            ms = [[int(v) for v in plan.msrc[5 * (R.koff_off + k):5 * (R.koff_off + k) + 5]] for k in range(R.n_ks)]
            d.update(n_in=R.n_ks, src_place=[place(e[0]) for e in ms],
                     src_layout=["gapped" if e[4] != c else ("compact" if (e[2], e[3]) == (0, w * c) else "padded") for e in ms])
            if kind == "MERGE":
                d.update(op=OPS[R.ph], shift="0" if (R.rs & 0xff) == 0 else ">0", group="dword" if c % 4 == 0 else "half",
                         band=band(nb * R.pix_per_img * ((c + 3) // 4)))
            else:
                d.update(parity="odd" if c % 2 else "even", band=band(nb * R.pix_per_img * c), differing=len({tuple(e[2:]) for e in ms}) > 1)
        runs.append(d)
    held, facts = _held(plan), set()
    for t, (lo, hi, st, last) in held.items():
        R = plan.R[st]
        if st != t:
            facts.add("fused pool output")
        if R.zero_border and any(plan.PL[j].type == T_CONV and (plan.PL[j].kh, plan.PL[j].kw, plan.PL[j].pad_h, plan.PL[j].pad_w) == (3, 3, 1, 1)
                                 for j in range(plan.P.n_layers) if t in plan.src[j]):
            facts.add("padded for a SAME 3x3 convolution")
        for u, (lo2, hi2, st2, last2) in held.items():
            if u >= t:
                continue
            alive = st2 <= last and st <= last2
            if alive and (lo2, hi2) != (lo, hi):
                facts.add("two alive")
            if not alive and lo2 < hi and lo < hi2:
                facts.add("offset reused")
    return dict(batch=M.batch, frag_mode=M.frag_mode, runs=runs, held=facts)


def items(plan, nb):
    """paths(plan, nb) as a set of coverage items."""
    p = paths(plan, nb)
    out = {("batch", p["batch"]), ("frag_mode", p["frag_mode"]), ("fill", p["batch"], nb)} | {("held", f) for f in p["held"]}
    for d in p["runs"]:
        k = d["kind"]
        out.add(("pass", k, d["frag_lds"]))
        out.add(("out", k, "held" if d["out_place"] == "held" else "region"))
        out.add(("out", k, "gap" if d["gap"] else ("border" if d["border"] else "compact")))
        out.add(("relu", k, d["relu"]))
        out.add(("band", k, d["band"]))
        if k != "CAT":
            out.add(("group", k, d["group"]))
        if k == "DW":
            out |= {("dw", "weights", "lds" if d["frag_lds"] else "l2"), ("dw", "taps", "skipped" if d["skipped"] else "all"),
                    ("dw", "stride", d["stride"]), ("dw", "kernel", "square" if d["square"] else "nonsquare")}
        elif k == "AVG":
            out.add(("avg", "taps", "varying" if d["skipped"] else "constant"))
            if d["whole_square"]:
                out.add(("avg", "whole square map"))
        elif k == "MERGE":
            out.add(("merge", d["op"] if d["n_in"] == 2 else "add3", d["shift"]))
            out |= {("merge", "src", s) for s in d["src_place"]} | {("merge", "src", s) for s in d["src_layout"]}
        else:
            out |= {("cat", "channels", d["parity"]), ("cat", "inputs", min(d["n_in"], 3)), ("cat", "layouts", "differing" if d["differing"] else "same")}
    return out


def plan_items(plan):
    """The union of items() over every per-wave fill 1 .. batch."""
    return set().union(*(items(plan, nb) for nb in range(1, plan.M.batch + 1)))


DECLINES = ("odd_merge", "pitch", "layouts", "msrc")


def full_set():
    """Every item a graph could reach: the product of the choices above."""
    s = {("batch", b) for b in (1, 2, 4)} | {("frag_mode", m) for m in (0, 2)} | {("fill", b, nb) for b in (1, 2, 4) for nb in range(1, b + 1)}
    s |= {("held", f) for f in ("two alive", "offset reused", "fused pool output", "padded for a SAME 3x3 convolution")}
    for k in ("DW", "AVG", "MERGE", "CAT"):
        s |= {("pass", k, fl) for fl in (False, True)} | {("out", k, v) for v in ("region", "held", "compact", "border", "gap")}
        s |= {("relu", k, r) for r in (False, True)} | {("band", k, b) for b in ("<64", "x64", ">64+")}
        if k != "CAT":
            s |= {("group", k, g) for g in ("dword", "half")}
    s |= {("dw", "weights", v) for v in ("lds", "l2")} | {("dw", "taps", v) for v in ("skipped", "all")} | {("dw", "stride", v) for v in ("1", "one axis")}
    s |= {("dw", "kernel", v) for v in ("square", "nonsquare")} | {("avg", "taps", v) for v in ("varying", "constant")} | {("avg", "whole square map")}
    s |= {("merge", op, sh) for op in ("add", "sub", "mult", "add3") for sh in ("0", ">0")}
    s |= {("merge", "src", v) for v in ("region", "held", "compact", "padded", "gapped")}
    s |= {("cat", "channels", v) for v in ("odd", "even")} | {("cat", "inputs", v) for v in (2, 3)} | {("cat", "layouts", v) for v in ("same", "differing")}
    s |= {("declined", why) for why in DECLINES}
    return s


# item -> why no legal plan produces it (derived from the planner, model_net_mm.c)
EXCLUDED = {
    ("relu", "AVG", True): "model_net.c:192-197 gives an AvgPool no ReLU (the importer accepts the tail activation only behind Conv2D, DW_Conv2D, "
                           "Dense and the merge layers), so model_net_mm.c:645 always sets lo_clamp = -128 for it",
    ("out", "MERGE", "gap"): "model_net_mm.c:176: the pixel-gap loop runs only for a sequential graph (`!br`), and a merge layer makes a graph branching",
    ("out", "CAT", "gap"): "model_net_mm.c:176: no pixel gaps in a branching graph, and a Concat makes a graph branching",
    ("merge", "src", "gapped"): "model_net_mm.c:176, 624: without pixel gaps in a branching graph every msrc pixel pitch is the channel count",
}


def claims(note):
    out = {}
    for t in note.split(";")[0].split():
        k, v = t.split("=")
        out[k] = v if k == "why" else int(v)
    return out


def decline_reasons(name):
    """Why the fused planner declines row `name`, restated from model_net_mm.c over the row's records: the set of
    odd_merge  :616  Add / Sub / Mult over an odd channel count
    pitch      :632  a DW / AvgPool / merge pass whose stored pixel pitch is odd (or not a multiple of 4 under dword groups)
    layouts    :214  two readers that demand different LDS layouts of one tensor: here a padded and an unpadded convolution
    msrc       :616  more than ED_MM_MAX_MSRC merge inputs"""
    shape, lay = layers(name)
    P = res_ref.net_ref.parse_blob(blob(name))[1]
    why, n_msrc, ch = set(), 0, []
    for i, (L, v) in enumerate(zip(lay, P)):
        c_in = shape[2] if L["src"][0] < 0 else ch[L["src"][0]]
        ch.append(v[1] if v[0] in (T_CONV, T_DENSE, T_ADD, T_SUB, T_MULT, T_CAT) else c_in)
        if v[0] in (T_ADD, T_SUB, T_MULT, T_CAT):
            n_msrc += len(L["src"])
            if n_msrc > MAX_MSRC:
                why.add("msrc")
            if v[0] != T_CAT and c_in % 2:
                why.add("odd_merge")
        if v[0] in (T_DW, T_AVG) and c_in % 2:
            why.add("pitch")
        pads = {(((v2[2] - 1) // 2, (v2[3] - 1) // 2) if (v2[8] >> 1) & 1 else (0, 0))
                for L2, v2 in zip(lay, P) if v2[0] == T_CONV and L2["src"] == [i]}
        if len(pads) > 1:
            why.add("layouts")
    return why


def variants(name):
    """The `wrong` readings of tests/res_ref.py and tests/dscnn_ref.py that change something row `name` computes: each one's operation
    is in the graph in a form the reading gets wrong (truncate: a merge at shift > 0; count_area: an AvgPool window that leaves the
    image; chw_weights: a DW_Conv2D with several taps and channels; ...)."""
    shape, lay = layers(name)
    out, ch = set(), []
    for L in lay:
        c_in = shape[2] if L["src"][0] < 0 else ch[L["src"][0]]
        t = L["type"]
        ch.append(L["out_ch"] if t == T_CONV else L["out"] if t == T_DENSE else c_in * len(L["src"]) if t == T_CAT else c_in)
        if t in (T_ADD, T_SUB, T_MULT) and L["out_shift"] > 0:
            out.add("truncate")
        if t == T_MULT and L["out_shift"] == 0:
            out.add("mult_no_q7")
        if t == T_ADD and len(L["src"]) >= 3:
            out.add("add_wide")
        if t == T_SUB:
            out.add("sub_swapped")
        if t == T_CAT:
            out.add("concat_planar")
        if t == T_AVG:
            out.add("floor_div")
            if L["same"] and (L["kh"] > 1 or L["kw"] > 1):
                out.add("count_area")
        if t == T_DW:
            if L["out_rshift"] > 0:
                out.add("no_round")
            if L["kh"] * L["kw"] > 1 and c_in > 1:
                out.add("chw_weights")
    return out


VARIANTS = ("truncate", "mult_no_q7", "add_wide", "sub_swapped", "concat_planar", "floor_div", "count_area", "no_round", "chw_weights")

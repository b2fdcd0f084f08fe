"""The int8 network sweep: named graphs chosen so that together they take every path of the general matrix-core network kernel
(ed_net_mfma_kernel, csrc/cnn_net_mfma_kernels.hip) and of a graph's own kernel (ed_net_mfma_spec, the same text with -DEMM_SPEC),
as the planner (csrc/model_net_mm.c) lays them out.

Test infrastructure, not a test: tests/test_net_sweep_cpu.py checks that the rows reach every item of the restated dispatch
(paths() below) but those in EXCLUDED, that each note agrees with the plan and that the plan walk (tests/plan_emulator.py) equals
oracle/net_ref.py; tests/test_gpu_net_sweep.py runs every row on the GPU bit for bit against oracle/net_ref.py.

A row is (spec, note). spec: shape (h, w, c) and layers, each
  ("conv", out_c, (kh, kw), (sh, sw), same, relu, rs, wmax, bl)
  ("pool", (kh, kw), (sh, sw), same)
  ("dense", n, relu, rs, wmax, bl)
  ("softmax",)
Weights are seeded and scaled layer by layer (_weights, at most wmax in magnitude) so that every layer's outputs spread over about
+-TARGET for the row's inputs: each layer's result reaches the logits (tests/test_net_sweep_cpu.py corrupts every layer in
oracle/net_ref.py and requires the logits to change). Biases centre each output channel, bias_lshift = rs - 1; but where
bl >= 20 the first two channels get 127 and -128 << bl and the others 0 -- the layer's accumulator bound then keeps the plain
shift-and-clamp requantisation while the other channels stay off the rails. The note starts with the plan facts it claims, "key=v" tokens before the ';': batch, frag_mode, waves, accelerated."""
import functools

import numpy as np

from edison_amd import nnom_import

import plan_emulator as pe

T_CONV, T_POOL, T_DENSE, T_SOFTMAX = 1, 2, 3, 4
RS_HI, RS_MASK = 0x100, 0xff
RES_MAX = 8        # EMM_RES_MAX, cnn_net_mfma_kernels.hip:303
INTAB_PAD = 512    # ED_MM_INTAB_PAD, edison_internal.h
PB = 2             # EMM_PB of the general kernel (a graph's own kernel: 4), cnn_net_mfma_kernels.hip:229-231

# the 32 x 32 tile groups (NW, R, C) of emm_layer_dispatch (cnn_net_mfma_kernels.hip:759-773) and the 16 x 16 x 64 units U
TILE_SHAPES = ((1, 2, 2), (1, 2, 1), (1, 1, 2), (1, 1, 1), (2, 2, 1), (2, 1, 2), (2, 1, 1), (4, 1, 1))
SMALL_UNITS = (1, 2, 4)
# the epilogue: 0 shift + two clamps (emm_pack4), 1 / 2 / 3 high byte of sat16 with no / a right / a left shift (emm_pack4_hi),
# 4 byte stores (C_out % 4 != 0)
EPILOGUES = (0, 1, 2, 3, 4)


def _c(oc, k=3, s=1, same=1, relu=1, rs=9, wmax=127, bl=0):
    kk = k if isinstance(k, tuple) else (k, k)
    ss = s if isinstance(s, tuple) else (s, s)
    return ("conv", oc, kk, ss, same, relu, rs, wmax, bl)


def _d(n, relu=1, rs=9, wmax=127, bl=0):
    return ("dense", n, relu, rs, wmax, bl)


def _p(k, s=None, same=0):
    kk = k if isinstance(k, tuple) else (k, k)
    ss = kk if s is None else (s if isinstance(s, tuple) else (s, s))
    return ("pool", kk, ss, same)


SM = ("softmax",)
# requantisation of a layer by the epilogue it is meant to take (the planner decides: ED_RUN_RS_HI, model_net_mm.c)
E0 = dict(rs=6, bl=23)              # with bias "rails": the bound << (8 - rs) leaves 32 bits -> shift and two clamps
E1 = dict(rs=8)                     # high byte, no shift
E2 = dict(rs=9)                     # high byte after a right shift
E3 = dict(rs=4, wmax=3)             # high byte after a left shift: small weights keep the bound << 4 inside 32 bits


def _heavy():
    """Dense layers of 1024 outputs and then of 1024 inputs: more than 96 KB of fragments, so the whole graph streams them from L2
    (frag_mode 0)."""
    return [_d(1024, relu=0, **E2), _d(100, relu=1, rs=13)]


# ---- the chains: layer by layer the epilogue and the tile group change; each comes twice, with the fragments resident in LDS
# (frag_mode 2) and, behind dense layers of more than 96 KB of fragments, streamed from L2 (frag_mode 0)
def _chain_nw1(tail):
    # 1 x 1 convolutions over 3 x 8 pixels: 24 / 48 columns (1 / 2 column tiles) at 1 / 2 inputs per wave; C_out <= 32 (one row
    # tile), 33..64 (two), 65..96 (three: an odd count) in turn, so that the inputs of the wide layers stay narrow
    return [_c(32, 1, relu=0, **E1), _c(48, 1, **E1), _c(16, 1, **E3), _c(64, 1, relu=0, **E3), _c(32, 1, relu=0, **E0),
            _c(96, 1, **E0), _c(16, 1, **E2), _c(80, 1, relu=0, **E2), _c(18, 1, **E2), _c(42, 1, **E2), _c(16, 1, **E2),
            _c(70, 1, **E2), _c(16, 1, **E2)] + tail


def _chain_nw2(order, tail):
    # conv + MaxPool (2, 1) / (1, 2) fused, 32 x 32 -> 1 x 1: 512 .. 64 pooled pixels (two or more column tiles), then 32 .. 1 (one);
    # order: (C_out, epilogue) per layer
    e = (E0, E1, E2, E3, E2)
    out = []
    for i, (oc, q) in enumerate(order):
        out += [_c(oc, 1, relu=i % 2, **e[q]), _p((2, 1) if i % 2 == 0 else (1, 2))]
    return out + tail


def _chain_nw4(tail):
    # conv + MaxPool (2, 2) fused, every epilogue: 32 x 32 -> 1 x 1
    return [_c(16, 1, **E0), _p(2), _c(18, 1, **E2), _p(2), _c(32, 1, relu=0, **E1), _p(2), _c(48, 1, **E2), _p(2), _c(32, 1, **E3), _p(2)] + tail


def _chain_small(head, tail):
    # dense layers on 16 x 16 x 64 tiles: 1 / 2 / 4 row tiles at a time (C_out <= 16, 17..32, >= 33)
    return head + [_d(36, relu=0, **E1), _d(16, **E2), _d(24, relu=0, **E3), _d(40, **E0), _d(12, **E3), _d(20, relu=1, **E1),
                   _d(44, **E2), _d(8, **E0), _d(32, **E0), _d(37, **E2), _d(10, **E1), _d(18, relu=0, **E2), _d(48, **E3),
                   _d(16, **E1), _d(28, **E2), _d(9, **E2)] + tail


ROWS = {}


def _row(name, shape, layers, note):
    ROWS[name] = (dict(shape=shape, layers=layers), note)


_row("nw1_lds", (3, 8, 16), _chain_nw1([_d(10, **E2), SM]), "batch=2 frag_mode=2; 32 x 32 tiles without windows: every group, every epilogue")
_row("nw1_l2", (3, 8, 16), _chain_nw1(_heavy() + [SM]), "batch=2 frag_mode=0; the same over fragments streamed from L2")
NW2A = [(16, 0), (16, 1), (32, 2), (16, 3), (16, 0), (18, 4), (16, 1), (16, 2), (48, 3)]
NW2B = [(16, 3), (10, 4), (16, 1), (48, 0), (64, 1), (40, 2), (64, 3), (38, 4), (48, 1)]
_row("nw2a_lds", (32, 16, 16), _chain_nw2(NW2A, [_d(12, **E1), SM]), "batch=1 frag_mode=2; fused (2, 1) and (1, 2) windows")
_row("nw2b_lds", (32, 16, 16), _chain_nw2(NW2B, [_d(12, **E1), SM]), "batch=1 frag_mode=2; the other epilogues on the same windows")
_row("nw2a_l2", (32, 16, 16), _chain_nw2(NW2A, _heavy() + [SM]), "batch=1 frag_mode=0; fused (2, 1) and (1, 2) windows")
_row("nw2b_l2", (32, 16, 16), _chain_nw2(NW2B, _heavy() + [SM]), "batch=1 frag_mode=0; the other epilogues on the same windows")
_row("nw4_lds", (32, 32, 16), _chain_nw4([_d(12, **E1), SM]), "batch=1 frag_mode=2; fused 2 x 2 windows, every epilogue")
_row("nw4_l2", (32, 32, 16), _chain_nw4(_heavy() + [SM]), "batch=1 frag_mode=0; fused 2 x 2 windows over fragments streamed from L2")
_row("small_lds", (4, 4, 8), _chain_small([], [SM]), "batch=4 frag_mode=2; 16 x 16 x 64 tiles, 1 / 2 / 4 units, every epilogue")
_row("small_l2", (8, 8, 16), _chain_small([_d(64, **E2)], [SM]), "batch=4 frag_mode=0; the same over fragments streamed from L2")


# ---- the tables, the input stages, the other runs
_row("tables_overflow", (36, 32, 4), [_c(8, 3, same=0, relu=0, **E2), _c(12, 3, 2, same=0, **E1), _c(16, 3, 2, same=0, **E2),
                                      _c(16, 3, 2, same=0, **E3), _d(10, **E2), SM],
     "batch=1 frag_mode=2; 4608 input bytes (no input table: the kernel divides), 1020 stored pixels in the first layer: the "
     "column table is full for the next two (32 x 32 tiles) and the fourth (16 x 16), the expansion table for the second")
_row("toeplitz_pools", (20, 13, 1), [_c(8, 3, same=0, **E2), _p((2, 1)), _p(3, 1, same=1), _c(16, 3, **E1), _c(10, 3, relu=0, **E2),
                                     _p(3, 2), _c(12, 3, **E3), _p(2, 2, same=1), _c(18, 1, **E2), _p((1, 3)), _d(40, **E2), SM],
     "batch=2 frag_mode=2; a row-Toeplitz first layer with a fused (2, 1) window; MaxPools over 4-channel dwords and over bytes, "
     "with and without the consumer's zero border; 40 classes")
_row("accel0_dense4112", (16, 257, 1), [_d(5, **E2), SM],
     "accelerated=0; a dense layer over 4112 inputs: 258 k-steps are more than a matrix-core plan holds, the layer-by-layer kernel runs it")


# ---- building ---------------------------------------------------------------------------------------------------------------
TARGET = 40        # the spread (rms) a layer's requantised outputs are scaled to, before the clamp and the ReLU


_BLK = np.array([(0, 0), (1, 0), (0, 2), (1, 2), (2, 0), (3, 0), (2, 2), (3, 2), (0, 1), (1, 1), (0, 3), (1, 3), (2, 1), (3, 1), (2, 3), (3, 3)])


def interleave_dense_opt(w):
    """[rows][cols] -> the weight stream nnom_import.deinterleave_dense_opt reads back as w (arm_fully_connected_q7_opt's order)."""
    rows, cols = w.shape
    r4, c4, cr = rows // 4, cols // 4, cols % 4
    pos = np.zeros((rows, cols), np.int64)       # stream position of each weight
    per = 16 * c4 + 4 * cr                       # stream bytes per group of 4 rows
    g, b, i = np.meshgrid(np.arange(r4), np.arange(c4), np.arange(16), indexing="ij")
    pos[4 * g + _BLK[i, 0], 4 * b + _BLK[i, 1]] = g * per + 16 * b + i
    g, c, d = np.meshgrid(np.arange(r4), np.arange(cr), np.arange(4), indexing="ij")
    pos[4 * g + d, 4 * c4 + c] = g * per + 16 * c4 + 4 * c + d
    r, c = np.meshgrid(np.arange(rows - 4 * r4), np.arange(cols), indexing="ij")
    pos[4 * r4 + r, c] = 4 * r4 * cols + r * cols + c
    out = np.empty(rows * cols, w.dtype)
    out[pos.ravel()] = w.ravel()
    return out


def _patches(a, kh, kw, sh, sw, same):
    """[n][h][w][c] -> [n * out pixels][kh * kw * c]: the taps of every output pixel in OHWI order, zero outside the image (the
    reference skips those taps, nnom_conv2d.c)."""
    n, h, w, c = a.shape
    ph, pw = ((kh - 1) // 2, (kw - 1) // 2) if same else (0, 0)
    oh, ow = nnom_import.out_dim(h, kh, sh, same), nnom_import.out_dim(w, kw, sw, same)
    p = np.zeros((n, (oh - 1) * sh + kh, (ow - 1) * sw + kw, c), np.float64)
    p[:, ph:ph + h, pw:pw + w] = a[:, :p.shape[1] - ph, :p.shape[2] - pw]
    cols = [p[:, ky:ky + (oh - 1) * sh + 1:sh, kx:kx + (ow - 1) * sw + 1:sw] for ky in range(kh) for kx in range(kw)]
    return np.stack(cols, axis=3).reshape(n * oh * ow, kh * kw * c)


def _weights(rng, P, oc, rs, wmax):
    """[oc][K] integer weights for the layer whose input taps are the rows of P: random directions with the taps' mean pattern
    projected out (what every input shares carries no information), scaled so that the accumulators spread over about TARGET << rs
    across the inputs; and the accumulators' mean per output channel."""
    w = rng.normal(0, 1, (oc, P.shape[1]))
    mu = P.mean(axis=0)
    if mu @ mu > 0:
        w -= np.outer(w @ mu / (mu @ mu), mu)
    sd = (P @ w.T).std(axis=0).mean()
    w = np.clip(np.round(w * TARGET * 2.0 ** rs / max(sd, 1e-9)), -wmax, wmax)
    return w.astype(np.int8), (P @ w.T).mean(axis=0)


@functools.lru_cache(maxsize=None)
def _layers(name):
    from oracle import net_ref
    spec = ROWS[name][0]
    shape = spec["shape"]
    rng = np.random.default_rng(sum(map(ord, name)) * 7919)
    h, w, c = shape
    x = inputs(name, 40, h * w * c)
    out = []
    for L in spec["layers"]:
        if L[0] in ("conv", "dense"):
            # this layer's input for 40 inputs of the row's sets, from the layers built so far (oracle/net_ref.py)
            cur = net_ref.run(nnom_import.build_blob(shape, [dict(q) for q in out]), x)["acts"][-1] if out else x
            cur = cur.reshape(len(x), h, w, c).astype(np.float64)
            if L[0] == "conv":
                _, oc, (kh, kw), (sh, sw), same, relu, rs, wmax, bl = L
                P = _patches(cur, kh, kw, sh, sw, same)
            else:
                _, oc, relu, rs, wmax, bl = L
                P = cur.reshape(len(x), -1)
            wt, mean = _weights(rng, P, oc, rs, wmax)
            if bl >= 20:    # rails: the bound, not the spread, picks the requantisation
                b = np.zeros(oc, np.int8)
                b[0], b[1 % oc] = 127, -128
            else:           # the bias centres every output channel, give or take a quarter of the spread
                bl = max(rs - 1, 0)
                b = np.clip(np.round((-mean + rng.normal(0, TARGET / 4 * 2.0 ** rs, oc)) / 2.0 ** bl), -128, 127).astype(np.int8)
            d = dict(w=wt.reshape(-1) if L[0] == "conv" else interleave_dense_opt(wt), b=b, out_rshift=rs, bias_lshift=bl, relu=relu)
            if L[0] == "conv":
                d.update(type=T_CONV, out_ch=oc, kh=kh, kw=kw, sh=sh, sw=sw, same=same)
                h, w, c = nnom_import.out_dim(h, kh, sh, same), nnom_import.out_dim(w, kw, sw, same), oc
            else:
                d.update(type=T_DENSE, out=oc)
                h, w, c = 1, 1, oc
            out.append(d)
        elif L[0] == "pool":
            _, (kh, kw), (sh, sw), same = L
            out.append(dict(type=T_POOL, kh=kh, kw=kw, sh=sh, sw=sw, same=same))
            h, w = nnom_import.out_dim(h, kh, sh, same), nnom_import.out_dim(w, kw, sw, same)
        else:
            out.append(dict(type=T_SOFTMAX))
    return shape, out


def layers(name):
    """Row `name` -> (shape, nnom_import.build_blob layer list) with seeded weights, scaled layer by layer (_weights)."""
    shape, lay = _layers(name)
    return shape, [dict(L) for L in lay]


def blob(name):
    shape, lay = layers(name)
    return nnom_import.build_blob(shape, lay)


def prefixes(name):
    """[(li, blob)]: row `name` cut behind each of its matrix-core layers li (and behind the MaxPool fused into it), so that the layer's
    own output is the logits the batch path returns -- a wrong byte deep in a chain can be washed out by the saturating layers behind
    it before it reaches the row's logits. The cut graph has a plan of its own; tests/test_net_sweep_cpu.py checks that the cuts still
    reach every instance of the 16 x 16 and 32 x 32 tiles over fragments resident in LDS."""
    shape, lay = layers(name)
    out = []
    for li, L in enumerate(lay):
        if L["type"] not in (T_CONV, T_DENSE):
            continue
        end = li + 1
        nxt = lay[li + 1] if li + 1 < len(lay) else None
        if L["type"] == T_CONV and nxt is not None and nxt["type"] == T_POOL and not nxt["same"] and (nxt["kh"], nxt["kw"]) == (nxt["sh"], nxt["sw"]) \
                and nxt["kh"] * nxt["kw"] in (2, 4):
            end = li + 2                                 # a fusable MaxPool stays with its convolution
        out.append((li, nnom_import.build_blob(shape, [dict(x) for x in lay[:end]])))
    return out


SETS = ("noise", "quiet", "zero", "max", "min")


def inputs(name, n, in_n):
    """n inputs [n][in_n] int8 of row `name`: input i from set SETS[i % 5] -- full-range noise, quiet (+-12), all 0, all 127, all -128."""
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.integers(-128, 128, (n, in_n)).astype(np.int8)
    q = rng.integers(-12, 13, (n, in_n)).astype(np.int8)
    k = np.arange(n) % len(SETS)
    x[k == 1] = q[k == 1]
    x[k == 2], x[k == 3], x[k == 4] = 0, 127, -128
    return x


# ---- the kernel's choices, restated ------------------------------------------------------------------------------------------
def epilogue(R):
    """The requantisation form of an MM run: cnn_net_mfma_kernels.hip:605-609 (32 x 32 tiles; the 16 x 16 tiles branch the same
    way, 723-741)."""
    hi, qsh = bool(R.rs & RS_HI), (R.rs & RS_MASK) - 8
    if R.out_c % 4:
        return 4
    if not hi:
        return 0
    return 1 if qsh == 0 else (2 if qsh > 0 else 3)


def tile_shape(R, n_cols):
    """(NW, R, C) of emm_layer_dispatch, cnn_net_mfma_kernels.hip:759-773."""
    nwin, n_ct = R.ph * R.pw, (n_cols + 31) >> 5
    if nwin == 1:
        return (1, 2 if R.n_rt >= 2 else 1, 2 if n_ct >= 2 else 1)
    if nwin == 2:
        return (2, 2, 1) if R.n_rt >= 2 else ((2, 1, 2) if n_ct >= 2 else (2, 1, 1))
    return (4, 1, 1)


def own_mode(R, shape, n_cols):
    """MODE of emm_chain in a graph's own kernel: the a_res / b_res rule of cnn_net_mfma_kernels.hip:481-482 (0: neither)."""
    NW, Rr, C = shape
    n_ct = (n_cols + 31) >> 5
    a_res = R.n_rt <= Rr and n_ct > C and R.n_ks * Rr <= RES_MAX
    b_res = not a_res and R.n_rt > Rr and n_ct <= C and R.n_ks * C * NW <= RES_MAX
    return 2 if a_res else (1 if b_res else 0)


def input_stage(plan, own=False):
    """The input stage of emm_net_body, cnn_net_mfma_kernels.hip:830, 860-936: prefetch, by table, or by division."""
    P, M = plan.P, plan.M
    if M.n_intab >= INTAB_PAD and M.batch <= (4 if own else PB) and 4 <= P.in_n <= 2 * 256:
        return "prefetch"
    return "table" if M.n_intab else "divide"


def _band(n, cuts=(16, 64)):
    return "<=16" if n <= cuts[0] else ("<=64" if n <= cuts[1] else ">64")


def paths(plan, nb):
    """What the general kernel runs for a pass whose per-wave fill is nb (1 .. batch), and what a graph's own kernel runs (its
    tile counts stay those of a full batch: cnn_net_mfma_kernels.hip:1009). dict(batch, frag_mode, input, own_input, out_n (the
    output stage's branch, 1123-1170), runs = one dict per layer)."""
    P, M = plan.P, plan.M
    fl = M.frag_mode == 2                                   # ed_launch_net_mfma: FRAG_LDS = frag_mode == 2 (1225-1226)
    runs = []
    for li, R in enumerate(plan.R):
        d = dict(kind={pe.RUN_SKIP: "SKIP", pe.RUN_MM: "MM", pe.RUN_POOL4: "POOL4", pe.RUN_POOL1: "POOL1", pe.RUN_SOFTMAX: "SOFTMAX"}[R.kind],
                 zero_border=R.zero_border)
        if R.kind == pe.RUN_MM:
            ML = plan.ML[li]
            n_cols, own_cols = nb * R.pix_per_img, M.batch * R.pix_per_img
            if R.small:                                     # 751-757
                U = 4 if R.n_rt >= 3 else (2 if R.n_rt == 2 else 1)
                d.update(tile=("small", U), own_tile=("small", U), own_mode=None)
            else:
                d.update(tile=("tiles",) + tile_shape(R, n_cols), own_tile=("tiles",) + tile_shape(R, own_cols))
                d["own_mode"] = own_mode(R, tile_shape(R, own_cols), own_cols)
            d.update(n_rt=R.n_rt, n_ct=(n_cols + 31) >> 5, frag_lds=fl, epilogue=epilogue(R), form="toeplitz" if ML.toep else ("expand" if R.expand else "direct"),
                     xtab=(R.xtab_off >= 0) if R.expand else None, coltab=R.col_off >= 0, relu=R.lo_clamp == 0)
        elif R.kind == pe.RUN_SOFTMAX:
            d["band"] = _band(R.in_n)                       # 1076-1116
        runs.append(d)
    return dict(batch=M.batch, frag_mode=M.frag_mode, input=input_stage(plan), own_input=input_stage(plan, own=True),
                out_n=_band(P.out_n), runs=runs)


def items(plan, nb):
    """paths(plan, nb) as a set of coverage items."""
    p = paths(plan, nb)
    fl = p["frag_mode"] == 2
    out = {("batch", p["batch"]), ("frag_mode", p["frag_mode"]), ("input", p["input"]), ("own_input", p["own_input"]), ("out_n", p["out_n"])}
    if nb < p["batch"]:
        out.add(("ragged",))
    for d in p["runs"]:
        out.add(("run", d["kind"]))
        if d["kind"] == "SKIP":
            continue
        out.add(("zero_border", d["kind"], d["zero_border"]))
        if d["kind"] == "SOFTMAX":
            out.add(("softmax", d["band"]))
        if d["kind"] != "MM":
            continue
        out.add(d["tile"] + (fl, d["epilogue"]))
        out.add(("relu", d["tile"][0], "hi" if d["epilogue"] in (1, 2, 3) else "plain", d["relu"]))   # the lower clamp of either packing
        out.add(("form", d["form"]))
        if d["xtab"] is not None:
            out.add(("xtab", d["xtab"]))
        out.add(("coltab", d["tile"][0], d["coltab"]))
        if d["own_mode"] is not None:
            out.add(("own", d["own_mode"], fl))
        if d["tile"][0] == "tiles" and d["n_rt"] % 2 and d["tile"][2] == 2 and d["n_rt"] > 1:
            out.add(("remainder", "row tiles"))          # the last group of row tiles has a spare slot (545)
        if d["tile"][0] == "tiles" and d["n_ct"] % 2 and d["tile"][3] == 2 and d["n_ct"] > 1:
            out.add(("remainder", "column tiles"))       # the last group of column tiles has a spare slot (505)
        if d["own_tile"] != d["tile"]:
            out.add(("own_tile_differs",))
    return out


def plan_items(plan):
    """The union of items() over every per-wave fill 1 .. batch."""
    return set().union(*(items(plan, nb) for nb in range(1, plan.M.batch + 1)))


def full_set():
    """Every item a graph could reach: the product of the kernel's choices."""
    s = set()
    for fl in (False, True):
        s |= {("tiles",) + t + (fl, e) for t in TILE_SHAPES for e in EPILOGUES}
        s |= {("small", u, fl, e) for u in SMALL_UNITS for e in EPILOGUES}
        s |= {("own", m, fl) for m in (0, 1, 2)}
    s |= {("batch", b) for b in (1, 2, 4)} | {("frag_mode", m) for m in (0, 2)} | {("ragged",), ("own_tile_differs",)}
    s |= {("input", k) for k in ("prefetch", "table", "divide")} | {("own_input", k) for k in ("prefetch", "table", "divide")}
    s |= {("out_n", b) for b in ("<=16", "<=64", ">64")} | {("softmax", b) for b in ("<=16", "<=64", ">64")}
    s |= {("run", k) for k in ("SKIP", "MM", "POOL4", "POOL1", "SOFTMAX")}
    s |= {("zero_border", k, z) for k in ("MM", "POOL4", "POOL1", "SOFTMAX") for z in (0, 1)}
    s |= {("relu", t, k, r) for t in ("tiles", "small") for k in ("hi", "plain") for r in (False, True)}
    s |= {("form", f) for f in ("toeplitz", "expand", "direct")} | {("xtab", v) for v in (False, True)}
    s |= {("coltab", t, v) for t in ("tiles", "small") for v in (False, True)}
    s |= {("accelerated", 0), ("remainder", "row tiles"), ("remainder", "column tiles")}
    return s


# item -> why no legal plan produces it (derived from the planner, model_net_mm.c)
EXCLUDED = {
    ("zero_border", "SOFTMAX", 1): "a Softmax writes the compact input of its consumer or the compact last output: never a padded layout",
}


def claims(note):
    return {k: int(v) for k, v in (t.split("=") for t in note.split(";")[0].split())}

"""Quantise a float32 X-CUBE-AI network (``.ednf``, cube_import.read_blob) to an int8 NNoM graph (``.ednn``, nnom_import.build_blob)
from calibration statistics: the step the reference takes with ``generate_model(model, x, name=.../weights.h)`` (kws_nnom.py:305),
whose implementation (nnom_utils.py) it never vendored. This module restates NNoM's published power-of-two rule; byte parity with
that generator cannot be pinned. Pure Python: the statistics come from the GPU calibrator
(``Context.calibrator``, edison_fcal_*) or from any host restatement of it.

Statistics (``stats``): for index 0 = the network input and index i = conv / dense record i - 1 of the float network,
  absmax uint32 [n + 1]       the largest bit pattern of fabsf(v): v the input floats, or acc + bias in f32 before ReLU and pool
  hist   uint64 [n + 1][256]  counts of v by biased exponent field (bits >> 23) & 0xff
  count  uint64 [n + 1]       values seen

The rule. A tensor whose largest magnitude is a gets int_bits = ceil(log2(a)) and dec = 7 - int_bits fractional bits;
q = clip(round_half_even(x 2^dec), -128, 127). With method "saturate", an activation's int_bits is instead the smallest k that leaves
at most saturate x count values at or above 2^k (counted by exponent: sum(hist[e >= k + 127])), the intent kws_nnom.py:228-229 states.
A layer reads its predecessor's output format (ReLU, MaxPool and Flatten inherit it), and the shifts are the macros of the
reference's header (weights.h:72-105): OUTPUT_RSHIFT = in_dec + w_dec - out_dec, BIAS_LSHIFT = in_dec + w_dec - b_dec. The bias dec is
clamped to in_dec + w_dec so that its shift is not negative; an all-zero bias gets exactly that. An all-zero weight tensor gets dec 7.

Padded records (``.ednf`` version 2). NNoM has one flag per layer, PADDING_SAME, and NNoM 0.3.0 computes with
it: output ceil(in / stride) and a leading pad of (k - 1) // 2 on both axes, taps outside the image zero (a max pool: absent). A padded
conv or pool maps to that flag only where the record computes the same thing on both axes at once (``nnom_same``); anything else
raises a QuantizeError naming the layer and both pad sets: NNoM cannot express it.
"""
import math

import numpy as np

from . import cube_import, nnom_import

METHODS = ("max_min", "saturate")
MAX_SHIFT = 31   # the int8 kernels and NNoM shift 32-bit accumulators


class QuantizeError(ValueError):
    pass


# ---- formats ----------------------------------------------------------------------------------------------------------------------
def int_bits_of(absmax):
    """ceil(log2(absmax)) for a finite absmax > 0, exactly (no logarithm: 1.0 gives 0, the next float above gives 1)."""
    m, e = math.frexp(float(absmax))     # absmax = m 2^e, 0.5 <= m < 1
    return e - 1 if m == 0.5 else e


def dec_bits_of(absmax):
    return 7 - int_bits_of(absmax)


def int_bits_saturate(hist, count, saturate):
    """The smallest k with sum(hist[e >= k + 127]) <= saturate * count."""
    hist = [int(v) for v in hist]
    tail, limit = 0, float(saturate) * int(count)
    k = 129                              # e >= 256: nothing
    for e in range(255, -1, -1):
        if tail + hist[e] > limit:
            break
        tail += hist[e]
        k = e - 127
    return k


def quantize_tensor(x, dec):
    """q = clip(round_half_even(x 2^dec), -128, 127) as int8, and the RMS of q 2^-dec - x."""
    x = np.asarray(x, np.float64)
    q = np.clip(np.rint(np.ldexp(x, int(dec))), -128, 127)
    rms = float(np.sqrt(np.mean((np.ldexp(q, -int(dec)) - x) ** 2))) if x.size else 0.0
    return q.astype(np.int8), rms


def quantize_input(x, in_dec):
    """Network inputs (float32, as the float network takes them) -> the int8 inputs of the quantised graph."""
    return quantize_tensor(np.asarray(x, np.float32), in_dec)[0]


def shifts(in_dec, w_dec, b_dec, out_dec):
    """(BIAS_LSHIFT, OUTPUT_RSHIFT) of a layer, the derived macros of the reference's header."""
    return in_dec + w_dec - b_dec, in_dec + w_dec - out_dec


def _f32_from_bits(bits):
    return float(np.array([int(bits)], np.uint32).view(np.float32)[0])


def _act_dec(name, absmax_bits, hist, count, method, saturate):
    """dec bits of an activation from its statistic, or a QuantizeError naming it."""
    if int(count) == 0:
        raise QuantizeError("%s: no values were calibrated (count == 0)" % name)
    bits = int(absmax_bits)
    if (bits >> 23) & 0xff == 0xff or int(hist[255]) != 0:
        raise QuantizeError("%s: the calibration saw an Inf or NaN" % name)
    if bits == 0:
        raise QuantizeError("%s: every calibrated value is zero" % name)
    if method == "saturate":
        return 7 - int_bits_saturate(hist, count, saturate)
    return dec_bits_of(_f32_from_bits(bits))


# ---- the graph --------------------------------------------------------------------------------------------------------------------
def nnom_same(name, what, in_hw, k, s, pads, out_hw):
    """0 for a window without pads (PADDING_VALID), 1 where NNoM 0.3.0's PADDING_SAME computes what pads = (top, left, bottom, right)
    do: on both axes out = ceil(in / s) and the leading pad is (k - 1) // 2. A QuantizeError naming the layer otherwise."""
    if not any(pads):
        return 0
    nnom = tuple((k[a] - 1) // 2 for a in (0, 1))
    ok = all(out_hw[a] == -(-in_hw[a] // s[a]) and pads[a] == nnom[a] for a in (0, 1))
    if not ok:
        raise QuantizeError("%s: its %s pads (top, left, bottom, right) = %s over %dx%d, window %dx%d, stride %dx%d give %dx%d; NNoM's PADDING_SAME "
                            "pads (top, left) = %s and gives %dx%d: NNoM cannot express this layer"
                            % (name, what, tuple(pads), in_hw[0], in_hw[1], k[0], k[1], s[0], s[1], out_hw[0], out_hw[1], nnom,
                               -(-in_hw[0] // s[0]), -(-in_hw[1] // s[1])))
    return 1


def layer_names(model):
    """NNoM's names for the float network's conv records: conv2d_i, or dense_j for a record whose kernel covers its whole input."""
    names, nc, nd = [], 0, 0
    for L in model["layers"]:
        if L["type"] != cube_import.T_CONV:
            continue
        if tuple(L["k"]) == tuple(L["inp"][:2]) and not any(L.get("cpad", ())):
            nd += 1
            names.append("dense_%d" % nd)
        else:
            nc += 1
            names.append("conv2d_%d" % nc)
    return names


def assemble(in_shape, in_dec, layers):
    """The .ednn blob of a sequential graph given integer tensors and dec bits. layers: nnom_import layer dicts (type, kh, kw, sh, sw,
    same, out_ch / out, relu, w, b int8) where a conv / dense carries w_dec, b_dec and out_dec in place of its shifts and a dense
    matrix is plain row-major [out][in]; pools and the softmax pass the format on."""
    out, dec = [], int(in_dec)
    for L in layers:
        L = dict(L)
        if L["type"] in (nnom_import.T_CONV, nnom_import.T_DENSE):
            L["bias_lshift"], L["out_rshift"] = shifts(dec, L["w_dec"], L["b_dec"], L["out_dec"])
            dec = L["out_dec"]
        elif L["type"] not in (nnom_import.T_POOL, nnom_import.T_SOFTMAX):
            raise QuantizeError("layer type %d is not part of a quantised sequential graph" % L["type"])
        out.append(L)
    return nnom_import.build_blob(tuple(in_shape), out, dense_plain=True)


def quantize(model, stats, method="max_min", saturate=0.0, scale=1.0):
    """model: cube_import.read_blob's dict; stats: dict(absmax, hist, count) as above. Returns (ednn_blob, report). report: method,
    saturate, in_shape, input = dict(dec, absmax), layers = [dict(name, kind, absmax, w_dec, b_dec, b_clamped, out_dec, bias_lshift,
    out_rshift, w_rms, b_rms)], net_input_scale = scale 2^in_dec (scale: what the float flow multiplies its features by; the int8 graph's
    features are round(feature x net_input_scale)), graph = the layer list assemble() and write_weights_h() take."""
    if method not in METHODS:
        raise QuantizeError("method must be one of %s (NNoM's KLD method is not built)" % (METHODS,))
    if not 0.0 <= float(saturate) < 1.0:
        raise QuantizeError("saturate must be in [0, 1)")
    recs = [L for L in model["layers"] if L["type"] == cube_import.T_CONV]
    names = layer_names(model)
    absmax, hist, count = (np.asarray(stats[k]) for k in ("absmax", "hist", "count"))
    if absmax.shape != (len(recs) + 1,) or hist.shape != (len(recs) + 1, 256) or count.shape != (len(recs) + 1,):
        raise QuantizeError("the statistics are not those of this network (%d conv / dense records)" % len(recs))
    in_dec = _act_dec("input", absmax[0], hist[0], count[0], method, saturate)
    rep_layers, graph, dec = [], [], in_dec
    for i, (L, name) in enumerate(zip(recs, names)):
        out_dec = _act_dec(name, absmax[i + 1], hist[i + 1], count[i + 1], method, saturate)
        w = np.asarray(L["w"], np.float32)
        b = np.asarray(L["b"], np.float32)
        if not (np.isfinite(w).all() and np.isfinite(b).all()):
            raise QuantizeError("%s: a weight or bias is Inf or NaN" % name)
        wmax, bmax = float(np.abs(w).max()), float(np.abs(b).max())
        w_dec = dec_bits_of(wmax) if wmax > 0 else 7
        b_free = dec_bits_of(bmax) if bmax > 0 else dec + w_dec
        b_dec = min(b_free, dec + w_dec)
        bl, rs = shifts(dec, w_dec, b_dec, out_dec)
        if rs < 0:
            raise QuantizeError("%s: OUTPUT_RSHIFT = %d + %d - %d is negative: the output format is finer than input x weights" % (name, dec, w_dec, out_dec))
        if rs > MAX_SHIFT or bl > MAX_SHIFT:
            raise QuantizeError("%s: a shift above %d (OUTPUT_RSHIFT %d, BIAS_LSHIFT %d)" % (name, MAX_SHIFT, rs, bl))
        wq, w_rms = quantize_tensor(w, w_dec)
        bq, b_rms = quantize_tensor(b, b_dec)
        oc, (kh, kw), (sh, sw), (ph, pw) = L["out"][2], L["k"], L["s"], L["p"]
        dense = name.startswith("dense")
        cpad, ppad = tuple(L.get("cpad", (0, 0, 0, 0))), tuple(L.get("ppad", (0, 0, 0, 0)))
        ih, iw = L["inp"][:2]
        ch, cw = (ih + cpad[0] + cpad[2] - kh) // sh + 1, (iw + cpad[1] + cpad[3] - kw) // sw + 1      # the conv's map, before the pool
        conv_same = nnom_same(name, "conv", (ih, iw), (kh, kw), (sh, sw), cpad, (ch, cw))
        pool_same = nnom_same(name, "pool", (ch, cw), (ph, pw), (ph, pw), ppad, L["out"][:2])
        if dense:
            graph.append(dict(type=nnom_import.T_DENSE, out=oc, w=wq.reshape(oc, -1), b=bq, relu=int(L["relu"]), w_dec=w_dec, b_dec=b_dec, out_dec=out_dec))
        else:
            graph.append(dict(type=nnom_import.T_CONV, out_ch=oc, kh=kh, kw=kw, sh=sh, sw=sw, same=conv_same, w=wq.reshape(-1), b=bq, relu=int(L["relu"]),
                              w_dec=w_dec, b_dec=b_dec, out_dec=out_dec))
            if (ph, pw) != (1, 1):
                graph.append(dict(type=nnom_import.T_POOL, kh=ph, kw=pw, sh=ph, sw=pw, same=pool_same))
        rep_layers.append(dict(name=name, kind="dense" if dense else "conv2d", absmax=_f32_from_bits(absmax[i + 1]), w_dec=w_dec, b_dec=b_dec,
                               b_clamped=b_dec != b_free, out_dec=out_dec, bias_lshift=bl, out_rshift=rs, w_rms=w_rms, b_rms=b_rms))
        dec = out_dec
    if model["layers"][-1]["type"] == cube_import.T_SOFTMAX:
        graph.append(dict(type=nnom_import.T_SOFTMAX))
    blob = assemble(model["in_shape"], in_dec, graph)
    report = dict(method=method, saturate=float(saturate), in_shape=tuple(model["in_shape"]), input=dict(dec=in_dec, absmax=_f32_from_bits(absmax[0])),
                  layers=rep_layers, net_input_scale=float(scale) * 2.0 ** in_dec, graph=graph)
    return blob, report


def format_report(report):
    lines = ["method %s%s" % (report["method"], " (saturate %g)" % report["saturate"] if report["method"] == "saturate" else ""),
             "input      dec %3d   absmax %-12g net_input_scale %g" % (report["input"]["dec"], report["input"]["absmax"], report["net_input_scale"]),
             "layer      w_dec b_dec out_dec  bias_lshift out_rshift  absmax        w_rms      b_rms"]
    for L in report["layers"]:
        lines.append("%-10s %5d %5d%s %6d  %11d %10d  %-12g  %-9.3g  %-9.3g" % (L["name"], L["w_dec"], L["b_dec"], "*" if L["b_clamped"] else " ", L["out_dec"],
                                                                                  L["bias_lshift"], L["out_rshift"], L["absmax"], L["w_rms"], L["b_rms"]))
    if any(L["b_clamped"] for L in report["layers"]):
        lines.append("(* bias dec clamped to in_dec + w_dec)")
    return "\n".join(lines)


# ---- the header, for the firmware ------------------------------------------------------------------------------------------------
def interleave_dense_opt(w):
    """Plain [rows][cols] -> arm_fully_connected_q7_opt's storage order, the inverse of nnom_import.deinterleave_dense_opt."""
    w = np.asarray(w, np.int8)
    rows, cols = w.shape
    blk = [(0, 0), (1, 0), (0, 2), (1, 2), (2, 0), (3, 0), (2, 2), (3, 2), (0, 1), (1, 1), (0, 3), (1, 3), (2, 1), (3, 1), (2, 3), (3, 3)]
    out = []
    for r in range(0, rows - rows % 4, 4):
        for c in range(0, cols - cols % 4, 4):
            out += [w[r + dr, c + dc] for dr, dc in blk]
        for c in range(cols - cols % 4, cols):
            out += [w[r + dr, c] for dr in range(4)]
    for r in range(rows - rows % 4, rows):
        out += list(w[r, :])
    return np.array(out, np.int8)


def _c_array(a):
    return "{" + ", ".join(str(int(v)) for v in np.asarray(a).reshape(-1)) + "}"


def _paren(v):
    return "(%d)" % v


def write_weights_h(layers, in_shape, in_dec):
    """The NNoM model header of a quantised sequential graph (report["graph"], report["in_shape"], report["input"]["dec"]), in the
    shape of the reference's weights.h: *_KERNEL_0 / *_BIAS_0 arrays with their *_SHIFT dec bits, every layer's *_OUTPUT_SHIFT, the
    derived *_OUTPUT_RSHIFT / *_BIAS_LSHIFT macros with their #error guards, nnom_model_create() and NNOM_INPUT_*. Dense matrices are
    written in arm_fully_connected_q7_opt's order (DENSE_WEIGHT_OPT 1, nnom_port.h:34), as the firmware reads them. NNOM_INPUT_SCALE is the
    divisor 2^-in_dec the firmware applies to its features (app.c:685-693) when in_dec <= 0, else 1."""
    named, nc, nd, npool = [], 0, 0, 0
    for L in layers:
        if L["type"] == nnom_import.T_CONV:
            nc += 1
            named.append(("conv2d_%d" % nc, L))
        elif L["type"] == nnom_import.T_DENSE:
            nd += 1
            named.append(("dense_%d" % nd, L))
        elif L["type"] == nnom_import.T_POOL:
            npool += 1
            named.append(("max_pooling2d_%d" % npool, L))
        elif L["type"] == nnom_import.T_SOFTMAX:
            named.append(("softmax_1", L))
        else:
            raise QuantizeError("layer type %d cannot be written" % L["type"])
    o = ['#include "nnom.h"', ""]
    for name, L in named:
        if "w" not in L:
            continue
        U = name.upper()
        w = interleave_dense_opt(L["w"]) if L["type"] == nnom_import.T_DENSE else L["w"]
        o += ["#define %s_KERNEL_0 %s" % (U, _c_array(w)), "", "#define %s_KERNEL_0_SHIFT %s" % (U, _paren(L["w_dec"])), "",
              "#define %s_BIAS_0 %s" % (U, _c_array(L["b"])), "", "#define %s_BIAS_0_SHIFT %s" % (U, _paren(L["b_dec"])), "", ""]
    o += ["", "/* output enconding for each layer */", "#define INPUT_1_OUTPUT_SHIFT %s" % _paren(in_dec)]
    dec, prev_of = in_dec, {}
    prev = "INPUT_1"
    for name, L in named:
        U = name.upper()
        if "w" in L:
            prev_of[name] = prev
            dec = L["out_dec"]
        o.append("#define %s_OUTPUT_SHIFT %s" % (U, _paren(7 if L["type"] == nnom_import.T_SOFTMAX else dec)))
        prev = U
    o += ["", "/* bias shift and output shift for each layer */"]
    for name, L in named:
        if "w" not in L:
            continue
        U, P = name.upper(), prev_of[name]
        o += ["#define %s_OUTPUT_RSHIFT (%s_OUTPUT_SHIFT+%s_KERNEL_0_SHIFT-%s_OUTPUT_SHIFT)" % (U, P, U, U),
              "#define %s_BIAS_LSHIFT   (%s_OUTPUT_SHIFT+%s_KERNEL_0_SHIFT-%s_BIAS_0_SHIFT)" % (U, P, U, U),
              "#if %s_OUTPUT_RSHIFT < 0" % U, "#error %s_OUTPUT_RSHIFT must be bigger than 0" % U, "#endif",
              "#if %s_BIAS_LSHIFT < 0" % U, "#error %s_BIAS_RSHIFT must be bigger than 0" % U, "#endif"]
    o += ["", "/* weights for each layer */"]
    for name, L in named:
        if "w" not in L:
            continue
        U = name.upper()
        o += ["static const int8_t %s_weights[] = %s_KERNEL_0;" % (name, U),
              "static const nnom_weight_t %s_w = { (const void*)%s_weights, %s_OUTPUT_RSHIFT};" % (name, name, U),
              "static const int8_t %s_bias[] = %s_BIAS_0;" % (name, U),
              "static const nnom_bias_t %s_b = { (const void*)%s_bias, %s_BIAS_LSHIFT};" % (name, name, U)]
    h, w_, c = in_shape
    body, k = ["\tlayer[0] = Input(shape(%d, %d, %d), nnom_input_data);" % (h, w_, c)], 0
    for name, L in named:
        k += 1
        if L["type"] == nnom_import.T_CONV:
            oh, ow = nnom_import.out_dim(h, L["kh"], L["sh"], L["same"]), nnom_import.out_dim(w_, L["kw"], L["sw"], L["same"])
            body.append("\tlayer[%d] = model.hook(Conv2D(%d, kernel(%d, %d), stride(%d, %d), %s, &%s_w, &%s_b), layer[%d]);"
                        % (k, L["out_ch"], L["kh"], L["kw"], L["sh"], L["sw"], "PADDING_SAME" if L["same"] else "PADDING_VALID", name, name, k - 1))
            h, w_, c = oh, ow, L["out_ch"]
        elif L["type"] == nnom_import.T_DENSE:
            body.append("\tlayer[%d] = model.hook(Dense(%d, &%s_w, &%s_b), layer[%d]);" % (k, L["out"], name, name, k - 1))
            h, w_, c = 1, 1, L["out"]
        elif L["type"] == nnom_import.T_POOL:
            body.append("\tlayer[%d] = model.hook(MaxPool(kernel(%d, %d), stride(%d, %d), %s), layer[%d]);"
                        % (k, L["kh"], L["kw"], L["sh"], L["sw"], "PADDING_SAME" if L["same"] else "PADDING_VALID", k - 1))
            h, w_ = nnom_import.out_dim(h, L["kh"], L["sh"], L["same"]), nnom_import.out_dim(w_, L["kw"], L["sw"], L["same"])
        else:
            body.append("\tlayer[%d] = model.hook(Softmax(), layer[%d]);" % (k, k - 1))
        if L.get("relu"):
            k += 1
            body.append("\tlayer[%d] = model.active(act_relu(), layer[%d]);" % (k, k - 1))
    k += 1
    n_out = h * w_ * c
    body.append("\tlayer[%d] = model.hook(Output(shape(%d,1,1), nnom_output_data), layer[%d]);" % (k, n_out, k - 1))
    o += ["", "/* nnom model */", "static int8_t nnom_input_data[%d];" % (in_shape[0] * in_shape[1] * in_shape[2]),
          "static int8_t nnom_output_data[%d];" % n_out, "static nnom_model_t* nnom_model_create(void)", "{", "\tstatic nnom_model_t model;",
          "\tnnom_layer_t* layer[%d];" % (k + 1), "", "\tnew_model(&model);", ""] + body
    o += ["\tmodel_compile(&model, layer[0], layer[%d]);" % k, "\treturn &model;", "}",
          "#define NNOM_INPUT_SCALE %d" % (2 ** -in_dec if in_dec <= 0 else 1), "#define NNOM_INPUT_MIN -128", "#define NNOM_INPUT_MAX 127", ""]
    return "\n".join(o)

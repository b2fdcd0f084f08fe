"""Padded float32 networks ('same' convolutions and pools, .ednf version 2): the float64 restatement with pads,
the bit-exact host model of the kernel's padded path, the restated version-2 plan (parse() in csrc/edison_fnet.hip), the sweep rows and
the blobs the loader must refuse. Test infrastructure, not a test: tests/test_fnet_pad_cpu.py holds the restatement to torch's float64
conv2d / max_pool2d and the exact model to the restatement; tests/test_gpu_fnet_pad.py holds the kernels to the exact model bit for bit.

Semantics (Keras / TensorFlow's). Conv pads (top, left, bottom, right): out = (in + before + after - k) // stride + 1; a tap outside
the image is the operand +0.0f and stays in the k-ordered fmaf chain (tests/fnet_exact.py), which is therefore as long as without
pads. Pool pads, window = stride: pooled = (conv + before + after - p) // p + 1; an element of a window outside the conv's map is
absent: it takes no part in the max (identity -inf, never 0).

The two models are written differently from the kernel on purpose: both work on a zero-bordered (for the pool: -inf-bordered) copy of
the image, the kernel on the dense image with a predicate per tap.

A row is (spec, note). spec: in_shape; layers, each ("conv", out_c, (kh, kw), (sh, sw), (ph, pw), relu, cpad, ppad) or ("dense", n,
relu), a softmax follows; or zoo: one of kws_keras.get_model's padded architectures, written in X-CUBE-AI's source format
(cube_sources) and imported; bias: a constant; positive: |weights|; sets: fnet_sweep's input sets."""
import struct

import numpy as np

from edison_amd import cube_import

import cube_synth
import fnet_exact as fe
import fnet_sweep as fs

Z4 = (0, 0, 0, 0)


def pads(L):
    return tuple(L.get("cpad", Z4)), tuple(L.get("ppad", Z4))


def conv_map(L):
    """(conv_h, conv_w) of record L: its map before the pool."""
    (ih, iw, _), (kh, kw), (sh, sw), (c, _) = L["inp"], L["k"], L["s"], pads(L)
    return (ih + c[0] + c[2] - kh) // sh + 1, (iw + c[1] + c[3] - kw) // sw + 1


def out_hw(inp_hw, k, s, p, cpad, ppad):
    ch, cw = (inp_hw[0] + cpad[0] + cpad[2] - k[0]) // s[0] + 1, (inp_hw[1] + cpad[1] + cpad[3] - k[1]) // s[1] + 1
    return cube_import.pooled_dim(ch, ppad[0], ppad[2], p[0]), cube_import.pooled_dim(cw, ppad[1], ppad[3], p[1])


# ---- float64 restatement ------------------------------------------------------------------------------------------------------------
def _pool(y, L, fill):
    (ph, pw), (_, q) = L["p"], pads(L)
    Ph, Pw = L["out"][:2]
    y = np.pad(y, ((0, 0), (q[0], q[2]), (q[1], q[3]), (0, 0)), constant_values=fill)
    n, oc = y.shape[0], y.shape[3]
    return y[:, :Ph * ph, :Pw * pw].reshape(n, Ph, ph, Pw, pw, oc).max(axis=(2, 4))


def conv_layer(L, x):
    """One conv / dense record on x [n][in_h][in_w][in_c] float64 -> (y [n][out_h][out_w][out_c], S [n][conv_h][conv_w][out_c]: the
    bound scale sum |a| |w| + |bias| of every real conv output; a padded tap adds nothing to it)."""
    x = np.asarray(x, np.float64)
    (kh, kw), (sh, sw), (c, _) = L["k"], L["s"], pads(L)
    xp = np.pad(x, ((0, 0), (c[0], c[2]), (c[1], c[3]), (0, 0)))
    win = np.lib.stride_tricks.sliding_window_view(xp, (kh, kw), axis=(1, 2))[:, ::sh, ::sw]   # [n][ch][cw][c][kh][kw]
    n, ch, cw = win.shape[:3]
    assert (ch, cw) == conv_map(L)
    cols = win.transpose(0, 1, 2, 4, 5, 3).reshape(n, ch, cw, -1)
    w = L["w"].astype(np.float64).reshape(L["w"].shape[0], -1)
    b = L["b"].astype(np.float64)
    y = cols @ w.T + b
    S = np.abs(cols) @ np.abs(w).T + np.abs(b)
    if L["relu"]:
        y = np.maximum(y, 0.0)
    return _pool(y, L, -np.inf), S


def layer_from(model, i, a_in):
    """Conv record i on a given flat input -> (y flat float64, the largest S of each output's real window elements)."""
    L = fe.conv_records(model)[i]
    y, S = conv_layer(L, np.asarray(a_in, np.float64).reshape((-1,) + tuple(L["inp"])))
    return y.reshape(y.shape[0], -1), _pool(S, L, 0.0).reshape(S.shape[0], -1)


def run64(model, x):
    """Every conv record's output [n][out_n] float64, each fed the previous one."""
    a, out = np.asarray(x, np.float64), []
    for i in range(len(fe.conv_records(model))):
        a = layer_from(model, i, a)[0]
        out.append(a)
    return out


# ---- the bit-exact host model -------------------------------------------------------------------------------------------------------
def gather(L, x):
    """The kernel's A operand of record L for inputs x [n][in_n]: ([n * rows][K] float32 with +0.0f at the padded taps, rows in the
    kernel's order, and live [rows]: False for the absent elements of a pool window, whose A row is not used)."""
    (ih, iw, ic), (kh, kw), (sh, sw), (ph, pw), (c, q) = L["inp"], L["k"], L["s"], L["p"], pads(L)
    Ph, Pw = L["out"][:2]
    ch, cw = conv_map(L)
    x = np.asarray(x, np.float32).reshape(-1, ih, iw, ic)
    xp = np.zeros((x.shape[0], ih + c[0] + c[2], iw + c[1] + c[3], ic), np.float32)
    xp[:, c[0]:c[0] + ih, c[1]:c[1] + iw] = x
    Wp = xp.shape[2]
    k = np.arange(kh * kw * ic)
    ci, t = k % ic, k // ic
    koff = ((t // kw) * Wp + t % kw) * ic + ci
    qq, e = np.divmod(np.arange(Ph * Pw * ph * pw), ph * pw)
    py, px = np.divmod(qq, Pw)
    ey, ex = np.divmod(e, pw)
    cy, cx = py * ph + ey - q[0], px * pw + ex - q[1]
    live = (cy >= 0) & (cy < ch) & (cx >= 0) & (cx < cw)
    rowin = np.where(live, (cy * sh * Wp + cx * sw) * ic, 0)
    return xp.reshape(x.shape[0], -1)[:, rowin[:, None] + koff[None, :]].reshape(-1, kh * kw * ic), live


def pre_activation(L, x, variant=None):
    """acc + bias (f32) of every row, and live tiled over the utterances: ([n * rows][out_c] float32, [n * rows] bool)."""
    oc = L["out"][2]
    A, live = gather(L, x)
    v = fe.chain(A, L["w"].reshape(oc, -1).T, variant) + L["b"].astype(np.float32)[None, :]
    return v.astype(np.float32), np.tile(live, A.shape[0] // live.size)


def layer(L, x, variant=None, absent=-np.inf):
    """Record L on x [n][in_n] float32 -> [n][out_n] float32 as the kernel writes it. `absent`: the value an absent element takes
    in the max; anything but -inf is a wrong kernel (the CPU test uses 0 to show what it changes)."""
    oc, P = L["out"][2], L["p"][0] * L["p"][1]
    v, live = pre_activation(L, x, variant)
    if L["relu"]:
        v = np.maximum(v, np.float32(0))
    v = np.where(live[:, None], v, np.float32(absent))
    return v.reshape(-1, P, oc).max(axis=1).reshape(-1, int(np.prod(L["out"]))).astype(np.float32)


def run(model, x):
    out, a = [], np.asarray(x, np.float32)
    for L in fe.conv_records(model):
        a = layer(L, a)
        out.append(a)
    return out


def layers_from(model, x, acts):
    """fnet_exact.layers_from with the padded layer model."""
    want, got, off, prev = [], [], 0, np.asarray(x, np.float32)
    for L in fe.conv_records(model):
        n_out = int(np.prod(L["out"]))
        want.append(layer(L, prev))
        got.append(np.asarray(acts[:, off:off + n_out], np.float32))
        prev, off = got[-1], off + n_out
    assert off == acts.shape[1]
    return want, got


# ---- the plan: parse() restated for versions 1 and 2 --------------------------------------------------------------------------------
def plan(blob):
    """fnet_exact.plan for a version 1 or 2 blob; every layer also carries pad, cpad, ppad, live (rows that are not absent) and kn
    (ints of its k tables in LDS). The checks run in parse()'s order."""
    E_SIZE, E_NO_IMPL = fe.E_SIZE, fe.E_NO_IMPL
    if len(blob) < 32 or blob[:4] != b"EDNF":
        return dict(error=E_SIZE)
    ver, nl, in_h, in_w, in_c, n_out, kwb = struct.unpack_from("<7i", blob, 4)
    if ver not in (1, 2):
        return dict(error=E_NO_IMPL)
    ri = 16 if ver == 1 else 24
    if nl < 2 or nl > fe.MAX_LAYERS + 1:
        return dict(error=E_NO_IMPL)
    if min(in_h, in_w, in_c) < 1 or max(in_h, in_w, in_c) > fe.MAX_DIM or kwb < 0 or kwb % 4:
        return dict(error=E_SIZE)
    if in_h * in_w * in_c > 1 << 20:
        return dict(error=E_NO_IMPL)
    off = 32 + nl * ri * 4
    if off + kwb > len(blob):
        return dict(error=E_SIZE)
    off += kwb
    h, w, c = in_h, in_w, in_c
    wfl = tabn = acts = 0
    buf = [h * w * c, 0]
    layers, w_lds, k_lds = [], 0, 0
    for i in range(nl):
        v = list(struct.unpack_from("<%di" % ri, blob, 32 + 4 * ri * i)) + [0] * (24 - ri)
        if v[0] not in (cube_import.T_CONV, cube_import.T_SOFTMAX):
            return dict(error=E_NO_IMPL)
        for j in range(1, (15 if v[0] == cube_import.T_CONV else 6) + 1):
            if v[j] < (0 if j == 11 else 1) or v[j] > fe.MAX_DIM * (16 if j >= 14 else 1):
                return dict(error=E_SIZE)
        if v[0] == cube_import.T_CONV and (min(v[16:24]) < 0 or max(v[16:24]) > fe.MAX_DIM):
            return dict(error=E_SIZE)
        cur = h * w * c
        if v[1] * v[2] * v[3] != cur:
            return dict(error=E_SIZE)
        if v[0] == cube_import.T_SOFTMAX:
            if i != nl - 1:
                return dict(error=E_NO_IMPL)
            if v[4] * v[5] * v[6] != cur:
                return dict(error=E_SIZE)
            continue
        if i == nl - 1:
            return dict(error=E_NO_IMPL)
        ih, iw, ic, kh, kw, sh, sw, ph, pw = v[1], v[2], v[3], v[7], v[8], v[9], v[10], v[12], v[13]
        (pt, pl, pb, pr), (qt, ql, qb, qr) = v[16:20], v[20:24]
        if max(pt, pb) >= kh or max(pl, pr) >= kw:
            return dict(error=E_NO_IMPL)
        if max(qt, qb) >= ph or max(ql, qr) >= pw:
            return dict(error=E_NO_IMPL)
        if kh > ih + pt + pb or kw > iw + pl + pr:
            return dict(error=E_SIZE)
        oh, ow = (ih + pt + pb - kh) // sh + 1, (iw + pl + pr - kw) // sw + 1
        Ph, Pw = cube_import.pooled_dim(oh, qt, qb, ph), cube_import.pooled_dim(ow, ql, qr, pw)
        if v[4] != Ph or v[5] != Pw:
            return dict(error=E_SIZE)
        if v[4] * v[5] * v[6] * ph * pw > 1 << 20 or kh * kw * ic > 1 << 16:
            return dict(error=E_NO_IMPL)
        P = ph * pw
        if P not in (1, 2, 4):
            return dict(error=E_NO_IMPL)
        if v[11] > 1:
            return dict(error=E_SIZE)
        K, oc = kh * kw * ic, v[6]
        if v[14] != (K + 3) // 4 * 4 or v[15] != (oc + 15) // 16 * 16:
            return dict(error=E_SIZE)
        if len(layers) == fe.MAX_LAYERS:
            return dict(error=E_NO_IMPL)
        k_pad, n_pad = v[14], v[15]
        rows, out_n = v[4] * v[5] * P, v[4] * v[5] * oc
        wl = k_pad * n_pad
        if wl > fe.LDS_BYTES // 4:
            return dict(error=E_NO_IMPL)
        pad = any(v[16:24])
        kn = 2 * k_pad if pad else k_pad
        live = sum(qt <= y < qt + oh for y in range(Ph * ph)) * sum(ql <= x < ql + ow for x in range(Pw * pw))
        src = len(layers) & 1
        NT = n_pad // 16
        NG = (NT + 3) // 4
        wfl += wl + n_pad
        tabn += kn + rows
        acts += out_n
        if out_n > 1 << 20 or tabn > 1 << 26 or acts > 1 << 26:
            return dict(error=E_NO_IMPL)
        buf[src ^ 1] = max(buf[src ^ 1], out_n)
        w_lds, k_lds = max(w_lds, wl), max(k_lds, kn)
        layers.append(dict(P=P, rows=rows, K=K, k_pad=k_pad, n_pad=n_pad, NT=NT, NG=NG, nt_last=NT - 4 * (NG - 1), src=src, dst=src ^ 1,
                           relu=v[11], out_c=oc, out_n=out_n, in_c=ic, k=(kh, kw), s=(sh, sw), p=(ph, pw), pad=pad, cpad=(pt, pl, pb, pr),
                           ppad=(qt, ql, qb, qr), live=live, kn=kn, inp=(ih, iw, ic)))
        h, w, c = v[4], v[5], oc
    if not layers or h * w * c != n_out:
        return dict(error=E_SIZE)
    if off + 4 * wfl != len(blob):
        return dict(error=E_SIZE)
    buf_n = [(buf[0] + 3) & ~3, (buf[1] + 3) & ~3]
    fixed, per = 4 * (w_lds + k_lds), 4 * (buf_n[0] + buf_n[1])
    batch = min((fe.LDS_BYTES - fixed) // per, fe.MAX_BATCH)
    if batch < 1:
        return dict(error=E_NO_IMPL)
    if batch * layers[-1]["rows"] > (2 ** 31 - 1) // 16:
        return dict(error=E_NO_IMPL)
    return dict(n_layers=len(layers), in_n=in_h * in_w * in_c, n_out=n_out, batch=batch, buf_n=buf_n, w_lds=w_lds, k_lds=k_lds,
                acts_floats=acts, lds_bytes=4 * (batch * (buf_n[0] + buf_n[1]) + w_lds) + 4 * k_lds, layers=layers)


# ---- the zoo: kws_keras.get_model's padded architectures ------------------------------------------------------------------------------
def _same(h, w, k, s):
    (t, b), (l, r) = cube_import.same_pads(h, k[0], s[0]), cube_import.same_pads(w, k[1], s[1])
    return t, l, b, r


def zoo_specs(name, in_shape=(31, 13, 1), n_classes=10):
    """The layers of one of the reference training script's padded sequential architectures at in_shape, as cube_sources specs:
    padding='same' convolutions (ReLU) and MaxPooling2D((2, 2)), 'same' or 'valid', then Dense and Softmax."""
    arch = dict(tiny_conv=[(8, (8, 10), (2, 2), None)],
                medium_embedding_conv=[(16, (8, 8), (2, 2), "same"), (12, (4, 4), (1, 1), None)],
                tiny_embedding_conv=[(8, (8, 10), (2, 2), "same"), (8, (8, 10), (8, 8), None)],
                simple_conv=[(8, (8, 8), (1, 1), "valid")])[name]
    h, w, _ = in_shape
    specs = []
    for oc, k, s, pool in arch:
        cp = _same(h, w, k, s)
        ch, cw = -(-h // s[0]), -(-w // s[1])
        p, pp = ((2, 2), _same(ch, cw, (2, 2), (2, 2)) if pool == "same" else Z4) if pool else ((1, 1), Z4)
        specs.append(("conv", oc, k, s, p, 1, cp, pp))
        h, w = out_hw((h, w), k, s, p, cp, pp)
    return specs + [("dense", n_classes), ("softmax",)]


ZOO = ("tiny_conv", "medium_embedding_conv", "tiny_embedding_conv", "simple_conv")


def cube_sources(in_shape, specs, seed=0, name="net", declared=None, pad_order="xyxy"):
    """cube_synth.cube_sources for conv specs with pads: ("conv", out_c, (kh, kw), (sh, sw), (ph, pw), relu, cpad, ppad), pads (top,
    left, bottom, right), written as X-CUBE-AI's (x start, y start, x end, y end). declared: {layer index: (h, w)} writes another
    output shape than the computed one; the importer must refuse it."""
    rng = np.random.default_rng(seed)
    hwc = cube_synth._hwc
    h, w, c = in_shape
    tensors, arrays, layers, blob, woff = [], {}, [], bytearray(), {}
    t_in = hwc("input_0_output", h, w, c)
    tensors.append(t_in)
    arrays[t_in["array"]] = (t_in["n"], "AI_ARRAY_FORMAT_FLOAT|AI_FMT_FLAG_IS_IO")
    cur = t_in

    def add_weights(tname, shape, stride, vals):
        arr = tname + "_array"
        tensors.append(dict(name=tname, shape=shape, stride=stride, array=arr, n=vals.size))
        arrays[arr] = (vals.size, "AI_ARRAY_FORMAT_FLOAT")
        woff[arr] = len(blob)
        blob.extend(np.asarray(vals, "<f4").tobytes())
        return tname

    def shape4(p):
        return "AI_SHAPE_INIT(4, %d, %d, %d, %d)" % (p[1], p[0], p[3], p[2])

    for i, s in enumerate(specs):
        lname = "layer_%d" % i
        if s[0] == "conv":
            _, oc, (kh, kw), (sh, sw), (ph, pw), relu, cp, pp = s
            ic, ch, cw = cur["shape"][1], cur["shape"][3], cur["shape"][2]
            oh, ow = (declared or {}).get(i) or out_hw((ch, cw), (kh, kw), (sh, sw), (ph, pw), cp, pp)
            W = rng.normal(0, 1.0 / np.sqrt(kh * kw * ic), (oc, kh, kw, ic)).astype(np.float32)
            B = rng.normal(0, 0.1, oc).astype(np.float32)
            wt = add_weights(lname + "_weights", (ic, kw, kh, oc), (4, 4 * ic, 4 * ic * kw, 4 * ic * kw * kh), W.reshape(-1))
            bt = add_weights(lname + "_bias", (1, oc, 1, 1), (4, 4, 4 * oc, 4 * oc), B)
            out = hwc(lname + "_output", oh, ow, oc)
            pool = (ph, pw) != (1, 1)
            fields = [".groups = 1", ".nl_func = %s" % ("nl_func_relu_array_f32" if relu else "NULL"),
                      ".filter_stride = AI_SHAPE_2D_INIT(%d, %d)" % (sw, sh), ".dilation = AI_SHAPE_2D_INIT(1, 1)", ".filter_pad = " + shape4(cp)]
            if pool:
                fields += [".pool_size = AI_SHAPE_2D_INIT(%d, %d)" % (pw, ph), ".pool_stride = AI_SHAPE_2D_INIT(%d, %d)" % (pw, ph),
                           ".pool_pad = " + shape4(pp), ".pool_func = pool_func_mp_array_f32"]
            kind = ("OPTIMIZED_CONV2D_TYPE", "conv2d_nl_pool", "forward_conv2d_nl_pool") if pool else ("CONV2D_TYPE", "conv2d", "forward_conv2d")
            layers.append(dict(name=lname, kind=kind, fields=fields, inp=cur, out=out, params=[wt, bt]))
        elif s[0] == "dense":
            n_in, n_out = cur["n"], s[1]
            view = dict(hwc(cur["name"] + "0", 1, 1, n_in), array=cur["array"])
            tensors.append(view)
            W = rng.normal(0, 1.0 / np.sqrt(n_in), (n_out, n_in)).astype(np.float32)
            B = rng.normal(0, 0.1, n_out).astype(np.float32)
            wt = add_weights(lname + "_weights", (n_in, n_out, 1, 1), (4, 4, 4 * n_in, 4 * n_in * n_out), W.reshape(-1))
            bt = add_weights(lname + "_bias", (1, n_out, 1, 1), (4, 4, 4 * n_out, 4 * n_out), B)
            out = hwc(lname + "_output", 1, 1, n_out)
            layers.append(dict(name=lname, kind=("DENSE_TYPE", "dense", "forward_dense"), fields=[], inp=view, out=out, params=[wt, bt]))
        elif s[0] == "softmax":
            out = hwc(lname + "_output", cur["shape"][3], cur["shape"][2], cur["shape"][1])
            layers.append(dict(name=lname, kind=("NL_TYPE", "nl", "forward_sm"), fields=[], inp=cur, out=out, params=None))
        else:
            raise ValueError(s)
        tensors.append(out)
        arrays[out["array"]] = (out["n"], "AI_ARRAY_FORMAT_FLOAT")
        cur = out

    L = ["/* written in X-CUBE-AI's format from seeded random weights */", '#include "%s.h"' % name, ""]
    for a, (n, fmt) in arrays.items():
        L.append("AI_ARRAY_OBJ_DECLARE(\n    %s, %s,\n    NULL, NULL, %d,\n     AI_STATIC)" % (a, fmt, n))
    for t in tensors:
        L.append("AI_TENSOR_OBJ_DECLARE(\n  %s, AI_STATIC,\n  0x0, 0x0, AI_SHAPE_INIT(4, %d, %d, %d, %d), AI_STRIDE_INIT(4, %d, %d, %d, %d),\n  1, &%s, NULL)"
                 % ((t["name"],) + tuple(t["shape"]) + tuple(t["stride"]) + (t["array"],)))
    for i, ly in enumerate(layers):
        p = "AI_TENSOR_LIST_ENTRY(%s, NULL)" % ", ".join("&" + x for x in ly["params"]) if ly["params"] else "AI_TENSOR_LIST_EMPTY"
        L.append("AI_TENSOR_CHAIN_OBJ_DECLARE(\n  %s_chain, AI_STATIC_CONST, 4,\n  AI_TENSOR_LIST_ENTRY(&%s),\n  AI_TENSOR_LIST_ENTRY(&%s),\n  %s,\n  AI_TENSOR_LIST_EMPTY\n)"
                 % (ly["name"], ly["inp"]["name"], ly["out"]["name"], p))
        nxt = layers[i + 1]["name"] if i + 1 < len(layers) else ly["name"]
        f = "".join(", \n  %s" % x for x in [".tensors = &%s_chain" % ly["name"]] + ly["fields"])
        L.append("AI_LAYER_OBJ_DECLARE(\n  %s, %d,\n  %s,\n  %s, %s,\n  &AI_NET_OBJ_INSTANCE, &%s, AI_STATIC%s, \n)"
                 % (ly["name"], i, ly["kind"][0], ly["kind"][1], ly["kind"][2], nxt, f))
    L.append("AI_NETWORK_OBJ_DECLARE(\n  AI_NET_OBJ_INSTANCE, AI_STATIC,\n  AI_BUFFER_OBJ_INIT(AI_BUFFER_FORMAT_U8,\n                     1, 1, %d, 1,\n                     NULL),\n"
             "  AI_BUFFER_OBJ_INIT(AI_BUFFER_FORMAT_U8,\n                     1, 1, 0, 1,\n                     NULL),\n"
             "  AI_TENSOR_LIST_IO_ENTRY(AI_FLAG_NONE, AI_NET_IN_NUM, &%s),\n  AI_TENSOR_LIST_IO_ENTRY(AI_FLAG_NONE, AI_NET_OUT_NUM, &%s),\n  &%s, 0, NULL)"
             % (len(blob), t_in["name"], cur["name"], layers[0]["name"]))
    L.append("AI_DECLARE_STATIC\nai_bool %s_configure_weights(\n  ai_network* net_ctx, const ai_buffer* weights_buffer)\n{\n  ai_ptr weights = AI_PTR(weights_buffer->data);\n  {" % name)
    for a, off in woff.items():
        L.append("    %s.data = AI_PTR(weights + %d);\n    %s.data_start = AI_PTR(weights + %d);" % (a, off, a, off))
    L.append("  }\n  return true;\n}\n")
    rows = [", ".join("0x%02x" % b for b in blob[i:i + 10]) for i in range(0, len(blob), 10)]
    data = ('#include "%s_data.h"\n\nai_handle ai_%s_data_weights_get(void)\n{\n  AI_ALIGNED(4)\n  static const ai_u8 s_%s_weights[ %d ] = {\n    %s\n  };\n'
            "  return AI_HANDLE_PTR(s_%s_weights);\n}\n" % (name, name, name, len(blob), ",\n    ".join(rows), name))
    return "\n\n".join(L), data


def import_sources(net_c, data_c):
    return cube_import.build_blob(cube_import.convert(cube_import.parse_net_c(net_c), cube_import.parse_data_c(data_c)))


# ---- the sweep rows -------------------------------------------------------------------------------------------------------------------
def _c(oc, k, s=(1, 1), p=(1, 1), relu=1, cpad=Z4, ppad=Z4):
    return ("conv", oc, k, s, p, relu, cpad, ppad)


ROWS = {
    "sym3x3": (dict(in_shape=(5, 4, 1), layers=[_c(3, (3, 3), cpad=(1, 1, 1, 1)), ("dense", 3, 0)]),
               "one pad on every side of a 3x3 kernel: every corner and edge window has taps outside"),
    "asym_even": (dict(in_shape=(6, 5, 2), layers=[_c(5, (4, 2), cpad=(1, 0, 2, 1)), ("dense", 4, 0)]),
                  "even kernel extents, four different pads, two input channels (ci runs inside a tap), ReLU"),
    "stride2_same": (dict(in_shape=(7, 6, 1), layers=[_c(4, (3, 3), s=(2, 2), cpad=(1, 0, 1, 1)), ("dense", 3, 0)]),
                     "Keras's 'same' at stride 2: an odd extent pads both ends, an even one only the far end"),
    "top_only": (dict(in_shape=(4, 3, 1), layers=[_c(2, (3, 2), cpad=(2, 0, 0, 0)), ("dense", 3, 0)]),
                 "two rows above and nothing else: swapped axes or swapped ends change the shape or the values"),
    "left_only": (dict(in_shape=(3, 4, 1), layers=[_c(2, (2, 3), cpad=(0, 2, 0, 0)), ("dense", 3, 0)]),
                  "two columns on the left and nothing else"),
    "k_wider_than_input": (dict(in_shape=(4, 3, 2), layers=[_c(3, (2, 5), cpad=(0, 1, 0, 1)), ("dense", 3, 0)]),
                           "a 2x5 kernel over 3 columns: it fits only with the pads, the output is one column wide"),
    "pool22_odd": (dict(in_shape=(6, 4, 1), layers=[_c(4, (2, 2), p=(2, 2), ppad=(0, 0, 1, 1)), ("dense", 3, 0)]),
                   "pool (2, 2) over a 5x3 map padded at the far ends: windows of 4, 2, 2 and 1 present elements"),
    "pool21_tail": (dict(in_shape=(6, 3, 1), layers=[_c(3, (2, 2), p=(2, 1), ppad=(0, 0, 1, 0)), ("dense", 3, 0)]),
                    "pool (2, 1) over 5 rows: the last window has one present element"),
    "pool41_lead": (dict(in_shape=(6, 4, 1), layers=[_c(4, (2, 2), p=(4, 1), ppad=(1, 0, 2, 0)), ("dense", 3, 0)]),
                    "pool (4, 1) over 5 rows, pads 1 and 2: absent elements lead one window and trail the other; 24 rows per utterance, "
                    "so M tiles end inside an utterance"),
    "pool14_oc17": (dict(in_shape=(4, 6, 1), layers=[_c(17, (2, 2), p=(1, 4), ppad=(0, 1, 0, 2)), ("dense", 3, 0)]),
                    "the same along the width, 17 channels: two channel tiles in a padded layer"),
    "neg_no_relu": (dict(in_shape=(5, 5, 1), layers=[_c(4, (3, 3), p=(2, 2), relu=0, cpad=(1, 1, 1, 1), ppad=(1, 1, 0, 0)), ("dense", 3, 0)],
                         bias=-30.0, positive=True, sets=["neg"]),
                    "conv and pool pads together, no ReLU, bias -30, positive weights on all-negative inputs: every real value is below "
                    "-30, an absent element that turned into 0 would win every window it is in"),
    "mid_pads_batch": (dict(in_shape=(24, 20, 2), layers=[_c(4, (3, 3)), _c(8, (3, 3), cpad=(1, 2, 1, 0)),
                                                           _c(6, (3, 3), s=(2, 2), p=(1, 2), cpad=(1, 1, 0, 0), ppad=(0, 0, 0, 1)), ("dense", 5, 0)]),
                       "three convs, pads on the second and third (the padded gather reads both LDS buffers), 4752 floats of activations "
                       "per utterance: a plan batch below 16"),
    "oc65_pad": (dict(in_shape=(4, 4, 1), layers=[_c(65, (3, 3), cpad=(1, 0, 1, 0)), ("dense", 4, 0)]),
                 "65 channels on a padded layer: two channel groups, the second with one tile"),
}
ROWS.update({name: (dict(in_shape=(31, 13, 1), zoo=name), "kws_keras.get_model's %s at the shipped 31x13x1 input, through the importer" % name)
             for name in ZOO})


def _records(in_shape, layers):
    h, w, c = in_shape
    out = []
    for L in layers:
        if L[0] == "dense":
            out.append(dict(type=cube_import.T_CONV, inp=(h, w, c), out=(1, 1, L[1]), k=(h, w), s=(1, 1), p=(1, 1), relu=L[2], cpad=Z4, ppad=Z4))
        else:
            _, oc, k, s, p, relu, cp, pp = L
            out.append(dict(type=cube_import.T_CONV, inp=(h, w, c), out=out_hw((h, w), k, s, p, cp, pp) + (oc,), k=k, s=s, p=p, relu=relu,
                            cpad=cp, ppad=pp))
        h, w, c = out[-1]["out"]
    return out


def _seed(name):
    return sum(map(ord, name))


def model(name):
    """Row `name` -> the cube_import model dict (float32 weights, cpad / ppad on every conv record)."""
    spec = ROWS[name][0]
    if "zoo" in spec:
        return cube_import.read_blob(blob(name))
    rng = np.random.default_rng(2000 + _seed(name))
    recs = _records(spec["in_shape"], spec["layers"])
    for L in recs:
        oc, (kh, kw), ic = L["out"][2], L["k"], L["inp"][2]
        w = rng.normal(0, 1, (oc, kh, kw, ic)) / np.sqrt(kh * kw * ic)
        L["w"] = (np.abs(w) if spec.get("positive") else w).astype(np.float32)
        L["b"] = (np.full(oc, spec["bias"]) if "bias" in spec else rng.normal(0, 0.1, oc)).astype(np.float32)
    last = recs[-1]["out"]
    recs.append(dict(type=cube_import.T_SOFTMAX, inp=last, out=last))
    return dict(in_shape=spec["in_shape"], layers=recs)


def sources(name):
    spec = ROWS[name][0]
    return cube_sources(spec["in_shape"], zoo_specs(spec["zoo"], spec["in_shape"]), seed=_seed(name))


_BLOBS = {}


def blob(name):
    if name not in _BLOBS:
        _BLOBS[name] = import_sources(*sources(name)) if "zoo" in ROWS[name][0] else cube_import.build_blob(model(name))
    return _BLOBS[name]


def unpadded(m):
    """The same layers with every pad removed (shapes shrink; a dense layer's weights are cut to its new input). None when a kernel
    no longer fits."""
    h, w, c = was = m["in_shape"]
    out = []
    for L in m["layers"]:
        L, before = dict(L), was
        was = L["out"]
        if L["type"] == cube_import.T_CONV:
            dense = tuple(L["k"]) == tuple(L["inp"][:2]) and not any(L.get("cpad", Z4))
            if dense:
                flat = tuple(L["inp"][:2]) == (1, 1) and tuple(before[:2]) != (1, 1)      # the importer's dense: 1 x 1 over a flat view
                L["w"] = np.ascontiguousarray(L["w"].reshape((-1,) + tuple(before))[:, :h, :w, :c])
                if flat:
                    L["w"] = L["w"].reshape(-1, 1, 1, h * w * c)
                    h, w, c = 1, 1, h * w * c
                L["k"] = (h, w)
            L["inp"] = (h, w, c)
            L["cpad"] = L["ppad"] = Z4
            oh, ow = out_hw((h, w), L["k"], L["s"], L["p"], Z4, Z4)
            if oh < 1 or ow < 1:
                return None
            L["out"] = (oh, ow, L["out"][2])
        else:
            L["inp"] = L["out"] = (h, w, c)
        h, w, c = L["out"]
        out.append(L)
    return dict(in_shape=m["in_shape"], layers=out)


def inputs(name, n, in_n):
    """n inputs [n][in_n] float32 of row `name`, from fnet_sweep's input sets."""
    sets = ROWS[name][0].get("sets", fs.SETS)
    rng = np.random.default_rng(_seed(name))
    x = np.empty((n, in_n), np.float32)
    for i in range(n):
        g = rng.normal(0, 1, in_n)
        x[i] = dict(n1=g, n60=60 * g, i16=rng.integers(-32768, 32768, in_n), zero=0 * g, neg=-np.abs(30 * g) - 1.0)[sets[i % len(sets)]]
    return x


def facts(name):
    """What row `name` takes that another row may not: its padded layers' pads, strides and pools, kernels wider than their input,
    padded layers behind the first, channel groups in a padded layer, a plan batch below 16."""
    p = plan(blob(name))
    f = set()
    for i, L in enumerate(p["layers"]):
        if not L["pad"]:
            continue
        if any(L["cpad"]):
            f.add(("cpad", L["cpad"], L["s"], any(L["ppad"])))
        if any(L["ppad"]):
            f.add(("ppad", L["p"], L["ppad"]))
        f |= {("k>in", a) for a in (0, 1) if L["k"][a] > L["inp"][a]}
        f |= {("pad_layer", i)} if i else set()
        f |= {("pad_NG", L["NG"])} if L["NG"] > 1 else set()
        f |= {("pad_nt", L["nt_last"])} if L["nt_last"] > 1 else set()
        f |= {("pad_no_relu",)} if not L["relu"] else set()
        if L["P"] == 4 and L["live"] < L["rows"] and any(nu * L["rows"] % 16 for nu in range(1, p["batch"] + 1)):
            f.add(("m_tail_P4_absent",))
    if 1 < p["batch"] < 16:
        f.add(("batch_mid",))
    return frozenset(f)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _pack(ver, in_shape, recs, n_out, payload=b""):
    head = cube_import.HDR.pack(cube_import.MAGIC, ver, len(recs), *in_shape, n_out) + b"\0\0\0\0"
    return head + b"".join(np.asarray(r, "<i4").tobytes() for r in recs) + payload


def _conv_rec(inp, out, k, s, p, relu, cpad=Z4, ppad=Z4):
    return fs._conv_rec(inp, out, k, s, p, relu) + list(cpad) + list(ppad)


def _sm_rec(shape):
    return fs._sm_rec(shape) + [0] * 8


def _payload(recs):
    return b"\0" * (4 * sum(r[14] * r[15] + r[15] for r in recs if r[0] == cube_import.T_CONV))


def _v2(in_shape, conv, n_out=None):
    recs = [conv, _sm_rec(tuple(conv[4:7]))]
    return _pack(2, in_shape, recs, n_out or conv[4] * conv[5] * conv[6], _payload(recs))


REFUSALS = {
    # a pad as large as the window on its axis: a window wholly in padding
    "conv_pad_is_kernel": (lambda: _v2((5, 4, 1), _conv_rec((5, 4, 1), (6, 4, 3), (3, 3), (1, 1), (1, 1), 1, cpad=(3, 1, 0, 1))), fe.E_NO_IMPL,
                           "top pad 3 under a 3x3 kernel (the shape follows from the formula: only the pad is wrong)"),
    "pool_pad_is_pool": (lambda: _v2((6, 4, 1), _conv_rec((6, 4, 1), (3, 3, 4), (2, 2), (1, 1), (2, 1), 1, ppad=(2, 0, 0, 0))), fe.E_NO_IMPL,
                         "top pool pad 2 under a (2, 1) pool"),
    "out_shape_off_by_one": (lambda: _v2((5, 4, 1), _conv_rec((5, 4, 1), (5, 5, 3), (3, 3), (1, 1), (1, 1), 1, cpad=(1, 1, 1, 1))), fe.E_SIZE,
                             "pads (1, 1, 1, 1) under 3x3 give 5x4, the record declares 5x5"),
    "negative_pad": (lambda: _v2((5, 4, 1), _conv_rec((5, 4, 1), (4, 4, 3), (4, 3), (1, 1), (1, 1), 1, cpad=(-1, 1, 3, 1))), fe.E_SIZE,
                     "top pad -1 under a 4x3 kernel (with bottom 3 the sums still give the declared shape)"),
    "version3": (lambda: blob("sym3x3")[:4] + b"\x03" + blob("sym3x3")[5:], fe.E_NO_IMPL, "a version the loader does not know"),
}

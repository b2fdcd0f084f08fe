"""The float32 network (edison_fnet_*, DESIGN.md sections 14, 14b, 14c) restated on the host, once, for every test of it and of what is
built on it (calibrator, quantiser, trainer, float stream and bank). Test infrastructure, not a test. Three things, all on a model
dict of cube_import.read_blob / build_blob, with or without pads:

The float64 restatement (conv_layer, layer_from, run64): what the Cube runtime's forward_conv2d_nl_pool / forward_conv2d /
forward_dense / forward_sm compute, in float64 with numpy. Activations are HWC (rows = time, columns = coefficients), conv weights
[out][kh][kw][in], a dense layer is a conv whose kernel covers its whole input; bias, then ReLU, then max pool. Beside every output
it gives S = sum |a| |w| + |bias|: the scale the kernel's f32 error is bounded by (K_BOUND 1e-7 S, `bound`).

The bit-exact model of the kernels (ed_fnet_kernel in csrc/fnet_kernels.hip, the layer road's in csrc/fnet_layer_kernels.hip): every
output before the epilogue is a k-ordered f32 fmaf chain, acc = +0.0f, then acc = fmaf(a_k, w_k, acc) for k = (ky kw + kx) in_c + ci
= 0 .. K - 1 (one v_mfma_f32_16x16x4_f32 per 4 k; the K padding multiplies zeros). Then one f32 add of the bias, ReLU = fmaxf(v, 0),
and the max over the P rows of each pool window. Nothing flushes subnormals. fma32 is a correctly rounded f32 fma in numpy: p = a b
is exact in float64 (48 bits), s = p + c rounded to float64 with its TwoSum error e, then rounded to odd (when e != 0 and s's last
bit is 0, s steps one ulp toward e) and cast to float32. Round-to-odd at 53 bits then round-to-nearest at 24 is the correctly
rounded result because 53 >= 24 + 2; that holds for subnormal results too.

The calibration statistic (edison_fcal_*, csrc/fnet_calib_kernels.hip) on that model: index 0 is the network
input, index i conv / dense record i - 1. Per index: absmax = the largest bit pattern of fabsf(v) as uint32, hist[e] = how many v
have biased exponent field e, count = how many v. For a record v = acc + bias in f32, before ReLU and before the pool, over the out_c
real channels of every real conv output of a pool window: a row that a truncating pool drops is not computed, an absent element --
one in the pool's padding -- is counted nowhere. Each record is fed this model's own previous output, as the kernel feeds its own.

Pads (Keras / TensorFlow's semantics; cpad / ppad = (top, left, bottom, right), absent = zeros). Conv: out = (in + before + after - k)
// stride + 1; a tap outside the image is the operand +0.0f and stays in the fmaf chain, which is therefore as long as without pads.
Pool, window = stride: pooled = (conv + before + after - p) // p + 1; an element of a window outside the conv's map is absent: it
takes no part in the max (identity -inf, never 0). Both models are written differently from the kernel on purpose: they work on a
zero-bordered (for the pool: -inf-bordered) copy of the image, the kernel on the dense image with a predicate per tap."""
import numpy as np

from edison_amd import cube_import

K_BOUND = 8.0                        # tests/test_gpu_fnet.py: |gpu - f64| <= 8e-7 S
Z4 = (0, 0, 0, 0)


def load(src):
    """An .ednf path or its bytes -> the model dict of cube_import.read_blob."""
    if isinstance(src, (bytes, bytearray)):
        return cube_import.read_blob(bytes(src))
    with open(src, "rb") as f:
        return cube_import.read_blob(f.read())


def swapped(model):
    """The same model with every conv kernel's kh and kw exchanged (square kernels): the layout the fixture guards against."""
    out = dict(model, layers=[])
    for L in model["layers"]:
        L = dict(L)
        if "w" in L and L["k"][0] == L["k"][1] and L["k"][0] > 1 and L["inp"][:2] != L["k"]:
            L["w"] = L["w"].transpose(0, 2, 1, 3).copy()
        out["layers"].append(L)
    return out


def conv_records(model):
    return [L for L in model["layers"] if L["type"] == cube_import.T_CONV]


def pads(L):
    return tuple(L.get("cpad", Z4)), tuple(L.get("ppad", Z4))


def conv_map(L):
    """(conv_h, conv_w) of record L: its map before the pool."""
    (ih, iw, _), (kh, kw), (sh, sw), (c, _) = L["inp"], L["k"], L["s"], pads(L)
    return (ih + c[0] + c[2] - kh) // sh + 1, (iw + c[1] + c[3] - kw) // sw + 1


def out_hw(inp_hw, k, s, p, cpad=Z4, ppad=Z4):
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
    cols = win.transpose(0, 1, 2, 4, 5, 3).reshape(n, ch, cw, -1)                               # k = (ky kw + kx) c + ci
    w = L["w"].astype(np.float64).reshape(L["w"].shape[0], -1)                                 # [out][K]
    b = L["b"].astype(np.float64)
    y = cols @ w.T + b
    S = np.abs(cols) @ np.abs(w).T + np.abs(b)
    if L["relu"]:
        y = np.maximum(y, 0.0)
    return _pool(y, L, -np.inf), S


def layer_from(model, i, a_in):
    """Conv record i (0-based among conv records) on a given flat input a_in [n][...] -> (y flat float64, bound scale S of each
    output after the pool: the largest S of its window's real elements)."""
    L = conv_records(model)[i]
    y, S = conv_layer(L, np.asarray(a_in, np.float64).reshape((-1,) + tuple(L["inp"])))
    return y.reshape(y.shape[0], -1), _pool(S, L, 0.0).reshape(S.shape[0], -1)


def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def run64(model, x):
    """x [n][in_h*in_w*in_c] (any float type) -> dict(acts: per conv layer [n][out_h*out_w*out_c] float64, each fed the previous
    one, S: per conv layer its pre-pool bound scale, logits [n][n_out], probs, argmax (first maximum))."""
    a, acts, S = np.asarray(x, np.float64), [], []
    for L in conv_records(model):
        a, s = conv_layer(L, a.reshape((-1,) + tuple(L["inp"])))
        a = a.reshape(a.shape[0], -1)
        acts.append(a)
        S.append(s)
    p = softmax(acts[-1])
    return dict(acts=acts, S=S, logits=acts[-1], probs=p, argmax=np.argmax(p, axis=1).astype(np.int32))


# ---- the bit-exact model ------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c), elementwise. Arguments: float32 values (any float dtype holding them); returns float32."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    return _fma_f64(a * b, c).astype(np.float32)


def _fma_f64(p, c):
    """p (an exact product of two float32) + c (a float32), both float64, rounded to odd at 53 bits: float64 that casts to the
    correctly rounded float32."""
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    odd = (e != 0) & ((bits & 1) == 0)
    if odd.any():
        # one ulp toward e: away from zero when s and e have the same sign, toward zero otherwise (s != 0 whenever e != 0)
        step = np.where((s > 0) == (e > 0), 1, -1).astype(np.int64)
        s = (bits + np.where(odd, step, 0)).view(np.float64)
    return s


def chain(A, W, variant=None):
    """acc[m][n] = the k-ordered fmaf chain of A [M][K] and W [K][N] from +0.0f (float32). `variant` names a wrong arithmetic the
    sensitivity test needs: "reversed" (k from K - 1 down), "rounded_product" (f32(a w) then an f32 add), "f64_sum" (the float64
    sum rounded once), "drop_last" (the last real k term left out)."""
    A = np.asarray(A, np.float32).astype(np.float64)
    W = np.asarray(W, np.float32).astype(np.float64)
    M, K = A.shape
    if variant == "f64_sum":
        return (A @ W).astype(np.float32)
    ks = range(K - 1, -1, -1) if variant == "reversed" else range(K - 1 if variant == "drop_last" else K)
    acc = np.zeros((M, W.shape[1]), np.float64)
    for k in ks:
        p = A[:, k, None] * W[None, k, :]
        if variant == "rounded_product":
            acc = (p.astype(np.float32) + acc.astype(np.float32)).astype(np.float64)
        else:
            acc = _fma_f64(p, acc).astype(np.float32).astype(np.float64)
    return acc.astype(np.float32)


def gather(L, x):
    """The kernel's A operand of record L for inputs x [n][in_n]: ([n * rows][K] float32 with +0.0f at the padded taps, rows in the
    kernel's order (row r = element r % P of the pool window of pooled position r / P), k = (ky kw + kx) in_c + ci; and live [rows]:
    False for the absent elements of a pool window, whose A row is not used)."""
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
    v = chain(A, L["w"].reshape(oc, -1).T, variant) + L["b"].astype(np.float32)[None, :]
    return v.astype(np.float32), np.tile(live, A.shape[0] // live.size)


def _epilogue(L, v, live, absent=-np.inf):
    oc, P = L["out"][2], L["p"][0] * L["p"][1]
    if L["relu"]:
        v = np.maximum(v, np.float32(0))
    v = np.where(live[:, None], v, np.float32(absent))
    return v.reshape(-1, P, oc).max(axis=1).reshape(-1, int(np.prod(L["out"]))).astype(np.float32)


def layer(L, x, variant=None, absent=-np.inf):
    """Record L on x [n][in_n] float32 -> [n][out_n] float32 as the kernel writes it: chain, + bias (f32), ReLU, max over the pool
    window; pooled position q, channel c at q out_c + c. `absent`: the value an absent element takes in the max; anything but -inf
    is a wrong kernel (the CPU test uses 0 to show what it changes)."""
    return _epilogue(L, *pre_activation(L, x, variant), absent)


def bound(L, S):
    """The GPU tests' 8e-7 S for conv record L, plus what underflow adds: each of the K + 1 roundings of an output errs by at most
    2^-150 (half the smallest subnormal) however small S is. The second term is below 1e-42: it only matters on subnormal outputs."""
    return K_BOUND * 1e-7 * S + (L["k"][0] * L["k"][1] * L["inp"][2] + 1) * 2.0 ** -150


def run(model, x, variant=None):
    """Every layer of the kernel on x [n][in_n], each fed this model's previous layer: list of float32 [n][out_n]."""
    out, a = [], np.asarray(x, np.float32)
    for L in conv_records(model):
        a = layer(L, a, variant)
        out.append(a)
    return out


def layers_from(model, x, acts, variant=None):
    """Every layer of the model, layer i fed layer i - 1 of `acts` (the kernel's own per-layer dump [n][acts_floats]) and layer 0 fed
    x: a mismatch points at one layer. Returns the list of float32 [n][out_n] and the list of the kernel's slices beside them."""
    want, got, off, prev = [], [], 0, np.asarray(x, np.float32)
    for L in conv_records(model):
        n_out = int(np.prod(L["out"]))
        want.append(layer(L, prev, variant))
        got.append(np.asarray(acts[:, off:off + n_out], np.float32))
        prev, off = got[-1], off + n_out
    assert off == acts.shape[1]
    return want, got


# ---- the calibration statistic ------------------------------------------------------------------------------------------------------
def of_values(v):
    """(absmax bits, hist[256], count) of a float32 array."""
    bits = np.ascontiguousarray(v, np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7fffffff)
    hist = np.bincount((bits >> np.uint32(23)).astype(np.int64), minlength=256).astype(np.uint64)
    return np.uint32(bits.max() if bits.size else 0), hist, np.uint64(bits.size)


def empty(n_records):
    return dict(absmax=np.zeros(n_records + 1, np.uint32), hist=np.zeros((n_records + 1, 256), np.uint64), count=np.zeros(n_records + 1, np.uint64))


def merge(a, b):
    return dict(absmax=np.maximum(a["absmax"], b["absmax"]), hist=a["hist"] + b["hist"], count=a["count"] + b["count"])


def stats(model, x):
    """The statistic of inputs x [n][in_n] through `model`."""
    recs = conv_records(model)
    s = empty(len(recs))
    a = np.ascontiguousarray(x, np.float32).reshape(-1, int(np.prod(model["in_shape"])))
    if a.shape[0] == 0:
        return s
    s["absmax"][0], s["hist"][0], s["count"][0] = of_values(a)
    for i, L in enumerate(recs):
        v, live = pre_activation(L, a)
        s["absmax"][i + 1], s["hist"][i + 1], s["count"][i + 1] = of_values(v[live])
        a = _epilogue(L, v, live)
    return s

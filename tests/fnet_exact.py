"""Bit-exact host model of the float32 network kernel (ed_fnet_kernel, edison_amd/csrc/fnet_kernels.hip) and a restatement of its
plan (parse() in edison_amd/csrc/edison_fnet.hip). Test infrastructure, not a test: tests/test_fnet_sweep_cpu.py holds it to glibc's
fmaf and to the float64 restatement (tests/fnet_ref.py), tests/test_gpu_fnet_sweep.py and tests/test_gpu_fnet.py hold the kernel to it.

The arithmetic the kernel claims, and this model computes: every output before the epilogue is a k-ordered f32 fmaf chain,
acc = +0.0f, then acc = fmaf(a_k, w_k, acc) for k = (ky kw + kx) in_c + ci = 0 .. K - 1 (one v_mfma_f32_16x16x4_f32 per 4 k; the K
padding multiplies zeros). Then one f32 add of the bias, ReLU = fmaxf(v, 0), and the max over the P rows of each pool window. Nothing
flushes subnormals.

fma32 is a correctly rounded f32 fma in numpy: p = a b is exact in float64 (48 bits), s = p + c rounded to float64 with its TwoSum
error e, then rounded to odd (when e != 0 and s's last bit is 0, s steps one ulp toward e) and cast to float32. Round-to-odd at 53
bits then round-to-nearest at 24 is the correctly rounded result because 53 >= 24 + 2; that holds for subnormal results too."""
import struct

import numpy as np

from edison_amd import cube_import

E_SIZE, E_NO_IMPL = -3, -17          # EDISON_E_SIZE, EDISON_E_NO_IMPL (include/edison_hip.h)
MAX_LAYERS = 16                      # ED_FNET_MAX_LAYERS (csrc/fnet.h)
MAX_BATCH = 16                       # ED_FNET_MAX_BATCH
LDS_BYTES = 160 * 1024               # ED_FNET_LDS_BYTES
MAX_DIM = 4096                       # EDF_MAX_DIM (edison_fnet.hip)
K_BOUND = 8.0                        # tests/test_gpu_fnet.py: |gpu - f64| <= 8e-7 S


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


# ---- the plan: parse() restated ------------------------------------------------------------------------------------------------
def plan(blob):
    """The kernel plan parse() builds from an .ednf blob: dict(n_layers, in_n, n_out, batch, buf_n, w_lds, k_lds, acts_floats,
    lds_bytes, layers=[dict(P, rows, k_pad, n_pad, NT, NG, nt_last, src, dst, relu, out_c, K)]), or dict(error=code) for a blob the
    loader refuses. The checks run in parse()'s order, so the code is the one the loader returns."""
    if len(blob) < 32 or blob[:4] != b"EDNF":
        return dict(error=E_SIZE)
    ver, nl, in_h, in_w, in_c, n_out, kwb = struct.unpack_from("<7i", blob, 4)
    if ver != 1:
        return dict(error=E_NO_IMPL)
    if nl < 2 or nl > MAX_LAYERS + 1:
        return dict(error=E_NO_IMPL)
    if min(in_h, in_w, in_c) < 1 or max(in_h, in_w, in_c) > MAX_DIM or kwb < 0 or kwb % 4:
        return dict(error=E_SIZE)
    if in_h * in_w * in_c > 1 << 20:
        return dict(error=E_NO_IMPL)
    off = 32 + nl * 64
    if off + kwb > len(blob):
        return dict(error=E_SIZE)
    off += kwb
    h, w, c = in_h, in_w, in_c
    wfl = tabn = acts = 0
    buf = [h * w * c, 0]
    layers, w_lds, k_lds = [], 0, 0
    for i in range(nl):
        v = struct.unpack_from("<16i", blob, 32 + 64 * i)
        if v[0] not in (cube_import.T_CONV, cube_import.T_SOFTMAX):
            return dict(error=E_NO_IMPL)
        for j in range(1, (15 if v[0] == cube_import.T_CONV else 6) + 1):
            if v[j] < (0 if j == 11 else 1) or v[j] > MAX_DIM * (16 if j >= 14 else 1):
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
        if kh > ih or kw > iw:
            return dict(error=E_SIZE)
        oh, ow = (ih - kh) // sh + 1, (iw - kw) // sw + 1
        if v[4] != oh // ph or v[5] != ow // pw:
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
        if len(layers) == MAX_LAYERS:
            return dict(error=E_NO_IMPL)
        k_pad, n_pad = v[14], v[15]
        rows, out_n = v[4] * v[5] * P, v[4] * v[5] * oc
        wl = k_pad * n_pad
        if wl > LDS_BYTES // 4:
            return dict(error=E_NO_IMPL)
        src = len(layers) & 1
        NT = n_pad // 16
        NG = (NT + 3) // 4
        wfl += wl + n_pad
        tabn += k_pad + rows
        acts += out_n
        if out_n > 1 << 20 or tabn > 1 << 26 or acts > 1 << 26:
            return dict(error=E_NO_IMPL)
        buf[src ^ 1] = max(buf[src ^ 1], out_n)
        w_lds, k_lds = max(w_lds, wl), max(k_lds, k_pad)
        layers.append(dict(P=P, rows=rows, K=K, k_pad=k_pad, n_pad=n_pad, NT=NT, NG=NG, nt_last=NT - 4 * (NG - 1), src=src, dst=src ^ 1,
                           relu=v[11], out_c=oc, out_n=out_n, in_c=ic, k=(kh, kw), s=(sh, sw), p=(ph, pw)))
        h, w, c = v[4], v[5], oc
    if not layers or h * w * c != n_out:
        return dict(error=E_SIZE)
    if off + 4 * wfl != len(blob):
        return dict(error=E_SIZE)
    buf_n = [(buf[0] + 3) & ~3, (buf[1] + 3) & ~3]
    fixed, per = 4 * (w_lds + k_lds), 4 * (buf_n[0] + buf_n[1])
    batch = min((LDS_BYTES - fixed) // per, MAX_BATCH)
    if batch < 1:
        return dict(error=E_NO_IMPL)
    if batch * layers[-1]["rows"] > (2 ** 31 - 1) // 16:
        return dict(error=E_NO_IMPL)
    return dict(n_layers=len(layers), in_n=in_h * in_w * in_c, n_out=n_out, batch=batch, buf_n=buf_n, w_lds=w_lds, k_lds=k_lds,
                acts_floats=acts, lds_bytes=4 * (batch * (buf_n[0] + buf_n[1]) + w_lds) + 4 * k_lds, layers=layers)


# ---- the layer model --------------------------------------------------------------------------------------------------------------
def gather(L, x):
    """The kernel's A operand of conv record L (cube_import.read_blob form) for inputs x [n][in_n]: [n * rows][K] float32, rows in the
    kernel's order (row r = element r % P of the pool window of pooled position r / P), k = (ky kw + kx) in_c + ci."""
    ih, iw, ic = L["inp"]
    kh, kw = L["k"]
    sh, sw = L["s"]
    ph, pw = L["p"]
    Ph, Pw = L["out"][:2]
    k = np.arange(kh * kw * ic)
    ci, t = k % ic, k // ic
    koff = ((t // kw) * iw + t % kw) * ic + ci
    q, e = np.divmod(np.arange(Ph * Pw * ph * pw), ph * pw)
    py, px = np.divmod(q, Pw)
    ey, ex = np.divmod(e, pw)
    rowin = ((py * ph + ey) * sh * iw + (px * pw + ex) * sw) * ic
    x = np.asarray(x, np.float32).reshape(-1, ih * iw * ic)
    return x[:, rowin[:, None] + koff[None, :]].reshape(-1, kh * kw * ic)


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


def layer(L, x, variant=None):
    """Conv record L on inputs x [n][in_n] float32 -> its output [n][out_n] float32 as the kernel writes it: chain, + bias (f32),
    ReLU, max over the pool window; pooled position q, channel c at q out_c + c."""
    oc = L["out"][2]
    P = L["p"][0] * L["p"][1]
    A = gather(L, x)
    W = L["w"].reshape(oc, -1).T
    v = chain(A, W, variant) + L["b"].astype(np.float32)[None, :]
    if L["relu"]:
        v = np.maximum(v, np.float32(0))
    v = v.reshape(-1, P, oc).max(axis=1)
    return v.reshape(-1, int(np.prod(L["out"]))).astype(np.float32)


def bound(L, S):
    """The GPU tests' 8e-7 S for conv record L, plus what underflow adds: each of the K + 1 roundings of an output errs by at most
    2^-150 (half the smallest subnormal) however small S is. The second term is below 1e-42: it only matters on subnormal outputs."""
    return K_BOUND * 1e-7 * S + (L["k"][0] * L["k"][1] * L["inp"][2] + 1) * 2.0 ** -150


def conv_records(model):
    return [L for L in model["layers"] if L["type"] == cube_import.T_CONV]


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

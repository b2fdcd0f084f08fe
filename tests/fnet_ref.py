"""Float64 restatement of an X-CUBE-AI float network read from its ``.ednf`` blob (edison_amd/cube_import.py): what the Cube
runtime's forward_conv2d_nl_pool / forward_conv2d / forward_dense / forward_sm compute, in float64 with numpy.

Activations are HWC (rows = time, columns = coefficients), conv weights [out][kh][kw][in], a dense layer is a conv whose kernel
covers its whole input; bias, then ReLU, then max pool. ``run`` also returns, per layer, S = sum |a| |w| + |bias| of every output
before the pool: the scale the kernel's f32 error is bounded by (k 1e-7 S)."""
import numpy as np

from edison_amd import cube_import


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


def conv_layer(L, x):
    """One conv / dense record on x [n][in_h][in_w][in_c] (float64) -> (y [n][out_h][out_w][out_c], S [n][oh][ow][out_c] pre-pool)."""
    x = np.asarray(x, np.float64)
    kh, kw = L["k"]
    sh, sw = L["s"]
    ph, pw = L["p"]
    win = np.lib.stride_tricks.sliding_window_view(x, (kh, kw), axis=(1, 2))[:, ::sh, ::sw]   # [n][oh][ow][c][kh][kw]
    n, oh, ow = win.shape[:3]
    cols = win.transpose(0, 1, 2, 4, 5, 3).reshape(n, oh, ow, -1)                               # k = (ky kw + kx) c + ci
    w = L["w"].astype(np.float64).reshape(L["w"].shape[0], -1)                                 # [out][K]
    b = L["b"].astype(np.float64)
    y = cols @ w.T + b
    S = np.abs(cols) @ np.abs(w).T + np.abs(b)
    if L["relu"]:
        y = np.maximum(y, 0.0)
    Ph, Pw = oh // ph, ow // pw
    y = y[:, :Ph * ph, :Pw * pw].reshape(n, Ph, ph, Pw, pw, -1).max(axis=(2, 4))
    return y, S


def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def run(model, x):
    """x [n][in_h*in_w*in_c] (any float type) -> dict(acts: per conv layer [n][out_h*out_w*out_c] float64, S: per conv layer
    its pre-pool bound scale, logits [n][n_out], probs, argmax (first maximum))."""
    h, w, c = model["in_shape"]
    a = np.asarray(x, np.float64).reshape(-1, h, w, c)
    acts, S = [], []
    for L in model["layers"]:
        if L["type"] == cube_import.T_CONV:
            a, s = conv_layer(L, a.reshape((-1,) + tuple(L["inp"])))
            acts.append(a.reshape(a.shape[0], -1))
            S.append(s)
    logits = acts[-1]
    p = softmax(logits)
    return dict(acts=acts, S=S, logits=logits, probs=p, argmax=np.argmax(p, axis=1).astype(np.int32))


def conv_records(model):
    return [L for L in model["layers"] if L["type"] == cube_import.T_CONV]


def layer_from(model, i, a_in):
    """Conv record i (0-based among conv records) on a given flat input a_in [n][...] -> (y flat float64, bound scale S of each
    output after the pool: the largest S in its pool window)."""
    L = conv_records(model)[i]
    x = np.asarray(a_in, np.float64).reshape((-1,) + tuple(L["inp"]))
    y, S = conv_layer(L, x)
    n, oh, ow, oc = S.shape
    ph, pw = L["p"]
    Ph, Pw = oh // ph, ow // pw
    Sp = S[:, :Ph * ph, :Pw * pw].reshape(n, Ph, ph, Pw, pw, oc).max(axis=(2, 4))
    return y.reshape(y.shape[0], -1), Sp.reshape(n, -1)

"""Float64 restatement of training a float network (edison_amd/train.py, csrc/fnet_grad_kernels.hip) on
fnet_ref's conventions: the loss, its gradient with respect to every weight and bias in the model dict's layout, Adam as Keras states
it, and a host trainer that edison_amd.train.fit drives like the GPU one. Test infrastructure, not a test:
tests/test_fgrad_cpu.py holds it to torch's float64 autograd and to central differences, tests/test_gpu_ftrain.py holds the kernels to it.

The definition. For n inputs and labels y, logits z: loss_u = logsumexp(z_u) - z_u[y_u], L = (1 / n_total) sum loss_u,
dL/dz_u = (softmax(z_u) - onehot(y_u)) / n_total. Backward through a record: the pool's gradient goes to the FIRST maximum of the
window in element order e = ey pw + ex (numpy's argmax), conv positions the pool's floor truncates get none; ReLU' is 1 where the
pre-activation is > 0, else 0; dW[out][k] = sum over positions and inputs of cols[.., k] dY[.., out]; dX by scattering dY W back
through the windows (input elements no window reads get 0). No probability clip (Keras's 1e-7 is not reproduced)."""
import numpy as np

from edison_amd import cube_import

import fnet_exact
import fnet_ref
import fnet_sweep

SATURATING = ("i16", "n60")   # input sets that saturate the softmax: they tell nothing about a gradient


def inputs(name, n, in_n):
    """n inputs of sweep row `name` as fnet_sweep.inputs draws them, without the rows of the i16 / n60 sets."""
    sets = fnet_sweep.ROWS[name][0].get("sets", fnet_sweep.SETS)
    keep = [i for i in range(len(sets)) if sets[i] not in SATURATING]
    m = (n + len(keep) - 1) // len(keep) * len(sets)
    x = fnet_sweep.inputs(name, m, in_n)
    rows = [i for i in range(m) if i % len(sets) in keep][:n]
    return np.ascontiguousarray(x[rows])


def conv_records(model):
    return fnet_ref.conv_records(model)


TIE_POOLS = ((1, 2), (2, 1), (2, 2), (4, 1), (1, 4))


def tie_case(pool, n=17):
    """(model, x [n][36], labels) whose pool windows tie exactly, without ReLU: a 2 x 2 conv to 3 channels on a 6 x 6 x 1 image, pool
    `pool` over its 5 x 5 map (truncating), a dense layer to 3 logits. The image is 0 / 1, the conv weights are +-0.5 / +-1 and the
    biases quarters, so every conv output is a sum that float32 holds exactly in any order and takes one of a few values: the first
    maximum of a window is tied at every element position. Channel 2 has zero weights: all its windows tie in every element."""
    rng = np.random.default_rng(77 + 10 * pool[0] + pool[1])
    recs = fnet_sweep._records((6, 6, 1), [("conv", 3, (2, 2), (1, 1), tuple(pool), 0), ("dense", 3, 0)])
    recs[0]["w"] = rng.choice([-1.0, -0.5, 0.5, 1.0], (3, 2, 2, 1)).astype(np.float32)
    recs[0]["w"][2] = 0.0
    recs[0]["b"] = np.array([0.25, -0.5, 0.75], np.float32)
    k = int(np.prod(recs[1]["inp"]))
    recs[1]["w"] = (rng.normal(0, 1, (3,) + tuple(recs[1]["k"]) + (3,)) / np.sqrt(k)).astype(np.float32)
    recs[1]["b"] = rng.normal(0, 0.1, 3).astype(np.float32)
    recs.append(dict(type=cube_import.T_SOFTMAX, inp=recs[1]["out"], out=recs[1]["out"]))
    x = rng.integers(0, 2, (n, 36)).astype(np.float32)
    return dict(in_shape=(6, 6, 1), layers=recs), x, (np.arange(n) % 3).astype(np.int32)


def _cols(L, x):
    kh, kw = L["k"]
    sh, sw = L["s"]
    win = np.lib.stride_tricks.sliding_window_view(x, (kh, kw), axis=(1, 2))[:, ::sh, ::sw]   # [n][oh][ow][c][kh][kw]
    n, oh, ow = win.shape[:3]
    return win.transpose(0, 1, 2, 4, 5, 3).reshape(n, oh, ow, -1)                              # k = (ky kw + kx) c + ci


def _weights64(model, weights):
    """Per conv record (w, b) float64: the model's own, or `weights` = [dict(w, b)]."""
    recs = conv_records(model)
    src = recs if weights is None else weights
    return [(np.asarray(t["w"], np.float64), np.asarray(t["b"], np.float64)) for t in src]


def loss_grad(model, x, labels, weights=None, n_total=None):
    """x [n][in_n], labels [n] -> dict(loss [n] per row, logits [n][n_out], argmax [n], grads [dict(w [out][kh][kw][in], b [out])] of
    the batch loss (1 / n_total) sum loss), all float64. weights: other values than the model's, same shapes."""
    recs = conv_records(model)
    W = _weights64(model, weights)
    labels = np.asarray(labels).reshape(-1)
    h, w, c = model["in_shape"]
    a = np.asarray(x, np.float64).reshape(-1, h, w, c)
    n = a.shape[0]
    n_total = n if n_total is None else n_total
    keep = []
    for L, (wt, b) in zip(recs, W):
        a = a.reshape((-1,) + tuple(L["inp"]))
        cols = _cols(L, a)
        pre = cols @ wt.reshape(wt.shape[0], -1).T + b
        act = np.maximum(pre, 0.0) if L["relu"] else pre
        ph, pw = L["p"]
        oh, ow, oc = pre.shape[1:]
        Ph, Pw = oh // ph, ow // pw
        win = act[:, :Ph * ph, :Pw * pw].reshape(n, Ph, ph, Pw, pw, oc).transpose(0, 1, 3, 5, 2, 4).reshape(n, Ph, Pw, oc, ph * pw)
        first = win.argmax(axis=-1)                                    # the first maximum in element order
        keep.append((a.shape, cols, pre, first))
        a = np.take_along_axis(win, first[..., None], -1)[..., 0]
    z = a.reshape(n, -1)
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    s = e.sum(axis=1, keepdims=True)
    loss = np.log(s[:, 0]) + mx[:, 0] - z[np.arange(n), labels]
    d = e / s
    d[np.arange(n), labels] -= 1.0
    d = d / n_total
    grads = [None] * len(recs)
    for i in range(len(recs) - 1, -1, -1):
        L, (wt, b) = recs[i], W[i]
        shape, cols, pre, first = keep[i]
        ph, pw = L["p"]
        oh, ow, oc = pre.shape[1:]
        Ph, Pw = oh // ph, ow // pw
        d = d.reshape(n, Ph, Pw, oc)
        dwin = np.zeros((n, Ph, Pw, oc, ph * pw))
        np.put_along_axis(dwin, first[..., None], d[..., None], -1)
        dy = np.zeros_like(pre)
        dy[:, :Ph * ph, :Pw * pw] = dwin.reshape(n, Ph, Pw, oc, ph, pw).transpose(0, 1, 4, 2, 5, 3).reshape(n, Ph * ph, Pw * pw, oc)
        if L["relu"]:
            dy = dy * (pre > 0.0)
        grads[i] = dict(w=np.einsum("nhwc,nhwk->ck", dy, cols).reshape(wt.shape), b=dy.sum(axis=(0, 1, 2)))
        if i == 0:
            break
        dcols = dy @ wt.reshape(oc, -1)                                # [n][oh][ow][K]
        kh, kw = L["k"]
        sh, sw = L["s"]
        ic = L["inp"][2]
        dx = np.zeros(shape)
        for ky in range(kh):
            for kx in range(kw):
                k0 = (ky * kw + kx) * ic
                dx[:, ky:ky + sh * oh:sh, kx:kx + sw * ow:sw, :] += dcols[..., k0:k0 + ic]
        d = dx
    return dict(loss=loss, logits=z, argmax=np.argmax(z, axis=1).astype(np.int32), grads=grads)


def torch_grads(model, x, labels, dtype, weights=None):
    """The same through torch's CPU autograd (conv2d / relu / max_pool2d / cross_entropy) in `dtype`: dict(loss [n], logits, grads) as
    numpy float64 arrays in the model dict's layout."""
    import torch
    import torch.nn.functional as F
    recs = conv_records(model)
    W = _weights64(model, weights)
    h, w, c = model["in_shape"]
    a = torch.tensor(np.asarray(x, np.float64).reshape(-1, h, w, c), dtype=dtype).permute(0, 3, 1, 2)
    params = []
    for L, (wt, b) in zip(recs, W):
        tw = torch.tensor(wt, dtype=dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)   # [out][in][kh][kw]
        tb = torch.tensor(b, dtype=dtype).requires_grad_(True)
        params.append((tw, tb))
        ih, iw, ic = L["inp"]
        a = a.permute(0, 2, 3, 1).reshape(-1, ih, iw, ic).permute(0, 3, 1, 2)
        a = F.conv2d(a, tw, tb, stride=tuple(L["s"]))
        if L["relu"]:
            a = F.relu(a)
        if tuple(L["p"]) != (1, 1):
            a = F.max_pool2d(a, tuple(L["p"]))
    z = a.permute(0, 2, 3, 1).reshape(a.shape[0], -1)
    rows = F.cross_entropy(z, torch.tensor(np.asarray(labels).reshape(-1), dtype=torch.long), reduction="none")
    rows.mean().backward()
    grads = [dict(w=tw.grad.permute(0, 2, 3, 1).double().numpy().copy(), b=tb.grad.double().numpy().copy()) for tw, tb in params]
    return dict(loss=rows.detach().double().numpy(), logits=z.detach().double().numpy(), grads=grads)


def tensor_error(got, want):
    """The GPU test's metric for one tensor: max |g - g64| / max |g64| (max |g| where g64 is all zero; 0 when both are)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    return 0.0 if err == 0.0 else err / scale if scale > 0 else np.inf


def terms(model, n):
    """Per conv record, how many terms the sums behind one element of dW and of db have at most: n rows x the conv positions."""
    out = []
    for L in conv_records(model):
        ph, pw = L["p"]
        out.append(n * L["out"][0] * ph * L["out"][1] * pw)
    return out


# ---- the trainer's plan and the order of its sums ---------------------------------------------------------------------------------
def train_lds_bytes(plan, batch):
    """ed_ftrain_lds_bytes of a restated plan (fnet_exact.plan) at `batch` utterances per workgroup: the larger of the forward half's
    LDS and the backward half's dY [16-padded batch x rows][n_pad] floats + row bases [16-padded batch x rows] ints, each the largest
    record's (ftrain_size_lds)."""
    fwd = 4 * (batch * sum(plan["buf_n"]) + plan["w_lds"]) + 4 * plan["k_lds"]
    mp = [(batch * L["rows"] + 15) // 16 * 16 for L in plan["layers"]]
    bwd = 4 * max(m * L["n_pad"] for m, L in zip(mp, plan["layers"])) + 4 * max(mp)
    return max(fwd, bwd)


def train_batch(plan, limit=None):
    """The utterances per workgroup edison_ftrain_create trains a restated plan at: the network's own batch, lowered while the training
    workgroup does not fit `limit` bytes of LDS (fnet_exact.LDS_BYTES); 0 for a plan it refuses, whose one utterance does not fit."""
    limit = fnet_exact.LDS_BYTES if limit is None else limit
    batch = plan["batch"]
    while batch > 1 and train_lds_bytes(plan, batch) > limit:
        batch -= 1
    return batch if train_lds_bytes(plan, batch) <= limit else 0


def fold_tiles(T, grid, scale):
    """The order ed_ftrain_grad_kernel and ed_ftrain_reduce_kernel sum a call's tiles in, in float32: T [n_tiles][w_floats] float32,
    tile j's packed gradient; workgroup g's slab is T[g] scale, then + T[g + grid] scale, then + T[g + 2 grid] scale ...; the result
    is slab 0 + slab 1 + ... in index order over the min(n_tiles, grid) slabs. `scale` is a power of two, so T scale is exact."""
    T = np.asarray(T)
    assert T.dtype == np.float32 and T.ndim == 2 and len(T) >= 1 and grid >= 1
    s = np.float32(scale)
    assert float(s) == float(scale) and np.frexp(s)[0] == 0.5, "scale is not a power of two that float32 holds"
    used = min(len(T), grid)
    slabs = T[:used] * s
    for j0 in range(grid, len(T), grid):
        part = T[j0:j0 + grid]
        slabs[:len(part)] += part * s
    out = slabs[0].copy()
    for g in range(1, used):
        out += slabs[g]
    assert out.dtype == np.float32
    return out


# ---- Adam as Keras states it ------------------------------------------------------------------------------------------------------
class Adam:
    """t from 1: m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g g, w -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps), float64, over
    any list of arrays."""

    def __init__(self, b1=0.9, b2=0.999, eps=1e-7):
        self.b1, self.b2, self.eps, self.t, self.m, self.v = b1, b2, eps, 0, None, None

    def step(self, ws, gs, lr):
        """ws, gs: lists of float64 arrays; ws is updated in place."""
        if self.m is None:
            self.m, self.v = [np.zeros_like(w) for w in ws], [np.zeros_like(w) for w in ws]
        self.t += 1
        f = lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        for w, g, m, v in zip(ws, gs, self.m, self.v):
            m *= self.b1
            m += (1.0 - self.b1) * g
            v *= self.b2
            v += (1.0 - self.b2) * g * g
            w -= f * m / (np.sqrt(v) + self.eps)


class HostTrainer:
    """The GPU trainer's grad / step in float64 on the host, for edison_amd.train.fit to drive: the replay the GPU's fit is held to."""

    def __init__(self, model):
        self.model = model
        self.weights = [dict(w=w.copy(), b=b.copy()) for w, b in _weights64(model, None)]
        self.adam = Adam()
        self._g = None

    def grad(self, x, y):
        r = loss_grad(self.model, x, y, weights=self.weights)
        self._g = r["grads"]
        return dict(loss=r["loss"], argmax=r["argmax"])

    def step(self, lr):
        ws = [t[k] for t in self.weights for k in ("w", "b")]
        gs = [t[k] for t in self._g for k in ("w", "b")]
        self.adam.step(ws, gs, lr)


# ---- the synthetic data set of the fit tests --------------------------------------------------------------------------------------
FIT_ROW, FIT_CLASSES, FIT_ROWS, FIT_NOISE = "pool21_trunc_h", 3, 96, 0.3
FIT_STEPS, FIT_BATCH, FIT_LR = 40, 32, 0.01


def fit_set():
    """Three classes on pool21_trunc_h's input shape: a fixed N(0, 1) pattern per class + N(0, 0.3), 96 rows, labels i % 3."""
    h, w, c = fnet_sweep.model(FIT_ROW)["in_shape"]
    rng = np.random.default_rng(2024)
    pattern = rng.normal(0, 1, (FIT_CLASSES, h * w * c))
    y = (np.arange(FIT_ROWS) % FIT_CLASSES).astype(np.int32)
    x = (pattern[y] + rng.normal(0, FIT_NOISE, (FIT_ROWS, h * w * c))).astype(np.float32)
    return x, y

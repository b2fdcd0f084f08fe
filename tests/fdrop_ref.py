"""Dropout in the float32 trainer (csrc/fnet_dropout.h, edison_ftrain_set_dropout): a numpy restatement of the mask
and of training with it. Test infrastructure, not a test: tests/test_fdrop_cpu.py holds it to Philox's known answers, to a stand-alone
host program on the header, to torch's float64 autograd and to central differences; tests/test_gpu_ftrain_dropout.py holds the kernels
to it.

The mask. Element e of record l is kept for sample u of training call `call` under `seed` iff fmix32(fmix32(e ^ kA) + kB) >= T, with
(kA, kB) words 0 and 1 of Philox4x32-10 at counter (u, call & 0xffffffff, call >> 32, l) and key (seed & 0xffffffff, seed >> 32), and
T = floor(rate 2^32 + 0.5). A kept value is multiplied by s = float32(1 / (1 - rate)), a dropped one is +0.0f. After the pool
e = q out_c + c; before the pool e = r out_c + c with r = q P + element the plan's output row, absent rows counted. A record without a
pool has one position.

Written differently from the kernel: the mask is built as whole 0 / s factor tensors in the image's layout and multiplied in, where
the kernel hashes per element in its accumulator layout."""
import os

import numpy as np

from edison_amd import cube_import, train

import fgrad_pad_ref as gp
import fgrad_ref
import fnet_pad
import fnet_sweep

M32 = np.uint64(0xffffffff)


# ---- the mask -----------------------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """Philox4x32-10: ctr 4 and key 2 words (ints or equal-shaped integer arrays) -> 4 uint64 arrays holding 32-bit words."""
    c = [np.asarray(v, np.uint64) & M32 for v in np.broadcast_arrays(*[np.asarray(v, np.uint64) for v in ctr])]
    k = [np.asarray(v, np.uint64) & M32 for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & M32, (k[1] + np.uint64(0xBB67AE85)) & M32]
    return c


def keys(seed, call, u, l):
    """(kA, kB) of samples u (array) and record l: uint32 arrays."""
    seed, call = int(seed), int(call)
    u = np.asarray(u, np.uint64)
    w = philox4x32_10([u, np.uint64(call & 0xffffffff), np.uint64(call >> 32), np.uint64(l)], [np.uint64(seed & 0xffffffff), np.uint64(seed >> 32)])
    return w[0].astype(np.uint32), w[1].astype(np.uint32)


def fmix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85ebca6b)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xc2b2ae35)
    x ^= x >> np.uint32(16)
    return x


def threshold(rate):
    return min(int(np.floor(float(rate) * 4294967296.0 + 0.5)), 0xffffffff)


def scale(rate):
    return np.float32(1.0 / (1.0 - float(rate)))


def hashes(seed, call, u, l, e):
    """h of samples u [n] x elements e [m]: uint32 [n][m]."""
    kA, kB = keys(seed, call, np.asarray(u).reshape(-1), l)
    with np.errstate(over="ignore"):
        return fmix32(fmix32(np.asarray(e, np.uint32).reshape(1, -1) ^ kA[:, None]) + kB[:, None])


def keep(seed, call, u, l, e, rate):
    """Is element e of record l kept for sample u (scalars) -> bool."""
    return bool(hashes(seed, call, [u], l, [e])[0, 0] >= np.uint32(threshold(rate)))


def kept(seed, call, n, l, m, rate, u0=0):
    """The keep bits of elements 0 .. m - 1 of record l for samples u0 .. u0 + n - 1: bool [n][m]."""
    return hashes(seed, call, np.arange(u0, u0 + n), l, np.arange(m)) >= np.uint32(threshold(rate))


# ---- a dropout setting on a model ---------------------------------------------------------------------------------------------------
def spec(model, dropout, before_pool=None):
    """train.dropout_spec on the model's records: [(rate, before)] with before only where the record has a pool."""
    rates, before = train.dropout_spec(dropout, before_pool)
    recs = gp.conv_records(model)
    assert len(rates) == len(recs) and rates[-1] == 0.0
    return [(r, bool(b) and L["p"][0] * L["p"][1] > 1) for r, b, L in zip(rates, before, recs)]


def factors(model, sp, seed, call, n):
    """Per record None (rate 0) or dict(before, rows [n][rows][oc] or [n][Ph Pw][oc]: 0 / s float32 in the plan's element order, keep:
    the same as bool, image: float64 in the layout loss_grad multiplies it in: [n][conv_h][conv_w][oc] before the pool (1 where
    the pool's floor reads nothing), [n][Ph][Pw][oc] behind it)."""
    out = []
    for l, (L, (rate, before)) in enumerate(zip(gp.conv_records(model), sp)):
        if rate == 0.0:
            out.append(None)
            continue
        (ph, pw), (Ph, Pw, oc) = L["p"], L["out"]
        P = ph * pw
        rows = Ph * Pw * (P if before else 1)
        k = kept(seed, call, n, l, rows * oc, rate).reshape(n, rows, oc)
        f = np.where(k, scale(rate), np.float32(0)).astype(np.float32)
        if before:
            ch, cw = fnet_pad.conv_map(L)
            pp = fnet_pad.pads(L)[1]
            bordered = np.ones((n, ch + pp[0] + pp[2], cw + pp[1] + pp[3], oc))
            bordered[:, :Ph * ph, :Pw * pw] = f.astype(np.float64).reshape(n, Ph, Pw, ph, pw, oc).transpose(0, 1, 3, 2, 4, 5).reshape(n, Ph * ph, Pw * pw, oc)
            image = bordered[:, pp[0]:pp[0] + ch, pp[1]:pp[1] + cw]
        else:
            image = f.astype(np.float64).reshape(n, Ph, Pw, oc)
        out.append(dict(before=before, rows=f, keep=k, image=image))
    return out


# ---- the bit-exact host model with the mask -----------------------------------------------------------------------------------------
def forward32(model, x, sp, seed, call, detail=False):
    """The kernel's forward half with dropout: every record's stored output [n][out_n] float32, bit for bit (the last is the logits).
    fnet_pad.pre_activation's values are the GPU's; ReLU, the mask, x s in float32 and the pool follow them. detail=True: per record
    also (first [n][Ph Pw][oc], positive [n][rows][oc], dropped [n][Ph Pw][oc]: the winner, or the pooled output, was dropped)."""
    a = np.asarray(x, np.float32)
    n = len(a)
    outs, det = [], []
    for L, F in zip(gp.conv_records(model), factors(model, sp, seed, call, n)):
        Ph, Pw, oc = L["out"]
        P = L["p"][0] * L["p"][1]
        v, live = fnet_pad.pre_activation(L, a)
        pos = v > 0
        if L["relu"]:
            v = np.maximum(v, np.float32(0))
        if F is not None and F["before"]:
            k = F["keep"].reshape(-1, oc)
            v = np.where(k, v * F["rows"].reshape(-1, oc), np.float32(0)).astype(np.float32)
        v = np.where(live[:, None], v, np.float32(-np.inf)).reshape(-1, P, oc)
        first = v.argmax(axis=1)
        out = v.max(axis=1)
        dropped = np.zeros(out.shape, bool)
        if F is not None and F["before"]:
            dropped = ~np.take_along_axis(F["keep"].reshape(-1, P, oc), first[:, None, :], 1)[:, 0]
        elif F is not None:
            k = F["keep"].reshape(-1, oc)
            out = np.where(k, out * F["rows"].reshape(-1, oc), np.float32(0)).astype(np.float32)
            dropped = ~k
        a = out.reshape(n, -1).astype(np.float32)
        outs.append(a)
        det.append((first.reshape(n, -1, oc), pos.reshape(n, -1, oc), dropped.reshape(n, -1, oc)))
    return (outs, det) if detail else outs


# ---- the float64 restatement --------------------------------------------------------------------------------------------------------
def loss_grad(model, x, labels, sp, seed, call, weights=None, n_total=None, detail=False):
    """fgrad_pad_ref.loss_grad with the mask as a constant 0 / s factor at the chosen position: before the pool on the activation map
    (then the first maximum is taken of the masked map), or on the pooled output. Where every rate is 0 no factor is applied and it is
    that function. detail=True adds per record dict(pre, first, dy, dropped [n][Ph][Pw][oc])."""
    recs = gp.conv_records(model)
    W = fgrad_ref._weights64(model, weights)
    labels = np.asarray(labels).reshape(-1)
    h, w, c = model["in_shape"]
    a = np.asarray(x, np.float64).reshape(-1, h, w, c)
    n = a.shape[0]
    n_total = n if n_total is None else n_total
    Fs = factors(model, sp, seed, call, n)
    keepers = []
    for L, (wt, b), F in zip(recs, W, Fs):
        cp, pp = fnet_pad.pads(L)
        a = a.reshape((-1,) + tuple(L["inp"]))
        cols = fgrad_ref._cols(L, gp._border(a, cp, 0.0))
        pre = cols @ wt.reshape(wt.shape[0], -1).T + b
        act = np.maximum(pre, 0.0) if L["relu"] else pre
        if F is not None and F["before"]:
            act = act * F["image"]
        ph, pw = L["p"]
        Ph, Pw, oc = L["out"]
        bordered = gp._border(act, pp, -np.inf)
        win = bordered[:, :Ph * ph, :Pw * pw].reshape(n, Ph, ph, Pw, pw, oc).transpose(0, 1, 3, 5, 2, 4).reshape(n, Ph, Pw, oc, ph * pw)
        first = win.argmax(axis=-1)
        keepers.append((a.shape, cols, pre, first, bordered.shape))
        a = np.take_along_axis(win, first[..., None], -1)[..., 0]
        assert np.isfinite(a).all()
        if F is not None and not F["before"]:
            a = a * F["image"]
    z = a.reshape(n, -1)
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    s = e.sum(axis=1, keepdims=True)
    loss = np.log(s[:, 0]) + mx[:, 0] - z[np.arange(n), labels]
    d = e / s
    probs = d.copy()
    d[np.arange(n), labels] -= 1.0
    d = d / n_total
    grads, details = [None] * len(recs), [None] * len(recs)
    for i in range(len(recs) - 1, -1, -1):
        L, (wt, b), F = recs[i], W[i], Fs[i]
        cp, pp = fnet_pad.pads(L)
        shape, cols, pre, first, bshape = keepers[i]
        ph, pw = L["p"]
        Ph, Pw, oc = L["out"]
        ch, cw = pre.shape[1:3]
        d = d.reshape(n, Ph, Pw, oc)
        dropped = np.zeros(d.shape, bool)
        if F is not None and not F["before"]:
            d = d * F["image"]
            dropped = F["image"] == 0
        dwin = np.zeros((n, Ph, Pw, oc, ph * pw))
        np.put_along_axis(dwin, first[..., None], d[..., None], -1)
        dyb = np.zeros(bshape)
        dyb[:, :Ph * ph, :Pw * pw] = dwin.reshape(n, Ph, Pw, oc, ph, pw).transpose(0, 1, 4, 2, 5, 3).reshape(n, Ph * ph, Pw * pw, oc)
        dy = dyb[:, pp[0]:pp[0] + ch, pp[1]:pp[1] + cw]
        assert np.count_nonzero(dyb) == np.count_nonzero(dy)
        if F is not None and F["before"]:
            dy = dy * F["image"]
            fb = gp._border(F["image"], pp, 1.0)[:, :Ph * ph, :Pw * pw].reshape(n, Ph, ph, Pw, pw, oc).transpose(0, 1, 3, 5, 2, 4).reshape(n, Ph, Pw, oc, ph * pw)
            dropped = np.take_along_axis(fb, first[..., None], -1)[..., 0] == 0
        if L["relu"]:
            dy = dy * (pre > 0.0)
        grads[i] = dict(w=np.einsum("nhwc,nhwk->ck", dy, cols).reshape(wt.shape), b=dy.sum(axis=(0, 1, 2)))
        details[i] = dict(pre=pre, first=first, dy=dy, dropped=dropped)
        if i == 0:
            break
        dcols = dy @ wt.reshape(oc, -1)
        kh, kw = L["k"]
        sh, sw = L["s"]
        ih, iw, ic = L["inp"]
        dxb = np.zeros((n, ih + cp[0] + cp[2], iw + cp[1] + cp[3], ic))
        for ky in range(kh):
            for kx in range(kw):
                k0 = (ky * kw + kx) * ic
                dxb[:, ky:ky + sh * ch:sh, kx:kx + sw * cw:sw, :] += dcols[..., k0:k0 + ic]
        d = dxb[:, cp[0]:cp[0] + ih, cp[1]:cp[1] + iw]
    out = dict(loss=loss, logits=z, argmax=np.argmax(z, axis=1).astype(np.int32), grads=grads, probs=probs)
    if detail:
        out["detail"] = details
    return out


def torch_grads(model, x, labels, dtype, sp, seed, call, weights=None):
    """fgrad_pad_ref.torch_grads with the factor tensors multiplied in."""
    import torch
    import torch.nn.functional as F
    recs = gp.conv_records(model)
    W = fgrad_ref._weights64(model, weights)
    h, w, c = model["in_shape"]
    a = torch.tensor(np.asarray(x, np.float64).reshape(-1, h, w, c), dtype=dtype).permute(0, 3, 1, 2)
    n = a.shape[0]
    params = []
    for L, (wt, b), fac in zip(recs, W, factors(model, sp, seed, call, n)):
        cp, pp = fnet_pad.pads(L)
        tw = torch.tensor(wt, dtype=dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        tb = torch.tensor(b, dtype=dtype).requires_grad_(True)
        params.append((tw, tb))
        ih, iw, ic = L["inp"]
        a = a.permute(0, 2, 3, 1).reshape(-1, ih, iw, ic).permute(0, 3, 1, 2)
        a = F.conv2d(F.pad(a, (cp[1], cp[3], cp[0], cp[2]), value=0.0), tw, tb, stride=tuple(L["s"]))
        if L["relu"]:
            a = F.relu(a)
        ft = None if fac is None else torch.tensor(fac["image"], dtype=dtype).permute(0, 3, 1, 2)
        if fac is not None and fac["before"]:
            a = a * ft
        if tuple(L["p"]) != (1, 1):
            a = F.max_pool2d(F.pad(a, (pp[1], pp[3], pp[0], pp[2]), value=float("-inf")), tuple(L["p"]))
        if fac is not None and not fac["before"]:
            a = a * ft
    z = a.permute(0, 2, 3, 1).reshape(a.shape[0], -1)
    rows = F.cross_entropy(z, torch.tensor(np.asarray(labels).reshape(-1), dtype=torch.long), reduction="none")
    rows.mean().backward()
    grads = [dict(w=tw.grad.permute(0, 2, 3, 1).double().numpy().copy(), b=tb.grad.double().numpy().copy()) for tw, tb in params]
    return dict(loss=rows.detach().double().numpy(), logits=z.detach().double().numpy(), grads=grads)


class HostTrainer(fgrad_ref.HostTrainer):
    """The float64 host trainer with the GPU trainer's counter rule: a training call masks with the current counter, then advances it;
    training=False masks nothing and leaves it."""

    def __init__(self, model, dropout, before_pool=None, seed=0):
        super().__init__(model)
        self.sp, self.seed, self.call = spec(model, dropout, before_pool), int(seed), 0
        self.none = [(0.0, False)] * len(self.sp)

    def dropout(self):
        return dict(rates=[r for r, _ in self.sp], before_pool=[int(b) for _, b in self.sp], seed=self.seed, call=self.call,
                    on=any(r > 0 for r, _ in self.sp))

    def grad(self, x, y, training=True):
        on = training and self.dropout()["on"]
        r = loss_grad(self.model, x, y, self.sp if on else self.none, self.seed, self.call, weights=self.weights)
        self.call += int(on)
        self._g = r["grads"]
        return dict(loss=r["loss"], argmax=r["argmax"])


# ---- the rows of the GPU test -------------------------------------------------------------------------------------------------------
N_ROWS = 17
SHIPPED = "cube_kws"
# name -> (source: "sweep" (fnet_sweep), "pad" (fgrad_pad_ref) or "shipped", the row there, dropout, seed of the masks)
ROWS = {
    "p1_inc3": ("sweep", "inc3_oc64_oc65_s21", None, 11),                       # P = 1 everywhere: the two positions coincide
    "p2_pool12_no_relu_before": ("sweep", "pool12_trunc_w", [(0.25, 1), 0], 12),   # P = 2 without ReLU: the dropped-winner bit decides
    "p4_pool22_before": ("sweep", "pool22_trunc_hw", [(0.5, 1), 0], 13),          # P = 4, 17 channels: two channel tiles
    "p4_pool22_after": ("sweep", "pool22_trunc_hw", [(0.25, 0), 0], 14),
    "pool21_before": ("sweep", "pool21_trunc_h", [(0.25, 1), 0], 15),
    "pool21_after": ("sweep", "pool21_trunc_h", [(0.5, 0), 0], 16),
    "neg_no_relu_before": ("pad", gp.NEG_T, [(0.25, 1), 0], 17),
    "mid_pads_batch": ("pad", "mid_pads_batch", [0.25, 0.5, (0.25, 1), 0], 18),
    "simple_conv": ("pad", "simple_conv", train.KERAS_DROPOUT["simple_conv"], 19),
    "medium_embedding_conv": ("pad", "medium_embedding_conv", train.KERAS_DROPOUT["medium_embedding_conv"], 20),
    "batch5": ("sweep", "batch5", [0.25, (0.5, 1), 0], 21),
    "shipped_kws_conv": ("shipped", SHIPPED, train.KERAS_DROPOUT["kws_conv"], 116),   # a trained network is sure of itself: most seeds leave a probability below 1e-4
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CASES = {}


def case(name):
    """Row `name` -> dict(model, blob, dropout, seed, x [17][in_n], y [17]), built once. The padded rows' inputs are fgrad_pad_ref.data's, the others' N(0, 1)."""
    if name in _CASES:
        return _CASES[name]
    kind, row, dropout, seed = ROWS[name]
    if kind == "pad":
        model, blob = gp.model(row), gp.blob(row)
        x, y = gp.data(row, N_ROWS)
    else:
        if kind == "shipped":
            with open(os.path.join(GOLDEN, "cube_kws.ednf"), "rb") as f:
                blob = f.read()
        else:
            blob = fnet_sweep.blob(row)
        model = cube_import.read_blob(blob)
        # N(0, 1), as fgrad_pad_ref.data draws: fnet_sweep's own input sets and the shipped network's features saturate the softmax
        x = np.random.default_rng(6000 + seed).normal(0, 1, (N_ROWS, int(np.prod(model["in_shape"])))).astype(np.float32)
        n_out = int(np.prod(gp.conv_records(model)[-1]["out"]))
        y = (np.arange(N_ROWS) % n_out).astype(np.int32)
    if dropout is None:                                                        # every record but the last, rates 0.25 and 0.5 in turn
        nl = len(gp.conv_records(model))
        dropout = [(0.25, 0.5)[i % 2] for i in range(nl - 1)] + [0]
    _CASES[name] = dict(model=model, blob=blob, dropout=dropout, seed=seed, x=x, y=y, sp=spec(model, dropout))
    return _CASES[name]


_REFS = {}


def reference(name, call=0):
    """loss_grad (float64, detail) of row `name` at counter `call`, computed once and shared."""
    if (name, call) not in _REFS:
        c = case(name)
        _REFS[name, call] = loss_grad(c["model"], c["x"], c["y"], c["sp"], c["seed"], call, detail=True)
    return _REFS[name, call]

"""BatchNorm in the float32 trainer (csrc/fnet_bn_kernels.hip, edison_ftrain_set_batchnorm): a numpy restatement
of a training call with BatchNorm, of the fold into the inference-mode network, of the moving statistics and of a host trainer. Test
infrastructure, not a test: tests/test_fbn_cpu.py holds it to torch's float64 autograd and to central differences,
tests/test_gpu_ftrain_bn.py holds the kernels to it.

The definition. A BatchNorm record is conv + bias = z -> BatchNorm -> ReLU -> dropout -> max pool. For a call of n rows,
N = n x conv_out_h x conv_out_w over the WHOLE conv map, the positions a floor-mode pool drops included: mean = sum z / N,
var = sum (z - mean)^2 / N, zhat = (z - mean) rstd with rstd = 1 / sqrt(var + eps), y = gamma zhat + beta. Backward: dy as without
BatchNorm (a truncated position gets 0), dbeta = sum dy, dgamma = sum dy zhat, dz = gamma rstd (dy - dbeta / N - zhat dgamma / N), which
is non-zero on truncated positions too; dW and dX from dz. The conv bias gradient of a BatchNorm record is reported as 0 (sum dz = 0
in exact arithmetic; "b_sum" keeps the rounding noise for the comparison with autograd). Moving statistics: mm = m mm + (1 - m) mean
and the same for the population variance (unbiased: var N / (N - 1)). Fold: W' = W s, b' = (b - mm) s + beta, s = gamma / sqrt(mv + eps).

Written differently from the kernels: whole tensors in the image's layout, statistics by numpy's mean over centred values, where the
kernels merge per-workgroup moments by Chan's formula over rows in the plan's order."""
import os

import numpy as np

from edison_amd import cube_import, train

import fdrop_ref as fd
import fgrad_ref
import fnet_sweep

MOMENTUM, EPS_BN = train.BN_MOMENTUM, train.BN_EPS


def conv_records(model):
    return fgrad_ref.conv_records(model)


def initial_state(model, has_bn, dtype=np.float64):
    """Per record None or dict(gamma 1, beta 0, mean 0, var 1)."""
    return [dict(gamma=np.ones(L["out"][2], dtype), beta=np.zeros(L["out"][2], dtype), mean=np.zeros(L["out"][2], dtype), var=np.ones(L["out"][2], dtype))
            if h else None for L, h in zip(conv_records(model), has_bn)]


def loss_grad(model, x, labels, state, eps=EPS_BN, sp=None, seed=0, call=0, weights=None, trunc_in_stats=True, dtype=np.float64, detail=False):
    """One training call. state: per record None or dict(gamma, beta, ..) (initial_state's form). sp: fdrop_ref.spec's dropout (None: off).
    Returns dict(loss [n], logits, argmax, probs, grads [dict(w, b, b_sum)], bn [None | dict(gamma, beta: the gradients, mean, var: the
    batch statistics, N)]) in `dtype`. trunc_in_stats=False is the MISTAKE of leaving the truncated positions out of the statistics and of
    dz, kept so that a test can show the right rule is visible. detail=True adds per record dict(y: the map behind BatchNorm, first)."""
    recs = conv_records(model)
    W = [(np.asarray(w, dtype), np.asarray(b, dtype)) for w, b in fgrad_ref._weights64(model, weights)]
    labels = np.asarray(labels).reshape(-1)
    h, w, c = model["in_shape"]
    a = np.asarray(x, dtype).reshape(-1, h, w, c)
    n = a.shape[0]
    sp = [(0.0, False)] * len(recs) if sp is None else sp
    Fs = fd.factors(model, sp, seed, call, n)
    eps = dtype(eps)
    keep, details = [], []
    for L, (wt, b), F, st in zip(recs, W, Fs, state):
        a = a.reshape((-1,) + tuple(L["inp"]))
        cols = fgrad_ref._cols(L, a)
        z = cols @ wt.reshape(wt.shape[0], -1).T + b
        ph, pw = L["p"]
        Ph, Pw, oc = L["out"]
        bn = None
        y = z
        if st is not None:
            region = z if trunc_in_stats else z[:, :Ph * ph, :Pw * pw]
            N = region.size // oc
            mean = region.mean(axis=(0, 1, 2), dtype=dtype)
            var = ((region - mean) ** 2).mean(axis=(0, 1, 2), dtype=dtype)
            rstd = dtype(1) / np.sqrt(var + eps)
            zhat = (z - mean) * rstd
            y = np.asarray(st["gamma"], dtype) * zhat + np.asarray(st["beta"], dtype)
            bn = dict(mean=mean, var=var, rstd=rstd, zhat=zhat, N=N, gamma=np.asarray(st["gamma"], dtype))
        act = np.maximum(y, dtype(0)) if L["relu"] else y
        if F is not None and F["before"]:
            act = act * F["image"].astype(dtype)
        win = act[:, :Ph * ph, :Pw * pw].reshape(n, Ph, ph, Pw, pw, oc).transpose(0, 1, 3, 5, 2, 4).reshape(n, Ph, Pw, oc, ph * pw)
        first = win.argmax(axis=-1)
        keep.append((a.shape, cols, y, first, bn))
        details.append(dict(y=y, first=first, win=win))
        a = np.take_along_axis(win, first[..., None], -1)[..., 0]
        if F is not None and not F["before"]:
            a = a * F["image"].astype(dtype)
    z = a.reshape(n, -1)
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    s = e.sum(axis=1, keepdims=True)
    loss = np.log(s[:, 0]) + mx[:, 0] - z[np.arange(n), labels]
    d = e / s
    probs = d.copy()
    d[np.arange(n), labels] -= dtype(1)
    d = d / dtype(n)
    grads, bns = [None] * len(recs), [None] * len(recs)
    for i in range(len(recs) - 1, -1, -1):
        L, (wt, b), F = recs[i], W[i], Fs[i]
        shape, cols, y, first, bn = keep[i]
        ph, pw = L["p"]
        Ph, Pw, oc = L["out"]
        d = d.reshape(n, Ph, Pw, oc)
        if F is not None and not F["before"]:
            d = d * F["image"].astype(dtype)
        dwin = np.zeros((n, Ph, Pw, oc, ph * pw), dtype)
        np.put_along_axis(dwin, first[..., None], d[..., None], -1)
        dy = np.zeros_like(y)
        dy[:, :Ph * ph, :Pw * pw] = dwin.reshape(n, Ph, Pw, oc, ph, pw).transpose(0, 1, 4, 2, 5, 3).reshape(n, Ph * ph, Pw * pw, oc)
        if F is not None and F["before"]:
            dy = dy * F["image"].astype(dtype)
        if L["relu"]:
            dy = dy * (y > 0)
        dz = dy
        if bn is not None:
            dbeta = dy.sum(axis=(0, 1, 2), dtype=dtype)
            dgamma = (dy * bn["zhat"]).sum(axis=(0, 1, 2), dtype=dtype)
            dz = bn["gamma"] * bn["rstd"] * (dy - dbeta / dtype(bn["N"]) - bn["zhat"] * (dgamma / dtype(bn["N"])))
            if not trunc_in_stats:
                full = np.zeros_like(dz)
                full[:, :Ph * ph, :Pw * pw] = dz[:, :Ph * ph, :Pw * pw]
                dz = full
            bns[i] = dict(gamma=dgamma, beta=dbeta, mean=bn["mean"], var=bn["var"], N=bn["N"])
        bsum = dz.sum(axis=(0, 1, 2), dtype=dtype)
        grads[i] = dict(w=np.einsum("nhwc,nhwk->ck", dz, cols).reshape(wt.shape), b=np.zeros_like(bsum) if bn is not None else bsum, b_sum=bsum)
        if i == 0:
            break
        dcols = dz @ wt.reshape(oc, -1)
        kh, kw = L["k"]
        sh, sw = L["s"]
        ic = L["inp"][2]
        ch, cw = y.shape[1:3]
        dx = np.zeros(shape, dtype)
        for ky in range(kh):
            for kx in range(kw):
                k0 = (ky * kw + kx) * ic
                dx[:, ky:ky + sh * ch:sh, kx:kx + sw * cw:sw, :] += dcols[..., k0:k0 + ic]
        d = dx
    out = dict(loss=loss, logits=z, argmax=np.argmax(z, axis=1).astype(np.int32), grads=grads, bn=bns, probs=probs)
    if detail:
        out["detail"] = details
    return out


def moved(state, bns, momentum=MOMENTUM, unbiased=False):
    """The moving statistics after a training call whose batch statistics are bns (loss_grad's "bn"): a new state list, float64."""
    out = []
    for st, b in zip(state, bns):
        if st is None:
            out.append(None)
            continue
        var = np.asarray(b["var"], np.float64) * (b["N"] / (b["N"] - 1.0) if unbiased else 1.0)
        out.append(dict(gamma=st["gamma"], beta=st["beta"], mean=momentum * np.asarray(st["mean"], np.float64) + (1.0 - momentum) * np.asarray(b["mean"], np.float64),
                        var=momentum * np.asarray(st["var"], np.float64) + (1.0 - momentum) * var))
    return out


def fold(weights, state, eps=EPS_BN):
    """[dict(w, b)] master weights and the state -> the inference-mode network's [dict(w, b)], float64."""
    out = []
    for t, st in zip(weights, state):
        w, b = np.asarray(t["w"], np.float64), np.asarray(t["b"], np.float64)
        if st is not None:
            s = np.asarray(st["gamma"], np.float64) / np.sqrt(np.asarray(st["var"], np.float64) + eps)
            w, b = w * s[:, None, None, None], (b - np.asarray(st["mean"], np.float64)) * s + np.asarray(st["beta"], np.float64)
        out.append(dict(w=w, b=b))
    return out


def inference(model, x, weights, state, eps=EPS_BN):
    """BatchNorm in inference mode, unfolded: the logits [n][n_out] float64 of conv -> (z - mm) / sqrt(mv + eps) gamma + beta -> ReLU -> pool."""
    recs = conv_records(model)
    h, w, c = model["in_shape"]
    a = np.asarray(x, np.float64).reshape(-1, h, w, c)
    n = a.shape[0]
    for L, t, st in zip(recs, weights, state):
        a = a.reshape((-1,) + tuple(L["inp"]))
        wt = np.asarray(t["w"], np.float64)
        z = fgrad_ref._cols(L, a) @ wt.reshape(wt.shape[0], -1).T + np.asarray(t["b"], np.float64)
        if st is not None:
            z = (z - st["mean"]) / np.sqrt(np.asarray(st["var"], np.float64) + eps) * st["gamma"] + st["beta"]
        if L["relu"]:
            z = np.maximum(z, 0.0)
        ph, pw = L["p"]
        Ph, Pw, oc = L["out"]
        a = z[:, :Ph * ph, :Pw * pw].reshape(n, Ph, ph, Pw, pw, oc).max(axis=(2, 4))
    return a.reshape(n, -1)


def torch_grads(model, x, labels, dtype, state, eps=EPS_BN, sp=None, seed=0, call=0, weights=None, momentum=MOMENTUM):
    """The same call through torch's CPU autograd: F.conv2d -> F.batch_norm(training=True) -> relu -> dropout mask -> F.max_pool2d (floor
    mode) -> cross_entropy. Returns dict(loss, logits, grads [dict(w, b)], bn [None | dict(gamma, beta: gradients, mean, var: torch's
    running statistics after the call, which use var N / (N - 1))]) as float64 arrays."""
    import torch
    import torch.nn.functional as F
    recs = conv_records(model)
    W = fgrad_ref._weights64(model, weights)
    h, w, c = model["in_shape"]
    a = torch.tensor(np.asarray(x, np.float64).reshape(-1, h, w, c), dtype=dtype).permute(0, 3, 1, 2)
    n = a.shape[0]
    sp = [(0.0, False)] * len(recs) if sp is None else sp
    params, bnp = [], []
    for L, (wt, b), fac, st in zip(recs, W, fd.factors(model, sp, seed, call, n), state):
        tw = torch.tensor(wt, dtype=dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        tb = torch.tensor(b, dtype=dtype).requires_grad_(True)
        params.append((tw, tb))
        ih, iw, ic = L["inp"]
        a = a.permute(0, 2, 3, 1).reshape(-1, ih, iw, ic).permute(0, 3, 1, 2)
        a = F.conv2d(a, tw, tb, stride=tuple(L["s"]))
        if st is None:
            bnp.append(None)
        else:
            g = torch.tensor(np.asarray(st["gamma"], np.float64), dtype=dtype).requires_grad_(True)
            be = torch.tensor(np.asarray(st["beta"], np.float64), dtype=dtype).requires_grad_(True)
            rm = torch.tensor(np.asarray(st["mean"], np.float64), dtype=dtype)
            rv = torch.tensor(np.asarray(st["var"], np.float64), dtype=dtype)
            a = F.batch_norm(a, rm, rv, g, be, training=True, momentum=1.0 - momentum, eps=eps)
            bnp.append((g, be, rm, rv))
        if L["relu"]:
            a = F.relu(a)
        ft = None if fac is None else torch.tensor(fac["image"], dtype=dtype).permute(0, 3, 1, 2)
        if fac is not None and fac["before"]:
            a = a * ft
        if tuple(L["p"]) != (1, 1):
            a = F.max_pool2d(a, tuple(L["p"]))
        if fac is not None and not fac["before"]:
            a = a * ft
    z = a.permute(0, 2, 3, 1).reshape(a.shape[0], -1)
    rows = F.cross_entropy(z, torch.tensor(np.asarray(labels).reshape(-1), dtype=torch.long), reduction="none")
    rows.mean().backward()
    grads = [dict(w=tw.grad.permute(0, 2, 3, 1).double().numpy().copy(), b=tb.grad.double().numpy().copy()) for tw, tb in params]
    bns = [None if p is None else dict(gamma=p[0].grad.double().numpy().copy(), beta=p[1].grad.double().numpy().copy(), mean=p[2].double().numpy().copy(),
                                       var=p[3].double().numpy().copy()) for p in bnp]
    return dict(loss=rows.detach().double().numpy(), logits=z.detach().double().numpy(), grads=grads, bn=bns)


class HostTrainer:
    """The float64 host trainer with BatchNorm (and dropout, fdrop_ref's counter rule) for edison_amd.train.fit to drive: Adam over the
    weights, gamma and beta; a training call moves the moving statistics; training=False runs the folded network and moves nothing."""

    def __init__(self, model, has_bn, dropout=None, seed=0, momentum=MOMENTUM, eps=EPS_BN, unbiased=False):
        self.model = model
        self.weights = [dict(w=w.copy(), b=b.copy()) for w, b in fgrad_ref._weights64(model, None)]
        self.state = initial_state(model, has_bn)
        self.sp = fd.spec(model, dropout) if dropout is not None else None
        self.seed, self.call, self.momentum, self.eps, self.unbiased = int(seed), 0, momentum, eps, unbiased
        self.adam = fgrad_ref.Adam()
        self._g = self._gbn = None

    def dropout(self):
        return dict(on=self.sp is not None and any(r > 0 for r, _ in self.sp), call=self.call)

    def batchnorm(self):
        return dict(on=True)

    def folded(self):
        return fold(self.weights, self.state, self.eps)

    def grad(self, x, y, training=True):
        if not training:
            r = fgrad_ref.loss_grad(self.model, x, y, weights=self.folded())
            self._g = self._gbn = None
            return dict(loss=r["loss"], argmax=r["argmax"])
        r = loss_grad(self.model, x, y, self.state, eps=self.eps, sp=self.sp, seed=self.seed, call=self.call, weights=self.weights)
        self.call += int(self.dropout()["on"])
        self.state = moved(self.state, r["bn"], self.momentum, self.unbiased)
        self._g, self._gbn = r["grads"], r["bn"]
        return dict(loss=r["loss"], argmax=r["argmax"])

    def step(self, lr):
        ws = [t[k] for t in self.weights for k in ("w", "b")] + [st[k] for st in self.state if st is not None for k in ("gamma", "beta")]
        gs = [np.asarray(t[k], np.float64) for t in self._g for k in ("w", "b")] + [np.asarray(b[k], np.float64) for b in self._gbn if b is not None
                                                                                    for k in ("gamma", "beta")]
        self.adam.step(ws, gs, lr)


# ---- the rows of the GPU test -------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_ROWS = 17
# name -> dict(in_shape, layers (fnet_sweep._records' form), bn, dropout, n, seed: of the inputs, chosen so that test_fbn_cpu's bound
# precondition holds, bias0: added to record 0's bias, neg: gamma and beta set through set_bn_state)
ROWS = {
    "bn_p1": dict(in_shape=(6, 5, 2), layers=[("conv", 5, (2, 2), (1, 1), (1, 1), 1), ("dense", 4, 0)], bn=[1, 0], seed=1),
    "bn_pool21_neg": dict(in_shape=(7, 5, 2), layers=[("conv", 17, (2, 2), (1, 1), (2, 1), 1), ("dense", 3, 0)], bn=[1, 0], neg=True, seed=1),
    "bn_trunc": dict(in_shape=(6, 5, 1), layers=[("conv", 6, (2, 2), (1, 1), (2, 2), 1), ("dense", 3, 0)], bn=[1, 0], seed=1),
    "bn_mixed": dict(in_shape=(12, 8, 1), layers=[("conv", 6, (3, 3), (1, 1), (2, 1), 1), ("conv", 8, (2, 2), (1, 1), (1, 1), 0),
                                                  ("conv", 5, (2, 2), (1, 1), (1, 1), 1), ("dense", 4, 0)], bn=[1, 0, 1, 0],
                     dropout=[(0.25, 1), 0, (0.25, 0), 0], seed=1),
    "bn_dense": dict(in_shape=(3, 4, 1), layers=[("dense", 6, 1), ("dense", 3, 0)], bn=[1, 0], n=2, seed=1),
    "bn_offset": dict(in_shape=(6, 5, 2), layers=[("conv", 5, (2, 2), (1, 1), (1, 1), 1), ("dense", 4, 0)], bn=[1, 0], bias0=30.0, seed=1, weights_of="bn_p1"),
    "shipped": dict(shipped=True, bn=train.KERAS_BATCHNORM["kws_conv"], dropout=train.KERAS_DROPOUT["kws_conv"], n=9, seed=1),
}
_CASES, _REFS = {}, {}


def fresh_model(name):
    """The row's model dict with fresh weights: N(0, 1) / sqrt(K) and N(0, 0.1) biases, float32."""
    row = ROWS[name]
    if row.get("shipped"):
        with open(os.path.join(GOLDEN, "cube_kws.ednf"), "rb") as f:
            shipped = cube_import.read_blob(f.read())
        in_shape = tuple(shipped["in_shape"])
        recs = [dict(L) for L in shipped["layers"]]
    else:
        in_shape = row["in_shape"]
        recs = fnet_sweep._records(in_shape, row["layers"])
        recs.append(dict(type=cube_import.T_SOFTMAX, inp=recs[-1]["out"], out=recs[-1]["out"]))
    rng = np.random.default_rng(4000 + sum(map(ord, row.get("weights_of", name))))
    for L in recs:
        if L["type"] != cube_import.T_CONV:
            continue
        oc, (kh, kw), ic = L["out"][2], L["k"], L["inp"][2]
        L["w"] = (rng.normal(0, 1, (oc, kh, kw, ic)) / np.sqrt(kh * kw * ic)).astype(np.float32)
        L["b"] = rng.normal(0, 0.1, oc).astype(np.float32)
    first = [L for L in recs if L["type"] == cube_import.T_CONV][0]
    first["b"] = (first["b"] + np.float32(row.get("bias0", 0.0))).astype(np.float32)
    return dict(in_shape=in_shape, layers=recs)


def case(name):
    """Row `name` -> dict(model, blob, bn, dropout, sp, seed, x [n][in_n] N(0, 1), y, state0: the state the test starts from), built once."""
    if name in _CASES:
        return _CASES[name]
    row = ROWS[name]
    model = fresh_model(name)
    n = row.get("n", N_ROWS)
    rng = np.random.default_rng(7000 + 100 * row["seed"] + sum(map(ord, name)))
    x = rng.normal(0, 1, (n, int(np.prod(model["in_shape"])))).astype(np.float32)
    n_out = int(np.prod(conv_records(model)[-1]["out"]))
    y = (np.arange(n) % n_out).astype(np.int32)
    state0 = initial_state(model, row["bn"], np.float32)
    if row.get("neg"):                         # half the channels with a negative gamma: the pool's winner behind BatchNorm is not the one before it
        for st in state0:
            if st is not None:
                oc = len(st["gamma"])
                st["gamma"] = (np.where(np.arange(oc) % 2, -1.0, 1.0) * rng.uniform(0.5, 1.5, oc)).astype(np.float32)
                st["beta"] = rng.normal(0, 0.3, oc).astype(np.float32)
    dropout = row.get("dropout")
    _CASES[name] = dict(model=model, blob=cube_import.build_blob(model), bn=list(row["bn"]), dropout=dropout, sp=None if dropout is None else fd.spec(model, dropout),
                        seed=40 + row["seed"], x=x, y=y, state0=state0, n=n)
    return _CASES[name]


def reference(name, call=0):
    """(loss_grad in float64 of row `name` at training call `call` (0 or 1: two consecutive calls on unchanged weights), the state after
    it), computed once and shared."""
    if (name, call) not in _REFS:
        c = case(name)
        state = c["state0"] if call == 0 else reference(name, call - 1)[1]
        r = loss_grad(c["model"], c["x"], c["y"], state, sp=c["sp"], seed=c["seed"], call=call, detail=True)
        _REFS[name, call] = (r, moved(state, r["bn"]))
    return _REFS[name, call]


def terms(model, n):
    """Per record, the terms behind one element of a gradient: n rows x the whole conv map."""
    out = []
    for L in conv_records(model):
        ch, cw = (L["inp"][0] - L["k"][0]) // L["s"][0] + 1, (L["inp"][1] - L["k"][1]) // L["s"][1] + 1
        out.append(n * ch * cw)
    return out


EPS32 = 2.0 ** -24


def bounds(name, call):
    """The GPU test's allowances on row `name` at call `call` (section 19's rule): per record dict(w, b, gamma, beta: (bound, e32)) and
    the loss's and the logits' (bound, e32). bound = 4 x the error of torch's CPU float32 autograd on the same call against the float64
    restatement, floored at 8 x 2^-24 x sqrt(terms); terms of a BatchNorm record count N. Computed once."""
    if ("bounds", name, call) in _REFS:
        return _REFS["bounds", name, call]
    import torch
    c = case(name)
    ref, _ = reference(name, call)
    state = c["state0"] if call == 0 else reference(name, call - 1)[1]
    t32 = torch_grads(c["model"], c["x"], c["y"], torch.float32, state, sp=c["sp"], seed=c["seed"], call=call)
    per = []
    for g32, g64, b32, b64, t in zip(t32["grads"], ref["grads"], t32["bn"], ref["bn"], terms(c["model"], c["n"])):
        floor = 8 * EPS32 * np.sqrt(t)
        rec = {}
        for k in ("w", "b"):
            e = fgrad_ref.tensor_error(g32[k], g64["b_sum" if k == "b" and b64 is not None else k])
            rec[k] = (max(4 * e, floor), e)
        if b64 is not None:
            for k in ("gamma", "beta"):
                e = fgrad_ref.tensor_error(b32[k], b64[k])
                rec[k] = (max(4 * e, floor), e)
        per.append(rec)
    chain = sum(int(np.prod(L["k"])) * L["inp"][2] for L in conv_records(c["model"])) + ref["logits"].shape[1]
    el, ez = fgrad_ref.tensor_error(t32["loss"], ref["loss"]), fgrad_ref.tensor_error(t32["logits"], ref["logits"])
    floor = 8 * EPS32 * np.sqrt(chain)
    _REFS["bounds", name, call] = (per, (max(4 * el, floor), el), (max(4 * ez, floor), ez))
    return _REFS["bounds", name, call]

"""Float64 restatement of training a float network (edison_amd/train.py, csrc/fnet_grad_kernels.hip, csrc/fnet_bn_kernels.hip,
csrc/fnet_data_kernels.hip) on fnet_host's conventions: the loss and its gradient with respect to
every weight and bias in the model dict's layout, with 'same' pads, dropout and BatchNorm as options of ONE function; the same network
through torch's autograd; the bound the GPU tests allow; the trainer's plan and the order of its sums; Adam and Adadelta as Keras states
them; and a host trainer that edison_amd.train.fit and fit_data drive like the GPU one. Test infrastructure, not a test: the CPU
suites (test_fgrad_cpu, test_fgrad_pad_cpu, test_fdrop_cpu, test_fbn_cpu, test_ftrain_zoo_cpu) hold it to torch's float64 autograd and
to central differences, the test_gpu_ftrain* suites hold the kernels to it. The dropout mask itself is tests/fdrop_ref.py's, the rows of
the suites tests/ftrain_rows.py's.

The definition. For n inputs and labels y, logits z: loss_u = logsumexp(z_u) - z_u[y_u], L = (1 / n_total) sum loss_u,
dL/dz_u = (softmax(z_u) - onehot(y_u)) / n_total. Backward through a record: the pool's gradient goes to the FIRST maximum of the
window in element order e = ey pw + ex (numpy's argmax), conv positions the pool's floor truncates get none; ReLU' is 1 where the
pre-activation is > 0, else 0; dW[out][k] = sum over positions and inputs of cols[.., k] dY[.., out]; dX by scattering dY W back
through the windows (input elements no window reads get 0). No probability clip (Keras's 1e-7 is not reproduced).

Written differently from the kernel on purpose: the conv runs over a zero-bordered copy of its input and the pool over a -inf-bordered
copy of the conv's map, where the kernel works on the dense images with a predicate per tap and per row. The pool's gradient goes to
the first maximum of the bordered window in element order (numpy's argmax): an absent element is -inf and every window has a present
one, so that is the first maximum among the present elements. dX is cropped back from the bordered gradient, dW comes from the
bordered columns (a tap outside the image is the operand 0 and adds nothing). Without pads the borders are empty.

Dropout (section 19b): the mask is a constant 0 / s factor (fdrop_ref.factors) at the chosen position: before the pool on the
activation map (then the first maximum is taken of the masked map), or on the pooled output.

BatchNorm (section 19c). A BatchNorm record is conv + bias = z -> BatchNorm -> ReLU -> dropout -> max pool. For a call of n rows,
N = n x conv_out_h x conv_out_w over the WHOLE conv map, the positions a floor-mode pool drops included: mean = sum z / N,
var = sum (z - mean)^2 / N, zhat = (z - mean) rstd with rstd = 1 / sqrt(var + eps), y = gamma zhat + beta. Backward: dy as without
BatchNorm (a truncated position gets 0), dbeta = sum dy, dgamma = sum dy zhat, dz = gamma rstd (dy - dbeta / N - zhat dgamma / N), which
is non-zero on truncated positions too; dW and dX from dz. The conv bias gradient of a BatchNorm record is reported as 0 (sum dz = 0
in exact arithmetic; "b_sum" keeps the rounding noise for the comparison with autograd). Moving statistics: mm = m mm + (1 - m) mean
and the same for the population variance (unbiased: var N / (N - 1)). Fold: W' = W s, b' = (b - mm) s + beta, s = gamma / sqrt(mv + eps).
Whole tensors in the image's layout, statistics by numpy's mean over centred values, where the kernels merge per-workgroup moments by
Chan's formula over rows in the plan's order. No kernel runs BatchNorm on a padded record, so none is defined here.

Adadelta (section 19d): a = rho a + (1 - rho) g g, u = g sqrt(d + eps) / sqrt(a + eps), w -= lr u, d = rho d + (1 - rho) u u, from
a = d = 0."""
import numpy as np

from edison_amd import cube_import, train

import fnet_host
import fnet_plan
import fnet_rows
from fdrop_ref import factors, spec
from fnet_host import conv_records

SATURATING = ("i16", "n60")   # input sets that saturate the softmax: they tell nothing about a gradient
MOMENTUM, EPS_BN = train.BN_MOMENTUM, train.BN_EPS
EPS32 = 2.0 ** -24


def inputs(name, n, in_n):
    """n inputs of sweep row `name` as fnet_rows.inputs draws them, without the rows of the i16 / n60 sets."""
    sets = fnet_rows.SWEEP[name][0].get("sets", fnet_rows.SETS)
    keep = [i for i in range(len(sets)) if sets[i] not in SATURATING]
    m = (n + len(keep) - 1) // len(keep) * len(sets)
    x = fnet_rows.inputs(name, m, in_n)
    rows = [i for i in range(m) if i % len(sets) in keep][:n]
    return np.ascontiguousarray(x[rows])


TIE_POOLS = ((1, 2), (2, 1), (2, 2), (4, 1), (1, 4))
TIE_PADS = {(4, 1): (1, 0, 2, 0), (1, 4): (0, 1, 0, 2)}      # pool -> the pool pads of the padded tie case


def tie_case(pool, n=17, ppad=None):
    """(model, x [n][36], labels) whose pool windows tie exactly, without ReLU: a 2 x 2 conv to 3 channels on a 6 x 6 x 1 image, pool
    `pool` over its 5 x 5 map (truncating), a dense layer to 3 logits. The image is 0 / 1, the conv weights are +-0.5 / +-1 and the
    biases quarters, so every conv output is a sum that float32 holds exactly in any order and takes one of a few values: the first
    maximum of a window is tied at every element position. Channel 2 has zero weights: all its windows tie in every element.
    ppad (TIE_PADS[pool]): pool pads, so that along the pooled axis window 0 is (absent, 0, 1, 2) and window 1 is (3, 4, absent,
    absent): channel 2's gradient must land on element 1 of window 0 and on element 0 of window 1."""
    pool = tuple(pool)
    rng = np.random.default_rng((77 if ppad is None else 177) + 10 * pool[0] + pool[1])
    if ppad is None:
        recs = fnet_rows._records((6, 6, 1), [("conv", 3, (2, 2), (1, 1), pool, 0), ("dense", 3, 0)], pad_keys=False)
    else:
        recs = fnet_rows._records((6, 6, 1), [fnet_rows._c(3, (2, 2), p=pool, relu=0, ppad=ppad), ("dense", 3, 0)])
    recs[0]["w"] = rng.choice([-1.0, -0.5, 0.5, 1.0], (3, 2, 2, 1)).astype(np.float32)
    recs[0]["w"][2] = 0.0
    recs[0]["b"] = np.array([0.25, -0.5, 0.75], np.float32)
    k = int(np.prod(recs[1]["inp"]))
    recs[1]["w"] = (rng.normal(0, 1, (3,) + tuple(recs[1]["k"]) + (3,)) / np.sqrt(k)).astype(np.float32)
    recs[1]["b"] = rng.normal(0, 0.1, 3).astype(np.float32)
    recs.append(dict(type=cube_import.T_SOFTMAX, inp=recs[1]["out"], out=recs[1]["out"]))
    x = rng.integers(0, 2, (n, 36)).astype(np.float32)
    return dict(in_shape=(6, 6, 1), layers=recs), x, (np.arange(n) % 3).astype(np.int32)


def class_set(in_n, classes, rows, seed, noise=0.3):
    """The synthetic set of the fit tests: a fixed N(0, 1) pattern per class + N(0, noise), labels i % classes -> (x float32, y)."""
    rng = np.random.default_rng(seed)
    pattern = rng.normal(0, 1, (classes, in_n))
    y = (np.arange(rows) % classes).astype(np.int32)
    return (pattern[y] + rng.normal(0, noise, (rows, in_n))).astype(np.float32), y


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _cols(L, x):
    kh, kw = L["k"]
    sh, sw = L["s"]
    win = np.lib.stride_tricks.sliding_window_view(x, (kh, kw), axis=(1, 2))[:, ::sh, ::sw]   # [n][oh][ow][c][kh][kw]
    n, oh, ow = win.shape[:3]
    return win.transpose(0, 1, 2, 4, 5, 3).reshape(n, oh, ow, -1)                              # k = (ky kw + kx) c + ci


def _border(a, pad, fill):
    return np.pad(a, ((0, 0), (pad[0], pad[2]), (pad[1], pad[3]), (0, 0)), constant_values=fill)


def _windows(b, L):
    """The pool's windows of a bordered map: [n][Ph][Pw][oc][ph pw], elements in the order e = ey pw + ex."""
    (ph, pw), (Ph, Pw, oc) = L["p"], L["out"]
    return b[:, :Ph * ph, :Pw * pw].reshape(-1, Ph, ph, Pw, pw, oc).transpose(0, 1, 3, 5, 2, 4).reshape(-1, Ph, Pw, oc, ph * pw)


def _weights64(model, weights):
    """Per conv record (w, b) float64: the model's own, or `weights` = [dict(w, b)]."""
    src = conv_records(model) if weights is None else weights
    return [(np.asarray(t["w"], np.float64), np.asarray(t["b"], np.float64)) for t in src]


def _factors(model, dropout, n):
    """fdrop_ref.factors of dropout = None | (sp, seed, call) for n rows; sp None is off too."""
    if dropout is None or dropout[0] is None:
        return [None] * len(conv_records(model))
    return factors(model, dropout[0], dropout[1], dropout[2], n)


def loss_grad(model, x, labels, weights=None, n_total=None, dropout=None, bn=None, dtype=np.float64, pick="first", detail=False):
    """x [n][in_n], labels [n] -> dict(loss [n] per row, logits [n][n_out], argmax [n], probs, grads [dict(w [out][kh][kw][in],
    b [out])] of the batch loss (1 / n_total) sum loss), all in `dtype`. weights: other values than the model's, same shapes.
    dropout: None or (sp: fdrop_ref.spec's, seed, call). bn: None or dict(state=[None | dict(gamma, beta, ..)] (initial_state's
    form), eps=EPS_BN, trunc_in_stats=True): then each record's grads also carry b_sum and the result bn = [None | dict(gamma, beta:
    the gradients, mean, var: the batch statistics, N)].
    Two deliberate MISTAKES are kept so that a test can show the right rule is visible: pick="last" sends a window's gradient to its
    last maximum, trunc_in_stats=False leaves the truncated positions out of the statistics and of dz.
    detail=True adds per record dict(pre [n][ch][cw][oc]: conv + bias, y: the map behind BatchNorm (pre without it), first
    [n][Ph][Pw][oc]: the chosen element of the bordered window, win: the windows, dy [n][ch][cw][oc], dropped [n][Ph][Pw][oc]: the
    winner, or the pooled output, was dropped)."""
    recs = conv_records(model)
    W = [(np.asarray(w, dtype), np.asarray(b, dtype)) for w, b in _weights64(model, weights)]
    labels = np.asarray(labels).reshape(-1)
    h, w, c = model["in_shape"]
    a = np.asarray(x, dtype).reshape(-1, h, w, c)
    n = a.shape[0]
    n_total = n if n_total is None else n_total
    Fs = _factors(model, dropout, n)
    state = [None] * len(recs) if bn is None else bn["state"]
    eps, trunc = dtype(EPS_BN if bn is None else bn.get("eps", EPS_BN)), bn is None or bn.get("trunc_in_stats", True)
    keep = []
    for L, (wt, b), F, st in zip(recs, W, Fs, state):
        cp, pp = fnet_host.pads(L)
        a = a.reshape((-1,) + tuple(L["inp"]))
        cols = _cols(L, _border(a, cp, 0.0))                           # [n][ch][cw][K], zeros at the taps outside
        pre = cols @ wt.reshape(wt.shape[0], -1).T + b
        assert pre.shape[1:3] == fnet_host.conv_map(L)
        ph, pw = L["p"]
        Ph, Pw, oc = L["out"]
        y, stats = pre, None
        if st is not None:
            assert not any(cp) and not any(pp), "BatchNorm on a padded record: no kernel runs it, nothing holds it to autograd"
            region = pre if trunc else pre[:, :Ph * ph, :Pw * pw]
            N = region.size // oc
            mean = region.mean(axis=(0, 1, 2), dtype=dtype)
            var = ((region - mean) ** 2).mean(axis=(0, 1, 2), dtype=dtype)
            rstd = dtype(1) / np.sqrt(var + eps)
            zhat = (pre - mean) * rstd
            y = np.asarray(st["gamma"], dtype) * zhat + np.asarray(st["beta"], dtype)
            stats = dict(mean=mean, var=var, rstd=rstd, zhat=zhat, N=N, gamma=np.asarray(st["gamma"], dtype))
        act = np.maximum(y, dtype(0)) if L["relu"] else y
        if F is not None and F["before"]:
            act = act * F["image"].astype(dtype)
        bordered = _border(act, pp, -np.inf)
        win = _windows(bordered, L)
        first = win.argmax(axis=-1) if pick == "first" else ph * pw - 1 - win[..., ::-1].argmax(axis=-1)
        keep.append((cols, pre, y, first, win, bordered.shape, stats))
        a = np.take_along_axis(win, first[..., None], -1)[..., 0]
        assert np.isfinite(a).all()                                    # every window has a present element
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
    d = d / dtype(n_total)
    grads, bns, details = [None] * len(recs), [None] * len(recs), [None] * len(recs)
    for i in range(len(recs) - 1, -1, -1):
        L, (wt, b), F = recs[i], W[i], Fs[i]
        cp, pp = fnet_host.pads(L)
        cols, pre, y, first, win, bshape, stats = keep[i]
        ph, pw = L["p"]
        Ph, Pw, oc = L["out"]
        ch, cw = pre.shape[1:3]
        d = d.reshape(n, Ph, Pw, oc)
        dropped = np.zeros(d.shape, bool)
        if F is not None and not F["before"]:
            d = d * F["image"].astype(dtype)
            dropped = F["image"] == 0
        dwin = np.zeros((n, Ph, Pw, oc, ph * pw), dtype)
        np.put_along_axis(dwin, first[..., None], d[..., None], -1)
        dyb = np.zeros(bshape, dtype)
        dyb[:, :Ph * ph, :Pw * pw] = dwin.reshape(n, Ph, Pw, oc, ph, pw).transpose(0, 1, 4, 2, 5, 3).reshape(n, Ph * ph, Pw * pw, oc)
        dy = dyb[:, pp[0]:pp[0] + ch, pp[1]:pp[1] + cw]                # an absent element is never chosen: nothing is cropped away
        assert np.count_nonzero(dyb) == np.count_nonzero(dy)
        if F is not None and F["before"]:
            dy = dy * F["image"].astype(dtype)
            dropped = np.take_along_axis(_windows(_border(F["image"], pp, 1.0), L), first[..., None], -1)[..., 0] == 0
        if L["relu"]:
            dy = dy * (y > 0)
        dz = dy
        if stats is not None:
            dbeta = dy.sum(axis=(0, 1, 2), dtype=dtype)
            dgamma = (dy * stats["zhat"]).sum(axis=(0, 1, 2), dtype=dtype)
            dz = stats["gamma"] * stats["rstd"] * (dy - dbeta / dtype(stats["N"]) - stats["zhat"] * (dgamma / dtype(stats["N"])))
            if not trunc:
                full = np.zeros_like(dz)
                full[:, :Ph * ph, :Pw * pw] = dz[:, :Ph * ph, :Pw * pw]
                dz = full
            bns[i] = dict(gamma=dgamma, beta=dbeta, mean=stats["mean"], var=stats["var"], N=stats["N"])
        bsum = dz.sum(axis=(0, 1, 2), dtype=dtype)
        grads[i] = dict(w=np.einsum("nhwc,nhwk->ck", dz, cols).reshape(wt.shape), b=np.zeros_like(bsum) if stats is not None else bsum)
        if bn is not None:
            grads[i]["b_sum"] = bsum
        details[i] = dict(pre=pre, y=y, first=first, win=win, dy=dy, dropped=dropped)
        if i == 0:
            break
        dcols = dz @ wt.reshape(oc, -1)                                # [n][ch][cw][K]
        kh, kw = L["k"]
        sh, sw = L["s"]
        ih, iw, ic = L["inp"]
        dxb = np.zeros((n, ih + cp[0] + cp[2], iw + cp[1] + cp[3], ic), dtype)
        for ky in range(kh):
            for kx in range(kw):
                k0 = (ky * kw + kx) * ic
                dxb[:, ky:ky + sh * ch:sh, kx:kx + sw * cw:sw, :] += dcols[..., k0:k0 + ic]
        d = dxb[:, cp[0]:cp[0] + ih, cp[1]:cp[1] + iw]
    out = dict(loss=loss, logits=z, argmax=np.argmax(z, axis=1).astype(np.int32), grads=grads, probs=probs)
    if bn is not None:
        out["bn"] = bns
    if detail:
        out["detail"] = details
    return out


def torch_grads(model, x, labels, dtype, weights=None, dropout=None, bn=None, momentum=MOMENTUM):
    """The same call through torch's CPU autograd in `dtype`: F.pad(value=0) where a conv has pads -> F.conv2d -> F.batch_norm(training=
    True) -> relu -> dropout's factor -> F.pad(value=-inf) where a pool has pads -> F.max_pool2d (floor mode) -> dropout's factor ->
    cross_entropy. Returns dict(loss [n], logits, grads [dict(w, b)]) as numpy float64 arrays in the model dict's layout; with bn also
    bn [None | dict(gamma, beta: gradients, mean, var: torch's running statistics after the call, which use var N / (N - 1))]."""
    import torch
    import torch.nn.functional as F
    recs = conv_records(model)
    W = _weights64(model, weights)
    h, w, c = model["in_shape"]
    a = torch.tensor(np.asarray(x, np.float64).reshape(-1, h, w, c), dtype=dtype).permute(0, 3, 1, 2)
    state = [None] * len(recs) if bn is None else bn["state"]
    params, bnp = [], []
    for L, (wt, b), fac, st in zip(recs, W, _factors(model, dropout, a.shape[0]), state):
        cp, pp = fnet_host.pads(L)
        tw = torch.tensor(wt, dtype=dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)   # [out][in][kh][kw]
        tb = torch.tensor(b, dtype=dtype).requires_grad_(True)
        params.append((tw, tb))
        ih, iw, ic = L["inp"]
        a = a.permute(0, 2, 3, 1).reshape(-1, ih, iw, ic).permute(0, 3, 1, 2)
        if any(cp):
            a = F.pad(a, (cp[1], cp[3], cp[0], cp[2]), value=0.0)
        a = F.conv2d(a, tw, tb, stride=tuple(L["s"]))
        if st is None:
            bnp.append(None)
        else:
            g, be = [torch.tensor(np.asarray(st[k], np.float64), dtype=dtype).requires_grad_(True) for k in ("gamma", "beta")]
            rm, rv = [torch.tensor(np.asarray(st[k], np.float64), dtype=dtype) for k in ("mean", "var")]
            a = F.batch_norm(a, rm, rv, g, be, training=True, momentum=1.0 - momentum, eps=bn.get("eps", EPS_BN))
            bnp.append((g, be, rm, rv))
        if L["relu"]:
            a = F.relu(a)
        ft = None if fac is None else torch.tensor(fac["image"], dtype=dtype).permute(0, 3, 1, 2)
        if fac is not None and fac["before"]:
            a = a * ft
        if tuple(L["p"]) != (1, 1):
            if any(pp):
                a = F.pad(a, (pp[1], pp[3], pp[0], pp[2]), value=float("-inf"))
            a = F.max_pool2d(a, tuple(L["p"]))
        if fac is not None and not fac["before"]:
            a = a * ft
    z = a.permute(0, 2, 3, 1).reshape(a.shape[0], -1)
    rows = F.cross_entropy(z, torch.tensor(np.asarray(labels).reshape(-1), dtype=torch.long), reduction="none")
    rows.mean().backward()
    out = dict(loss=rows.detach().double().numpy(), logits=z.detach().double().numpy(),
               grads=[dict(w=tw.grad.permute(0, 2, 3, 1).double().numpy().copy(), b=tb.grad.double().numpy().copy()) for tw, tb in params])
    if bn is not None:
        out["bn"] = [None if p is None else dict(gamma=p[0].grad.double().numpy().copy(), beta=p[1].grad.double().numpy().copy(),
                                                 mean=p[2].double().numpy().copy(), var=p[3].double().numpy().copy()) for p in bnp]
    return out


def tensor_error(got, want):
    """The GPU test's metric for one tensor: max |g - g64| / max |g64| (max |g| where g64 is all zero; 0 when both are)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    return 0.0 if err == 0.0 else err / scale if scale > 0 else np.inf


def live(L):
    """Rows of record L per utterance that are not absent: the conv positions inside the pooled windows."""
    (ph, pw), (_, q) = L["p"], fnet_host.pads(L)
    Ph, Pw = L["out"][:2]
    ch, cw = fnet_host.conv_map(L)
    return sum(q[0] <= y < q[0] + ch for y in range(Ph * ph)) * sum(q[1] <= x < q[1] + cw for x in range(Pw * pw))


def terms(model, n, whole_map=False):
    """Per conv record, how many terms the sums behind one element of dW and of db have at most: n rows x the live rows (Ph ph Pw pw
    without pads); whole_map: n rows x the whole conv map, what a BatchNorm record's sums run over."""
    return [n * (int(np.prod(fnet_host.conv_map(L))) if whole_map else live(L)) for L in conv_records(model)]


def bounds(model, x, y, ref, n_total=None, dropout=None, bn=None):
    """The GPU tests' allowances on a call whose float64 restatement is `ref` (section 19's rule): (per record dict(w, b, and with
    BatchNorm gamma, beta: (bound, e32)), the loss's (bound, e32), the logits' (bound, e32)). e32 is the error (tensor_error) of
    torch's CPU float32 autograd on the same call against ref, bound = 4 e32 floored at 8 x 2^-24 x sqrt(terms summed): terms(), over
    the whole map where bn is given; for the loss and the logits the k rows along the network plus the logits. n_total: ref is a part
    of a batch of n_total rows (torch's mean is over the rows it is given). A BatchNorm record's conv bias is held to ref's b_sum."""
    import torch
    t32 = torch_grads(model, x, y, torch.float32, dropout=dropout, bn=bn)
    scale = 1.0 if n_total is None else len(y) / n_total
    allow = lambda e, floor: (max(4 * e, floor), e)
    per = []
    for i, (g32, g64, t) in enumerate(zip(t32["grads"], ref["grads"], terms(model, len(y), whole_map=bn is not None))):
        floor = 8 * EPS32 * np.sqrt(t)
        b64 = None if bn is None else ref["bn"][i]
        rec = dict(w=allow(tensor_error(g32["w"] * scale, g64["w"]), floor),
                   b=allow(tensor_error(g32["b"] * scale, g64["b" if b64 is None else "b_sum"]), floor))
        for k in ("gamma", "beta") if b64 is not None else ():
            rec[k] = allow(tensor_error(t32["bn"][i][k] * scale, b64[k]), floor)
        per.append(rec)
    floor = 8 * EPS32 * np.sqrt(sum(int(np.prod(L["k"])) * L["inp"][2] for L in conv_records(model)) + ref["logits"].shape[1])
    return per, allow(tensor_error(t32["loss"], ref["loss"]), floor), allow(tensor_error(t32["logits"], ref["logits"]), floor)


# ---- BatchNorm's state ----------------------------------------------------------------------------------------------------------------
def initial_state(model, has_bn, dtype=np.float64):
    """Per record None or dict(gamma 1, beta 0, mean 0, var 1)."""
    return [dict(gamma=np.ones(L["out"][2], dtype), beta=np.zeros(L["out"][2], dtype), mean=np.zeros(L["out"][2], dtype), var=np.ones(L["out"][2], dtype))
            if h else None for L, h in zip(conv_records(model), has_bn)]


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
        z = _cols(L, a) @ wt.reshape(wt.shape[0], -1).T + np.asarray(t["b"], np.float64)
        if st is not None:
            z = (z - st["mean"]) / np.sqrt(np.asarray(st["var"], np.float64) + eps) * st["gamma"] + st["beta"]
        if L["relu"]:
            z = np.maximum(z, 0.0)
        ph, pw = L["p"]
        Ph, Pw, oc = L["out"]
        a = z[:, :Ph * ph, :Pw * pw].reshape(n, Ph, ph, Pw, pw, oc).max(axis=(2, 4))
    return a.reshape(n, -1)


# ---- the trainer's plan and the order of its sums -----------------------------------------------------------------------------------
def train_lds_bytes(plan, batch):
    """ed_ftrain_lds_bytes of a restated plan (fnet_plan.plan) at `batch` utterances per workgroup: the larger of
    the forward half's LDS and the backward half's dY [16-padded batch x rows][n_pad] floats + row bases [16-padded batch x rows], one
    int a row and two on a padded record, each the largest record's (ftrain_size_lds)."""
    fwd = 4 * (batch * sum(plan["buf_n"]) + plan["w_lds"]) + 4 * plan["k_lds"]
    mp = [(batch * L["rows"] + 15) // 16 * 16 for L in plan["layers"]]
    bwd = 4 * max(m * L["n_pad"] for m, L in zip(mp, plan["layers"])) + 4 * max(m * (2 if L.get("pad") else 1) for m, L in zip(mp, plan["layers"]))
    return max(fwd, bwd)


def train_batch(plan, limit=None):
    """The utterances per workgroup edison_ftrain_create trains a restated plan at: the network's own batch, lowered while the training
    workgroup does not fit `limit` bytes of LDS (fnet_plan.LDS_BYTES); 0 for a plan it refuses, whose one utterance does not fit."""
    limit = fnet_plan.LDS_BYTES if limit is None else limit
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


# ---- the optimisers as Keras states them ----------------------------------------------------------------------------------------------
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


class Adadelta:
    """float64, over any list of arrays (Adam's interface), as Keras and torch.optim.Adadelta state it."""

    def __init__(self, rho=0.95, eps=1e-7):
        self.rho, self.eps, self.a, self.d = rho, eps, None, None

    def step(self, ws, gs, lr):
        """ws, gs: lists of float64 arrays; ws is updated in place."""
        if self.a is None:
            self.a, self.d = [np.zeros_like(w) for w in ws], [np.zeros_like(w) for w in ws]
        for w, g, a, d in zip(ws, gs, self.a, self.d):
            a *= self.rho
            a += (1.0 - self.rho) * g * g
            u = g * np.sqrt(d + self.eps) / np.sqrt(a + self.eps)
            w -= lr * u
            d *= self.rho
            d += (1.0 - self.rho) * u * u


class Adadelta32:
    """ed_ftrain_adadelta_kernel's arithmetic in numpy float32: every product, sum, square root and quotient rounded to float32, the
    constants rho, 1 - rho (taken in double first, as the library does), eps and lr as floats. The kernel may fuse a product into the sum
    behind it, which this does not: one rounding fewer, inside the bound."""

    def __init__(self, rho=0.95, eps=1e-7):
        self.rho, self.omr, self.eps, self.a, self.d = np.float32(rho), np.float32(1.0 - rho), np.float32(eps), None, None

    def step(self, ws, gs, lr):
        """ws, gs: lists of float32 arrays; ws is updated in place."""
        lr = np.float32(lr)
        if self.a is None:
            self.a, self.d = [np.zeros_like(w) for w in ws], [np.zeros_like(w) for w in ws]
        for w, g, a, d in zip(ws, gs, self.a, self.d):
            assert w.dtype == g.dtype == a.dtype == d.dtype == np.float32
            a[...] = self.rho * a + self.omr * g * g
            u = g * np.sqrt(d + self.eps) / np.sqrt(a + self.eps)
            assert u.dtype == np.float32
            w -= lr * u
            d[...] = self.rho * d + self.omr * u * u


# ---- the host trainer -------------------------------------------------------------------------------------------------------------------
class HostData:
    """A data set for HostTrainer.epoch and evaluate, with train.DeviceData's n."""

    def __init__(self, x, y):
        self.x, self.y = np.asarray(x).reshape(len(x), -1), np.asarray(y).astype(np.int32).reshape(-1)
        self.n = len(self.y)


class HostTrainer:
    """The GPU trainer in float64 on the host, for edison_amd.train.fit and fit_data to drive: the replay the GPU's fit is held to.
    `opt` (Adam()) steps the weights and, with has_bn, gamma and beta. A training call masks with the current dropout counter, then
    advances it, and moves BatchNorm's moving statistics; training=False runs the folded network, masks nothing and moves nothing."""

    def __init__(self, model, dropout=None, before_pool=None, seed=0, has_bn=None, momentum=MOMENTUM, eps=EPS_BN, unbiased=False, opt=None):
        n = len(conv_records(model))
        self.model = model
        self.weights = [dict(w=w.copy(), b=b.copy()) for w, b in _weights64(model, None)]
        self.sp = spec(model, [0] * n if dropout is None else dropout, before_pool)
        self.seed, self.call = int(seed), 0
        self.has_bn = has_bn is not None
        self.state = initial_state(model, has_bn if self.has_bn else [0] * n)
        self.momentum, self.eps, self.unbiased = momentum, eps, unbiased
        self.opt = Adam() if opt is None else opt
        self._g = self._gbn = None

    def dropout(self):
        return dict(rates=[r for r, _ in self.sp], before_pool=[int(b) for _, b in self.sp], seed=self.seed, call=self.call,
                    on=any(r > 0 for r, _ in self.sp))

    def batchnorm(self):
        return dict(on=self.has_bn)

    def folded(self):
        return fold(self.weights, self.state, self.eps)

    def grad(self, x, y, training=True):
        self._g = self._gbn = None
        if not training:
            r = loss_grad(self.model, x, y, weights=self.folded())
        else:
            on = self.dropout()["on"]
            r = loss_grad(self.model, x, y, weights=self.weights, dropout=(self.sp, self.seed, self.call) if on else None,
                          bn=dict(state=self.state, eps=self.eps))
            self.call += int(on)
            self.state = moved(self.state, r["bn"], self.momentum, self.unbiased)
            self._g, self._gbn = r["grads"], r["bn"]
        return dict(loss=r["loss"], argmax=r["argmax"])

    def step(self, lr):
        ws = [t[k] for t in self.weights for k in ("w", "b")] + [st[k] for st in self.state if st is not None for k in ("gamma", "beta")]
        gs = [np.asarray(t[k], np.float64) for t in self._g for k in ("w", "b")] + [np.asarray(b[k], np.float64) for b in self._gbn if b is not None
                                                                                    for k in ("gamma", "beta")]
        self.opt.step(ws, gs, lr)

    def _sums(self, r, y):
        return float(np.sum(r["loss"], dtype=np.float64)), int((r["argmax"] == y).sum())

    def epoch(self, data, order, batch, lr, max_steps=None):
        """Trainer.epoch on a HostData: fit's batch loop, summed per batch as fit sums -> dict(loss_sum, hits, seen, steps)."""
        out = dict(loss_sum=0.0, hits=0, seen=0, steps=0)
        for b0 in range(0, len(order), batch):
            if max_steps is not None and out["steps"] >= max_steps:
                break
            rows = order[b0:b0 + batch]
            r = self.grad(data.x[rows], data.y[rows])
            self.step(lr)
            loss, hits = self._sums(r, data.y[rows])
            out = dict(loss_sum=out["loss_sum"] + loss, hits=out["hits"] + hits, seen=out["seen"] + len(rows), steps=out["steps"] + 1)
        return out

    def evaluate(self, data):
        """Trainer.evaluate on a HostData: fit's validation loop, 4096 rows a call -> dict(loss_sum, hits, seen, steps = 0)."""
        out = dict(loss_sum=0.0, hits=0, seen=0, steps=0)
        for b0 in range(0, data.n, 4096):
            y = data.y[b0:b0 + 4096]
            loss, hits = self._sums(self.grad(data.x[b0:b0 + 4096], y, training=False), y)
            out = dict(loss_sum=out["loss_sum"] + loss, hits=out["hits"] + hits, seen=out["seen"] + len(y), steps=0)
        return out

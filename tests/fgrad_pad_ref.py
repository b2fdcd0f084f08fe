"""Float64 restatement of training a padded float network ('same' convs and pools, DESIGN.md sections 14b and 19): fgrad_ref.loss_grad
with pads, on fnet_pad's conventions. Test infrastructure, not a test: tests/test_fgrad_pad_cpu.py holds it to torch's float64 autograd
and to central differences, tests/test_gpu_ftrain_pad.py holds the kernels (edison_ftrain_create_ex with EDISON_FTRAIN_PADDED) to it.

Written differently from the kernel on purpose: the conv runs over a zero-bordered copy of its input and the pool over a -inf-bordered
copy of the conv's map, where the kernel works on the dense images with a predicate per tap and per row. The pool's gradient goes to
the first maximum of the bordered window in element order (numpy's argmax): an absent element is -inf and every window has a present
one, so that is the first maximum among the present elements. dX is cropped back from the bordered gradient, dW comes from the
bordered columns (a tap outside the image is the operand 0 and adds nothing)."""
import numpy as np

from edison_amd import cube_import

import fgrad_ref
import fnet_exact
import fnet_pad

N_ROWS = 17                      # rows of a gradient check: two tiles at a batch of 16, the second of one row
NEG_T = "neg_no_relu_t"          # fnet_pad's neg_no_relu with a bias that does not saturate the softmax
ROWS = [NEG_T if name == "neg_no_relu" else name for name in fnet_pad.ROWS]
ALL_N = ("sym3x3", "pool41_lead", "mid_pads_batch")      # rows the GPU test also runs at n = 1, b - 1, b, b + 1 and 3 b + 2 for the trainer's batch b


def n_max(name):
    """The most rows of row `name` a gradient check draws: 3 x 16 + 2 on the ALL_N rows (mid_pads_batch trains at batch 5: 17)."""
    return 3 * 16 + 2 if name in ALL_N else N_ROWS


def conv_records(model):
    return fgrad_ref.conv_records(model)


# ---- the rows and their inputs ------------------------------------------------------------------------------------------------------
_MODELS = {}


def model(name):
    """fnet_pad.model; neg_no_relu_t: neg_no_relu's layers and pads with bias -3 and positive weights in every record."""
    if name not in _MODELS:
        if name == NEG_T:
            spec = fnet_pad.ROWS["neg_no_relu"][0]
            rng = np.random.default_rng(2000 + fnet_pad._seed(name))
            recs = fnet_pad._records(spec["in_shape"], spec["layers"])
            for L in recs:
                oc, (kh, kw), ic = L["out"][2], L["k"], L["inp"][2]
                L["w"] = np.abs(rng.normal(0, 1, (oc, kh, kw, ic)) / np.sqrt(kh * kw * ic)).astype(np.float32)
                L["b"] = np.full(oc, -3.0, np.float32)
            recs.append(dict(type=cube_import.T_SOFTMAX, inp=recs[-1]["out"], out=recs[-1]["out"]))
            _MODELS[name] = dict(in_shape=spec["in_shape"], layers=recs)
        else:
            _MODELS[name] = fnet_pad.model(name)
    return _MODELS[name]


def blob(name):
    return cube_import.build_blob(model(name)) if name == NEG_T else fnet_pad.blob(name)


def data(name, n=N_ROWS):
    """(x [n][in_n] float32, labels i % n_out) of row `name`: N(0, 1); neg_no_relu_t: -|N(0, 1)| - 0.1, every input negative."""
    m = model(name)
    in_n = int(np.prod(m["in_shape"]))
    x = np.random.default_rng(5000 + fnet_pad._seed(name)).normal(0, 1, (n, in_n)).astype(np.float32)
    if name == NEG_T:
        x = (-np.abs(x) - np.float32(0.1)).astype(np.float32)
    n_out = int(np.prod(conv_records(m)[-1]["out"]))
    return x, (np.arange(n) % n_out).astype(np.int32)


def tie_case(pool, n=N_ROWS):
    """fgrad_ref.tie_case with pool pads: a 2 x 2 conv to 3 channels on a 6 x 6 x 1 image of 0 / 1, weights +-0.5 / +-1, biases in
    quarters, no ReLU, then pool (4, 1) with pool pads (1, 0, 2, 0) or pool (1, 4) with (0, 1, 0, 2) over the 5 x 5 map: along the
    pooled axis window 0 is (absent, 0, 1, 2) and window 1 is (3, 4, absent, absent). Channel 2 has zero weights, so all the present
    elements of its windows tie: the gradient must land on element 1 of window 0 and on element 0 of window 1."""
    pool = tuple(pool)
    ppad = {(4, 1): (1, 0, 2, 0), (1, 4): (0, 1, 0, 2)}[pool]
    rng = np.random.default_rng(177 + 10 * pool[0] + pool[1])
    recs = fnet_pad._records((6, 6, 1), [fnet_pad._c(3, (2, 2), p=pool, relu=0, ppad=ppad), ("dense", 3, 0)])
    recs[0]["w"] = rng.choice([-1.0, -0.5, 0.5, 1.0], (3, 2, 2, 1)).astype(np.float32)
    recs[0]["w"][2] = 0.0
    recs[0]["b"] = np.array([0.25, -0.5, 0.75], np.float32)
    k = int(np.prod(recs[1]["inp"]))
    recs[1]["w"] = (rng.normal(0, 1, (3,) + tuple(recs[1]["k"]) + (recs[1]["inp"][2],)) / np.sqrt(k)).astype(np.float32)
    recs[1]["b"] = rng.normal(0, 0.1, 3).astype(np.float32)
    recs.append(dict(type=cube_import.T_SOFTMAX, inp=recs[1]["out"], out=recs[1]["out"]))
    x = rng.integers(0, 2, (n, 36)).astype(np.float32)
    return dict(in_shape=(6, 6, 1), layers=recs), x, (np.arange(n) % 3).astype(np.int32)


TIE_POOLS = ((4, 1), (1, 4))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _border(a, pad, fill):
    return np.pad(a, ((0, 0), (pad[0], pad[2]), (pad[1], pad[3]), (0, 0)), constant_values=fill)


def loss_grad(model, x, labels, weights=None, n_total=None, pick="first", detail=False):
    """fgrad_ref.loss_grad for records with cpad / ppad. pick="last" sends a window's gradient to its last maximum instead (what a
    wrong kernel might do; the CPU test measures how far that moves dW). detail=True adds per record dict(pre [n][ch][cw][oc], first
    [n][Ph][Pw][oc]: the chosen element of the bordered window, dy [n][ch][cw][oc])."""
    recs = conv_records(model)
    W = fgrad_ref._weights64(model, weights)
    labels = np.asarray(labels).reshape(-1)
    h, w, c = model["in_shape"]
    a = np.asarray(x, np.float64).reshape(-1, h, w, c)
    n = a.shape[0]
    n_total = n if n_total is None else n_total
    keep = []
    for L, (wt, b) in zip(recs, W):
        cp, pp = fnet_pad.pads(L)
        a = a.reshape((-1,) + tuple(L["inp"]))
        cols = fgrad_ref._cols(L, _border(a, cp, 0.0))                 # [n][ch][cw][K], zeros at the taps outside
        pre = cols @ wt.reshape(wt.shape[0], -1).T + b
        assert pre.shape[1:3] == fnet_pad.conv_map(L)
        act = np.maximum(pre, 0.0) if L["relu"] else pre
        ph, pw = L["p"]
        Ph, Pw, oc = L["out"]
        bordered = _border(act, pp, -np.inf)
        win = bordered[:, :Ph * ph, :Pw * pw].reshape(n, Ph, ph, Pw, pw, oc).transpose(0, 1, 3, 5, 2, 4).reshape(n, Ph, Pw, oc, ph * pw)
        first = win.argmax(axis=-1) if pick == "first" else ph * pw - 1 - win[..., ::-1].argmax(axis=-1)
        keep.append((a.shape, cols, pre, first, bordered.shape))
        a = np.take_along_axis(win, first[..., None], -1)[..., 0]
        assert np.isfinite(a).all()                                    # every window has a present element
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
        L, (wt, b) = recs[i], W[i]
        cp, pp = fnet_pad.pads(L)
        shape, cols, pre, first, bshape = keep[i]
        ph, pw = L["p"]
        Ph, Pw, oc = L["out"]
        ch, cw = pre.shape[1:3]
        d = d.reshape(n, Ph, Pw, oc)
        dwin = np.zeros((n, Ph, Pw, oc, ph * pw))
        np.put_along_axis(dwin, first[..., None], d[..., None], -1)
        dyb = np.zeros(bshape)
        dyb[:, :Ph * ph, :Pw * pw] = dwin.reshape(n, Ph, Pw, oc, ph, pw).transpose(0, 1, 4, 2, 5, 3).reshape(n, Ph * ph, Pw * pw, oc)
        dy = dyb[:, pp[0]:pp[0] + ch, pp[1]:pp[1] + cw]                # an absent element is never chosen: nothing is cropped away
        assert np.count_nonzero(dyb) == np.count_nonzero(dy)
        if L["relu"]:
            dy = dy * (pre > 0.0)
        grads[i] = dict(w=np.einsum("nhwc,nhwk->ck", dy, cols).reshape(wt.shape), b=dy.sum(axis=(0, 1, 2)))
        details[i] = dict(pre=pre, first=first, dy=dy)
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


def torch_grads(model, x, labels, dtype, weights=None):
    """fgrad_ref.torch_grads with F.pad(value=0) before conv2d and F.pad(value=-inf) before max_pool2d."""
    import torch
    import torch.nn.functional as F
    recs = conv_records(model)
    W = fgrad_ref._weights64(model, weights)
    h, w, c = model["in_shape"]
    a = torch.tensor(np.asarray(x, np.float64).reshape(-1, h, w, c), dtype=dtype).permute(0, 3, 1, 2)
    params = []
    for L, (wt, b) in zip(recs, W):
        cp, pp = fnet_pad.pads(L)
        tw = torch.tensor(wt, dtype=dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        tb = torch.tensor(b, dtype=dtype).requires_grad_(True)
        params.append((tw, tb))
        ih, iw, ic = L["inp"]
        a = a.permute(0, 2, 3, 1).reshape(-1, ih, iw, ic).permute(0, 3, 1, 2)
        a = F.conv2d(F.pad(a, (cp[1], cp[3], cp[0], cp[2]), value=0.0), tw, tb, stride=tuple(L["s"]))
        if L["relu"]:
            a = F.relu(a)
        if tuple(L["p"]) != (1, 1):
            a = F.max_pool2d(F.pad(a, (pp[1], pp[3], pp[0], pp[2]), value=float("-inf")), tuple(L["p"]))
    z = a.permute(0, 2, 3, 1).reshape(a.shape[0], -1)
    rows = F.cross_entropy(z, torch.tensor(np.asarray(labels).reshape(-1), dtype=torch.long), reduction="none")
    rows.mean().backward()
    grads = [dict(w=tw.grad.permute(0, 2, 3, 1).double().numpy().copy(), b=tb.grad.double().numpy().copy()) for tw, tb in params]
    return dict(loss=rows.detach().double().numpy(), logits=z.detach().double().numpy(), grads=grads)


def live(L):
    """Rows of record L per utterance that are not absent: the conv positions inside the pooled windows."""
    (ph, pw), (_, q) = L["p"], fnet_pad.pads(L)
    Ph, Pw = L["out"][:2]
    ch, cw = fnet_pad.conv_map(L)
    return sum(q[0] <= y < q[0] + ch for y in range(Ph * ph)) * sum(q[1] <= x < q[1] + cw for x in range(Pw * pw))


def terms(model, n):
    """Per conv record, how many terms the sums behind one element of dW and of db have at most: n rows x the live rows."""
    return [n * live(L) for L in conv_records(model)]


# ---- the trainer's plan -------------------------------------------------------------------------------------------------------------
def train_lds_bytes(plan, batch):
    """fgrad_ref.train_lds_bytes of a restated plan (fnet_pad.plan): a padded record's row base is two ints (ftrain_size_lds)."""
    fwd = 4 * (batch * sum(plan["buf_n"]) + plan["w_lds"]) + 4 * plan["k_lds"]
    mp = [(batch * L["rows"] + 15) // 16 * 16 for L in plan["layers"]]
    bwd = 4 * max(m * L["n_pad"] for m, L in zip(mp, plan["layers"])) + 4 * max(m * (2 if L["pad"] else 1) for m, L in zip(mp, plan["layers"]))
    return max(fwd, bwd)


def train_batch(plan, limit=None):
    """fgrad_ref.train_batch on train_lds_bytes above."""
    limit = fnet_exact.LDS_BYTES if limit is None else limit
    batch = plan["batch"]
    while batch > 1 and train_lds_bytes(plan, batch) > limit:
        batch -= 1
    return batch if train_lds_bytes(plan, batch) <= limit else 0


class HostTrainer(fgrad_ref.HostTrainer):
    """fgrad_ref.HostTrainer on the padded restatement."""

    def grad(self, x, y):
        r = loss_grad(self.model, x, y, weights=self.weights)
        self._g = r["grads"]
        return dict(loss=r["loss"], argmax=r["argmax"])


# ---- the synthetic data set of the fit tests ----------------------------------------------------------------------------------------
FIT_ROW, FIT_CLASSES, FIT_ROWS, FIT_NOISE = "stride2_same", 3, 96, 0.3


def fit_set():
    """fgrad_ref.fit_set on stride2_same's input shape (its dense layer has 3 outputs)."""
    h, w, c = fnet_pad.ROWS[FIT_ROW][0]["in_shape"]
    rng = np.random.default_rng(2025)
    pattern = rng.normal(0, 1, (FIT_CLASSES, h * w * c))
    y = (np.arange(FIT_ROWS) % FIT_CLASSES).astype(np.int32)
    x = (pattern[y] + rng.normal(0, FIT_NOISE, (FIT_ROWS, h * w * c))).astype(np.float32)
    return x, y


def kws_set(in_n=403, classes=10, rows=96):
    """The same for `kws train` on a zoo network at 31 x 13 x 1: ten classes, 96 rows."""
    rng = np.random.default_rng(2026)
    pattern = rng.normal(0, 1, (classes, in_n))
    y = (np.arange(rows) % classes).astype(np.int32)
    return (pattern[y] + rng.normal(0, FIT_NOISE, (rows, in_n))).astype(np.float32), y

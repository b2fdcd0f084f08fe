"""Dropout in the float32 trainer (csrc/fnet_dropout.h, edison_ftrain_set_dropout): a numpy restatement of the mask
and of the kernel's forward half with it; training with it in float64 is tests/ftrain_ref.py's, which takes `factors` from here. Test
infrastructure, not a test: tests/test_fdrop_cpu.py holds it to Philox's known answers and to a stand-alone host program on the header;
tests/test_gpu_ftrain_dropout.py holds the kernels to it.

The mask. Element e of record l is kept for sample u of training call `call` under `seed` iff fmix32(fmix32(e ^ kA) + kB) >= T, with
(kA, kB) words 0 and 1 of Philox4x32-10 at counter (u, call & 0xffffffff, call >> 32, l) and key (seed & 0xffffffff, seed >> 32), and
T = floor(rate 2^32 + 0.5). A kept value is multiplied by s = float32(1 / (1 - rate)), a dropped one is +0.0f. After the pool
e = q out_c + c; before the pool e = r out_c + c with r = q P + element the plan's output row, absent rows counted. A record without a
pool has one position.

Written differently from the kernel: the mask is built as whole 0 / s factor tensors in the image's layout and multiplied in, where
the kernel hashes per element in its accumulator layout."""
import numpy as np

from edison_amd import train

import fnet_host
from fnet_host import conv_records

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
    recs = conv_records(model)
    assert len(rates) == len(recs) and rates[-1] == 0.0
    return [(r, bool(b) and L["p"][0] * L["p"][1] > 1) for r, b, L in zip(rates, before, recs)]


def factors(model, sp, seed, call, n):
    """Per record None (rate 0) or dict(before, rows [n][rows][oc] or [n][Ph Pw][oc]: 0 / s float32 in the plan's element order, keep:
    the same as bool, image: float64 in the layout loss_grad multiplies it in: [n][conv_h][conv_w][oc] before the pool (1 where
    the pool's floor reads nothing), [n][Ph][Pw][oc] behind it)."""
    out = []
    for l, (L, (rate, before)) in enumerate(zip(conv_records(model), sp)):
        if rate == 0.0:
            out.append(None)
            continue
        (ph, pw), (Ph, Pw, oc) = L["p"], L["out"]
        P = ph * pw
        rows = Ph * Pw * (P if before else 1)
        k = kept(seed, call, n, l, rows * oc, rate).reshape(n, rows, oc)
        f = np.where(k, scale(rate), np.float32(0)).astype(np.float32)
        if before:
            ch, cw = fnet_host.conv_map(L)
            pp = fnet_host.pads(L)[1]
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
    fnet_host.pre_activation's values are the GPU's; ReLU, the mask, x s in float32 and the pool follow them. detail=True: per record
    also (first [n][Ph Pw][oc], positive [n][rows][oc], dropped [n][Ph Pw][oc]: the winner, or the pooled output, was dropped)."""
    a = np.asarray(x, np.float32)
    n = len(a)
    outs, det = [], []
    for L, F in zip(conv_records(model), factors(model, sp, seed, call, n)):
        Ph, Pw, oc = L["out"]
        P = L["p"][0] * L["p"][1]
        v, live = fnet_host.pre_activation(L, a)
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

"""Host restatement of the calibration statistic (edison_fcal_*, edison_amd/csrc/fnet_calib_kernels.hip), built
on fnet_exact's bit-exact f32 chain. Test infrastructure, not a test.

Index 0 is the network input, index i conv / dense record i - 1. Per index: absmax = the largest bit pattern of fabsf(v) as uint32,
hist[e] = how many v have biased exponent field e, count = how many v. For a record v = acc + bias in f32, before ReLU and before the
pool, over the rows fnet_exact.gather keeps (those a truncating pool drops are not computed) and the out_c real channels; each record
is fed this model's own previous output (after ReLU and pool), as the kernel feeds its own."""
import numpy as np

import fnet_exact


def of_values(v):
    """(absmax bits, hist[256], count) of a float32 array."""
    bits = np.ascontiguousarray(v, np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7fffffff)
    hist = np.bincount((bits >> np.uint32(23)).astype(np.int64), minlength=256).astype(np.uint64)
    return np.uint32(bits.max() if bits.size else 0), hist, np.uint64(bits.size)


def empty(n_records):
    return dict(absmax=np.zeros(n_records + 1, np.uint32), hist=np.zeros((n_records + 1, 256), np.uint64), count=np.zeros(n_records + 1, np.uint64))


def merge(a, b):
    return dict(absmax=np.maximum(a["absmax"], b["absmax"]), hist=a["hist"] + b["hist"], count=a["count"] + b["count"])


def pre_activation(L, x):
    """acc + bias of conv record L on inputs x [n][in_n]: float32 [n * rows][out_c], rows in the kernel's order."""
    oc = L["out"][2]
    return (fnet_exact.chain(fnet_exact.gather(L, x), L["w"].reshape(oc, -1).T) + L["b"].astype(np.float32)[None, :]).astype(np.float32)


def stats(model, x):
    """The statistic of inputs x [n][in_n] through `model` (cube_import.read_blob form)."""
    recs = fnet_exact.conv_records(model)
    s = empty(len(recs))
    a = np.ascontiguousarray(x, np.float32).reshape(-1, int(np.prod(model["in_shape"])))
    if a.shape[0] == 0:
        return s
    s["absmax"][0], s["hist"][0], s["count"][0] = of_values(a)
    for i, L in enumerate(recs):
        v = pre_activation(L, a)
        s["absmax"][i + 1], s["hist"][i + 1], s["count"][i + 1] = of_values(v)
        oc, P = L["out"][2], L["p"][0] * L["p"][1]
        if L["relu"]:
            v = np.maximum(v, np.float32(0))
        a = v.reshape(-1, P, oc).max(axis=1).reshape(-1, int(np.prod(L["out"]))).astype(np.float32)
    return s

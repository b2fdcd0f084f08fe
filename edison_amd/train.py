"""Training the loaded float32 network on the GPU (``edison_ftrain_*``, include/edison_hip.h): what the reference
does with ``kws_keras.train`` (kws_keras.py:400-416: Adam at 0.0005, batch 100, ReduceLROnPlateau and EarlyStopping on the validation
loss). The gradient and the optimiser step are HIP kernels and the weights never leave the device between steps; the epochs, the
shuffle, the history and the two callbacks are host code here, none of it hot.

    ctx.fnet_load(blob)                       # imported, or cube_import.build_blob(get_model("kws_conv")): a freshly initialised one
    tr = ctx.trainer(padded=True)             # padded: networks with 'same' convs and pools too
    hist = tr.fit(x, y, epochs=30, val=(vx, vy))
    trained = cube_import.build_blob(tr.model())

After a step the context's float network *is* the trained one: fnet, kws_float, streams and the calibrator run the new weights.

From scratch, on a data set that lives on the device: ``get_model`` builds the reference's architectures
(kws_keras.py:170-403 ``get_model``) with Keras's default initialisation, ``Context.train_data`` puts rows and labels (or audio, whose
features are computed there) into device memory once, and ``Trainer.fit_data`` is ``fit`` with each epoch one library call
(``edison_ftrain_epoch``: one gather, a gradient call and a step per batch, one reduction, one synchronisation):

    ctx.fnet_load(cube_import.build_blob(get_model("kws_conv")))
    with ctx.train_data(x, y) as data, ctx.train_data(vx, vy) as val, ctx.trainer(padded=True) as tr:
        hist = tr.fit_data(data, epochs=30, val=val)

``set_opt("adadelta", rho=ADADELTA_RHO)`` is what ``kws_nnom.train`` compiles its model with (kws_nnom.py:121-123).
"""
import ctypes

import numpy as np

from . import _lib, cube_import

ADAM, SGD, ADADELTA = 0, 1, 2   # EDISON_FTRAIN_ADAM, EDISON_FTRAIN_SGD, EDISON_FTRAIN_ADADELTA
FTRAIN_PADDED = 1         # EDISON_FTRAIN_PADDED: edison_ftrain_create_ex's flag
FTRAIN_EVAL = 1           # EDISON_FTRAIN_EVAL: edison_ftrain_grad_ex's flag
FTRAIN_BN_UNBIASED = 1    # EDISON_FTRAIN_BN_UNBIASED: edison_ftrain_set_batchnorm's flag
BN_MOMENTUM, BN_EPS = 0.99, 1e-3   # keras.layers.BatchNormalization's defaults
LEARNING_RATE = 0.0005    # kws_keras.py:53 initial_learningrate
BATCH_SIZE = 100          # kws_keras.py: batchSize
# Keras 2.3.1's 'adadelta' as remembered: lr 1.0, rho 0.95, epsilon 1e-7. Unpinned: no Keras was at hand to read them from.
ADADELTA_LR, ADADELTA_RHO, ADADELTA_EPS = 1.0, 0.95, 1e-7


# Where the reference's architectures put Dropout (kws_keras.py:194-393), per conv / dense record: 0, a rate (behind the record's output)
# or (rate, before_pool); before_pool = 1 is Conv(relu) -> Dropout -> MaxPool. The last record gives the logits: never a rate.
KERAS_DROPOUT = {
    "tiny_conv": [(0.25, 0), 0],
    "medium_embedding_conv": [(0.25, 1), (0.25, 0), 0],
    "tiny_embedding_conv": [(0.25, 1), (0.25, 0), 0],
    "conv_model": [(0.25, 1), (0.25, 0), 0],
    "low_latency_conv": [0.25, 0, 0.25, 0],
    "simple_conv": [(0.25, 0), 0],           # after the pool
    "kws_conv": [0, 0, 0.2, 0.3, 0],
    "single_fc": [0],
}


# Which conv / dense records the reference follows with BatchNormalization (kws_keras.py:194-398): only kws_conv has any, behind each of
# its four convolutions (Conv -> BatchNormalization -> ReLU -> MaxPool / Dropout). The last record gives the logits: never one.
KERAS_BATCHNORM = {
    "tiny_conv": [0, 0],
    "medium_embedding_conv": [0, 0, 0],
    "tiny_embedding_conv": [0, 0, 0],
    "conv_model": [0, 0, 0],
    "low_latency_conv": [0, 0, 0, 0],
    "simple_conv": [0, 0],
    "kws_conv": [1, 1, 1, 1, 0],
    "single_fc": [0],
}


# ---- the model zoo: kws_keras.get_model's architectures as model dicts ----------------------------------------------------------------
ARCHS = ("tiny_conv", "medium_embedding_conv", "tiny_embedding_conv", "conv_model", "low_latency_conv", "single_fc", "simple_conv", "kws_conv")


def _zoo(arch, in_shape, num_classes):
    """kws_keras.py:176-398 as layer specs: ("conv", filters, (rows, columns), strides, padding, pool) with pool None or ((ph, pw),
    padding), every one with ReLU (activation='relu', or kws_conv's ReLU layer), and ("dense", units); Dropout and BatchNorm are
    KERAS_DROPOUT's and KERAS_BATCHNORM's."""
    same22 = ((2, 2), "same")
    return dict(
        tiny_conv=[("conv", 8, (8, 10), (2, 2), "same", None), ("dense", num_classes)],
        medium_embedding_conv=[("conv", 16, (8, 8), (2, 2), "same", same22), ("conv", 12, (4, 4), (1, 1), "same", None), ("dense", num_classes)],
        tiny_embedding_conv=[("conv", 8, (8, 10), (2, 2), "same", same22), ("conv", 8, (8, 10), (8, 8), "same", None), ("dense", num_classes)],
        conv_model=[("conv", 64, (8, 20), (1, 1), "same", same22), ("conv", 64, (4, 10), (1, 1), "same", None), ("dense", num_classes)],
        low_latency_conv=[("conv", 186, (8, in_shape[0]), (1, 4), "same", None), ("dense", 128), ("dense", 128), ("dense", num_classes)],
        single_fc=[("dense", num_classes)],
        simple_conv=[("conv", 8, (8, 8), (1, 1), "same", ((2, 2), "valid")), ("dense", num_classes)],
        kws_conv=[("conv", 16, (5, 5), (1, 1), "valid", ((2, 1), "valid")), ("conv", 32, (3, 3), (1, 1), "valid", ((2, 1), "valid")),
                  ("conv", 64, (3, 3), (1, 1), "valid", None), ("conv", 32, (3, 3), (1, 1), "valid", None), ("dense", num_classes)],
    )[arch]


def _same4(h, w, k, s):
    (t, b), (l, r) = cube_import.same_pads(h, k[0], s[0]), cube_import.same_pads(w, k[1], s[1])
    return t, l, b, r


def glorot_limit(L, dense):
    """Keras's glorot_uniform limit sqrt(6 / (fan_in + fan_out)) of a conv / dense record: a conv's fans are kh kw in_c and kh kw out_c,
    a dense layer's its inputs and outputs."""
    (kh, kw), ic, oc = L["k"], L["inp"][2], L["out"][2]
    fan_in, fan_out = (kh * kw * ic, oc) if dense else (kh * kw * ic, kh * kw * oc)
    return float(np.sqrt(6.0 / (fan_in + fan_out)))


def get_model(arch, in_shape=(31, 13, 1), num_classes=10, seed=0):
    """One of the reference's eight architectures (ARCHS; kws_keras.py:170-403 get_model) as a cube_import model dict that
    cube_import.build_blob takes: MaxPooling2D inside its conv's record (p / ppad), Dense as a conv record whose kernel k = (h, w) is
    its whole input, which Flatten has made 1 x 1 x n (the records the X-CUBE-AI importer writes), 'same' pads from
    cube_import.same_pads, a closing softmax. Keras's default initialisation: every kernel glorot_uniform, every
    bias zero. Record r's kernel is drawn from np.random.default_rng([seed, r]) in float32: the random stream is this library's, not
    TensorFlow's, so the same seed gives the same network here and another one than Keras would. Dropout and BatchNorm are settings of
    the trainer (KERAS_DROPOUT[arch], KERAS_BATCHNORM[arch]), not of the dict. Which dicts the float path runs is the loader's business:
    conv_model and low_latency_conv have layers whose weights exceed the LDS, and load with Context.fnet_load(blob, large=True)."""
    if arch not in ARCHS:
        raise ValueError("arch is one of %s" % ", ".join(ARCHS))
    h, w, c = (int(v) for v in in_shape)
    if min(h, w, c) < 1 or int(num_classes) < 1:
        raise ValueError("in_shape and num_classes are positive")
    layers = []
    for r, spec in enumerate(_zoo(arch, (h, w, c), int(num_classes))):
        if spec[0] == "dense":
            h, w, c = 1, 1, h * w * c          # Flatten: a Dense reads its input as 1 x 1 x n, as the X-CUBE-AI importer's dense records do
            L = dict(type=cube_import.T_CONV, inp=(h, w, c), out=(1, 1, spec[1]), k=(h, w), s=(1, 1), p=(1, 1), relu=0, cpad=(0, 0, 0, 0), ppad=(0, 0, 0, 0))
        else:
            _, oc, k, s, padding, pool = spec
            cpad = _same4(h, w, k, s) if padding == "same" else (0, 0, 0, 0)
            if k[0] > h + cpad[0] + cpad[2] or k[1] > w + cpad[1] + cpad[3]:
                raise ValueError("%s: record %d's %dx%d kernel is larger than its %dx%d input" % (arch, r, k[0], k[1], h, w))
            ch, cw = (h + cpad[0] + cpad[2] - k[0]) // s[0] + 1, (w + cpad[1] + cpad[3] - k[1]) // s[1] + 1
            p, ppad = (1, 1), (0, 0, 0, 0)
            if pool is not None:
                p = pool[0]
                ppad = _same4(ch, cw, p, p) if pool[1] == "same" else ppad
            oh, ow = cube_import.pooled_dim(ch, ppad[0], ppad[2], p[0]), cube_import.pooled_dim(cw, ppad[1], ppad[3], p[1])
            if min(oh, ow) < 1:
                raise ValueError("%s: record %d has no output at input %dx%d" % (arch, r, h, w))
            L = dict(type=cube_import.T_CONV, inp=(h, w, c), out=(oh, ow, oc), k=tuple(k), s=tuple(s), p=tuple(p), relu=1, cpad=cpad, ppad=ppad)
        limit = np.float32(glorot_limit(L, spec[0] == "dense"))
        rng = np.random.default_rng([int(seed), r])
        shape = (L["out"][2],) + L["k"] + (c,)
        L["w"] = ((rng.random(shape, dtype=np.float32) * np.float32(2) - np.float32(1)) * limit).astype(np.float32)   # in [-limit, limit)
        L["b"] = np.zeros(L["out"][2], np.float32)
        layers.append(L)
        h, w, c = L["out"]
    layers.append(dict(type=cube_import.T_SOFTMAX, inp=(h, w, c), out=(h, w, c)))
    return dict(in_shape=tuple(int(v) for v in in_shape), layers=layers)


def dropout_spec(spec, before_pool=None):
    """A list of rates or (rate, before_pool) per record, and optionally the positions apart -> (rates [float], before [0 / 1])."""
    rates, before = [], []
    spec = list(spec)
    if before_pool is not None and len(before_pool) != len(spec):
        raise ValueError("%d rates, %d positions" % (len(spec), len(before_pool)))
    for i, s in enumerate(spec):
        r, b = s if isinstance(s, (tuple, list)) else (s, 0)
        rates.append(float(r))
        before.append(int(bool(b if before_pool is None else before_pool[i])))
    return rates, before


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _t_ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- the packed layout (host, no GPU) ---------------------------------------------------------------------------------------------
def conv_records(model):
    return [L for L in model["layers"] if L["type"] == cube_import.T_CONV]


def layout(model):
    """The packed weight array of a model dict, as the .ednf blob, the kernels and edison_ftrain_layout have it: per conv record
    dict(w_at, K, k_pad, out_c, n_pad, shape=(out_c, kh, kw, in_c)); B[k_pad][n_pad] at w_at, then bias[n_pad]. Returns (records, w_floats)."""
    out, at = [], 0
    for L in conv_records(model):
        (kh, kw), ic, oc = L["k"], L["inp"][2], L["out"][2]
        K = kh * kw * ic
        k_pad, n_pad = (K + 3) // 4 * 4, (oc + 15) // 16 * 16
        out.append(dict(w_at=at, K=K, k_pad=k_pad, out_c=oc, n_pad=n_pad, shape=(oc, kh, kw, ic)))
        at += k_pad * n_pad + n_pad
    return out, at


def unpack(packed, lay):
    """A packed array -> [dict(w [out][kh][kw][in], b [out])] per record, in the array's dtype (the padding is dropped)."""
    packed = np.asarray(packed)
    out = []
    for r in lay:
        nb = r["k_pad"] * r["n_pad"]
        B = packed[r["w_at"]:r["w_at"] + nb].reshape(r["k_pad"], r["n_pad"])
        out.append(dict(w=B[:r["K"], :r["out_c"]].T.reshape(r["shape"]).copy(), b=packed[r["w_at"] + nb:r["w_at"] + nb + r["out_c"]].copy()))
    return out


def pack(tensors, lay, base=None, dtype=np.float32):
    """[dict(w, b)] per record -> the packed array; the padding is `base`'s (a packed array), or zero."""
    n = lay[-1]["w_at"] + lay[-1]["k_pad"] * lay[-1]["n_pad"] + lay[-1]["n_pad"]
    packed = np.zeros(n, dtype) if base is None else np.array(base, dtype).reshape(n)
    if len(tensors) != len(lay):
        raise ValueError("%d records, the network has %d" % (len(tensors), len(lay)))
    for t, r in zip(tensors, lay):
        w, b = np.asarray(t["w"]), np.asarray(t["b"])
        if w.shape != r["shape"] or b.shape != (r["out_c"],):
            raise ValueError("a record's w %s / b %s, the network has %s / (%d,)" % (w.shape, b.shape, r["shape"], r["out_c"]))
        nb = r["k_pad"] * r["n_pad"]
        packed[r["w_at"]:r["w_at"] + nb].reshape(r["k_pad"], r["n_pad"])[:r["K"], :r["out_c"]] = w.reshape(r["out_c"], r["K"]).T
        packed[r["w_at"] + nb:r["w_at"] + nb + r["out_c"]] = b
    return packed


# ---- the host side of fit: shuffle and callbacks ----------------------------------------------------------------------------------
def epoch_order(n, seed, epoch):
    """The order of the n rows in epoch `epoch` (from 0): a permutation that depends on (seed, epoch) only."""
    return np.random.default_rng([int(seed), int(epoch)]).permutation(int(n))


class ReduceLROnPlateau:
    """keras.callbacks.ReduceLROnPlateau(factor=0.5, patience=1, min_lr=1e-9) on a loss (mode min, min_delta 1e-4, no cooldown): an
    epoch that does not improve the best loss by more than min_delta counts; after `patience` such epochs the rate is multiplied by
    factor, not below min_lr, and the count starts again."""

    def __init__(self, factor=0.5, patience=1, min_lr=1e-9, min_delta=1e-4):
        self.factor, self.patience, self.min_lr, self.min_delta = float(factor), int(patience), float(min_lr), float(min_delta)
        self.best, self.wait = np.inf, 0

    def update(self, loss, lr):
        """The epoch's monitored loss and the current rate -> the rate of the next epoch."""
        if loss < self.best - self.min_delta:
            self.best, self.wait = loss, 0
            return lr
        self.wait += 1
        if self.wait >= self.patience:
            self.wait = 0
            if lr > self.min_lr:
                return max(lr * self.factor, self.min_lr)
        return lr


class EarlyStopping:
    """keras.callbacks.EarlyStopping(patience=10) on a loss (min_delta 0): stop after `patience` epochs in a row that did not go
    below the best loss so far."""

    def __init__(self, patience=10):
        self.patience, self.best, self.wait = int(patience), np.inf, 0

    def update(self, loss):
        """The epoch's monitored loss -> True when training stops here."""
        if loss < self.best:
            self.best, self.wait = loss, 0
            return False
        self.wait += 1
        return self.wait >= self.patience


def _fit_epochs(run_epoch, run_val, epochs, batch_size, lr, max_steps, callbacks):
    """The epoch loop of fit and fit_data: the history, the two callbacks on the validation loss, the max_steps cut. run_epoch(epoch, lr,
    steps_left or None) -> (loss_sum, hits, seen, steps) trains one epoch, run_val() -> (loss_sum, hits, n) evaluates; run_val may be None."""
    if int(batch_size) < 1 or int(epochs) < 0:
        raise ValueError("batch_size must be at least 1 and epochs at least 0")
    plateau, stopper = ReduceLROnPlateau(), EarlyStopping()
    hist = dict(loss=[], acc=[], val_loss=[], val_acc=[], lr=[], steps=0, stopped_early=False)
    for epoch in range(int(epochs)):
        loss_sum, hits, seen, steps = run_epoch(epoch, lr, None if max_steps is None else max(max_steps - hist["steps"], 0))
        hist["steps"] += steps
        if not seen:
            break
        hist["loss"].append(loss_sum / seen)             # as Keras: the mean over the epoch's batches, weights moving
        hist["acc"].append(hits / seen)
        hist["lr"].append(lr)
        if run_val is not None:
            vl, vh, vn = run_val()
            hist["val_loss"].append(vl / max(vn, 1))
            hist["val_acc"].append(vh / max(vn, 1))
            if callbacks:
                lr = plateau.update(hist["val_loss"][-1], lr)
                if stopper.update(hist["val_loss"][-1]):
                    hist["stopped_early"] = True
                    break
        if max_steps is not None and hist["steps"] >= max_steps:
            break
    return hist


def fit(trainer, x, y, epochs, batch_size=BATCH_SIZE, val=None, seed=0, lr=LEARNING_RATE, max_steps=None, callbacks=True):
    """Trainer.fit on anything with grad(x, y) -> dict(loss [n], argmax [n]) and step(lr): the GPU trainer, or a host restatement of it."""
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1)
    y = np.asarray(y).astype(np.int32).reshape(-1)
    if x.shape[0] != y.shape[0] or x.shape[0] == 0:
        raise ValueError("x has %d rows, y %d" % (x.shape[0], y.shape[0]))
    n, bs = x.shape[0], int(batch_size)
    if val is not None:
        vx, vy = np.asarray(val[0]), np.asarray(val[1]).astype(np.int32).reshape(-1)
        vx = vx.reshape(vx.shape[0], -1)
    # validation runs with dropout off and on BatchNorm's moving statistics: the keyword goes only to a trainer that reports one of them
    # on, so anything without them keeps working
    state = trainer.dropout() if hasattr(trainer, "dropout") else None
    bn = trainer.batchnorm() if hasattr(trainer, "batchnorm") else None
    ev = dict(training=False) if (state and state.get("on")) or (bn and bn.get("on")) else {}

    def run_epoch(epoch, lr, steps_left):
        order = epoch_order(n, seed, epoch)
        loss_sum, hits, seen, steps = 0.0, 0, 0, 0
        for b0 in range(0, n, bs):                       # the last batch may be short
            if steps_left is not None and steps >= steps_left:
                break
            rows = order[b0:b0 + bs]
            r = trainer.grad(x[rows], y[rows])               # a training call: with dropout set, its mask and the counter's advance
            trainer.step(lr)
            steps += 1
            loss_sum += float(np.sum(r["loss"], dtype=np.float64))
            hits += int((r["argmax"] == y[rows]).sum())
            seen += len(rows)
        return loss_sum, hits, seen, steps

    def run_val():
        vl, vh = 0.0, 0
        for b0 in range(0, vx.shape[0], 4096):
            r = trainer.grad(vx[b0:b0 + 4096], vy[b0:b0 + 4096], **ev)   # the gradient it leaves is not stepped
            vl += float(np.sum(r["loss"], dtype=np.float64))
            vh += int((r["argmax"] == vy[b0:b0 + 4096]).sum())
        return vl, vh, vx.shape[0]

    return _fit_epochs(run_epoch, None if val is None else run_val, epochs, batch_size, lr, max_steps, callbacks)


def fit_data(trainer, data, epochs, batch_size=BATCH_SIZE, val=None, seed=0, lr=LEARNING_RATE, max_steps=None, callbacks=True):
    """fit on anything with epoch(data, order, batch, lr, max_steps) and evaluate(data), both -> dict(loss_sum, hits, seen, steps): the
    same orders, callbacks and history, each epoch one call."""
    if data.n == 0:
        raise ValueError("the data set is empty")

    def run_epoch(epoch, lr, steps_left):
        r = trainer.epoch(data, epoch_order(data.n, seed, epoch), int(batch_size), lr, steps_left)
        return r["loss_sum"], r["hits"], r["seen"], r["steps"]

    def run_val():
        v = trainer.evaluate(val)
        return v["loss_sum"], v["hits"], val.n

    return _fit_epochs(run_epoch, None if val is None else run_val, epochs, batch_size, lr, max_steps, callbacks)


# ---- a data set on the device -----------------------------------------------------------------------------------------------------
class DeviceData:
    """edison_ftrain_data on `ctx` (Context.train_data): rows [n][in_n] float32 and labels [n] int32 in device memory, owned by the
    context, not by a trainer: it outlives trainers and network loads, and Context.close closes it."""

    def __init__(self, ctx, in_n):
        self._ctx, self._L = ctx, ctx._L
        h = ctypes.c_void_p()
        ctx._check(self._L.edison_ftrain_data_create(ctx._h, int(in_n), ctypes.byref(h)))
        self._h = h
        ctx._train_data.add(self)                    # Context.close closes it first

    def close(self):
        if getattr(self, "_h", None):
            self._L.edison_ftrain_data_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _info(self):
        n, in_n = ctypes.c_int64(), ctypes.c_int32()
        self._ctx._check(self._L.edison_ftrain_data_info(self._h, ctypes.byref(n), ctypes.byref(in_n)))
        return n.value, in_n.value

    @property
    def n(self):
        return self._info()[0]

    @property
    def in_n(self):
        return self._info()[1]

    def set(self, x, y):
        """edison_ftrain_data_set: host rows [n][in_n] (any shape with n first) and class indices [n], uploaded once; replaces the contents."""
        lab = np.ascontiguousarray(y).reshape(-1)
        if lab.shape[0] and (lab.min() < 0 or lab.max() >= 2 ** 31):
            raise ValueError("a label is outside [0, 2^31)")
        lab = lab.astype(np.int32)
        f = np.ascontiguousarray(x, dtype=np.float32).reshape(lab.shape[0], -1)
        if lab.shape[0] and f.shape[1] != self.in_n:
            raise ValueError("rows of %d floats, the data set's have %d" % (f.shape[1], self.in_n))
        self._ctx._check(self._L.edison_ftrain_data_set(self._h, _np_ptr(f), _np_ptr(lab), lab.shape[0]))

    def set_t(self, x, y, n=None):
        """edison_ftrain_data_set_dev: torch device tensors x float32 [n][in_n], y int32 [n], contiguous."""
        self._ctx._check(self._L.edison_ftrain_data_set_dev(self._h, _t_ptr(x), _t_ptr(y), int(x.shape[0] if n is None else n)))

    def set_audio(self, audio, y, geometry=None, q15=False, clip_min=None, clip_max=None, chunk=16384, utt_stride=None):
        """edison_ftrain_data_audio: int16 utterances [n][samples] (or flat, utt_stride apart) -> their float-flow features, computed on the
        device chunk by chunk straight into the store: Context.kws_float's feat for the same arguments, bit for bit."""
        from . import config as cfg
        from .kws.geometry import KwsGeometry
        if geometry is None:
            geometry = KwsGeometry.from_config(net_input_scale=cfg.net_input_scale)
        lo = float(cfg.net_input_clip_min if clip_min is None else clip_min)
        hi = float(cfg.net_input_clip_max if clip_max is None else clip_max)
        lab = np.ascontiguousarray(y).reshape(-1)
        if lab.shape[0] and (lab.min() < 0 or lab.max() >= 2 ** 31):
            raise ValueError("a label is outside [0, 2^31)")
        lab = lab.astype(np.int32)
        a = np.ascontiguousarray(audio, dtype=np.int16)
        stride = int((a.shape[-1] if a.ndim == 2 else geometry.n_samples) if utt_stride is None else utt_stride)
        a = a.ravel()
        used = (geometry.frame_count - 1) * geometry.frame_step + geometry.frame_len
        if lab.shape[0] and (lab.shape[0] - 1) * stride + used > a.shape[0]:
            raise ValueError("audio too short for %d utterances" % lab.shape[0])
        g = geometry.to_ctypes()
        self._ctx._check(self._L.edison_ftrain_data_audio(self._h, ctypes.byref(g), 1 if q15 else 0, lo, hi, _np_ptr(a), lab.shape[0], stride,
                                                          _np_ptr(lab), int(chunk)))

    def rows(self):
        """(x float32 [n][in_n], y int32 [n]) copied back (synchronises)."""
        n, in_n = self._info()
        x, y = np.zeros((n, in_n), np.float32), np.zeros(n, np.int32)
        self._ctx._check(self._L.edison_ftrain_data_get(self._h, _np_ptr(x), _np_ptr(y)))
        return x, y


# ---- the GPU trainer --------------------------------------------------------------------------------------------------------------
class Trainer:
    """edison_ftrain on `ctx`, bound to the float network loaded now; loading another one invalidates it (EdisonError).
    padded=True (EDISON_FTRAIN_PADDED) also takes networks with conv or pool pads; without it they are refused.
    dropout: set_dropout's rates (None: off), with `seed`. batchnorm: set_batchnorm's records (None: off), or a dict of its arguments."""

    def __init__(self, ctx, padded=False, dropout=None, seed=0, batchnorm=None):
        self._ctx, self._L = ctx, ctx._L
        if ctx._fnet_blob is None:
            raise ValueError("no float network loaded (fnet_load)")
        h = ctypes.c_void_p()
        ctx._check(self._L.edison_ftrain_create_ex(ctx._h, FTRAIN_PADDED if padded else 0, ctypes.byref(h)))
        self._h = h
        self._model = cube_import.read_blob(ctx._fnet_blob)
        info = self.info()
        self.in_n, self.n_out, self.w_floats, self.n_layers = info["in_n"], info["n_out"], info["w_floats"], info["n_layers"]
        self.layout, n = layout(self._model)
        for i, r in enumerate(self.layout):                       # the library's layout is the one unpack / pack restate
            got = self.record_layout(i)
            if any(got[k] != r[k] for k in ("w_at", "K", "k_pad", "out_c", "n_pad")) or n != self.w_floats:
                raise RuntimeError("record %d: edison_ftrain_layout %s, the blob's %s" % (i, got, r))
        if dropout is not None:
            self.set_dropout(dropout, seed=seed)
        if batchnorm is not None:
            self.set_batchnorm(**batchnorm) if isinstance(batchnorm, dict) else self.set_batchnorm(batchnorm)

    def close(self):
        if getattr(self, "_h", None):
            if self._ctx._fnet_trainer is self:
                self.export()
            self._L.edison_ftrain_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        """dict of edison_ftrain_info_t: n_layers, in_n, n_out, batch, lds_bytes, grid, w_floats, steps, ignored (synchronises)."""
        info = _lib.FtrainInfo()
        self._ctx._check(self._L.edison_ftrain_info(self._h, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in _lib.FtrainInfo._fields_}

    def record_layout(self, record):
        """edison_ftrain_layout: dict(w_at, K, k_pad, out_c, n_pad) of conv / dense record `record`."""
        w_at = ctypes.c_int64()
        v = [ctypes.c_int32() for _ in range(4)]
        self._ctx._check(self._L.edison_ftrain_layout(self._h, int(record), ctypes.byref(w_at), *[ctypes.byref(a) for a in v]))
        return dict(w_at=w_at.value, K=v[0].value, k_pad=v[1].value, out_c=v[2].value, n_pad=v[3].value)

    # -- dropout
    def set_dropout(self, rates, before_pool=None, seed=0):
        """edison_ftrain_set_dropout: per conv / dense record a rate in [0, 1) behind its output, or (rate, before_pool) (KERAS_DROPOUT's
        form); before_pool [n_layers] gives the positions apart (1: between ReLU and the pool). The last record's rate is 0. All rates
        0 turns dropout off. Sets the call counter to 0."""
        r, b = dropout_spec(rates, before_pool)
        ra, ba = np.asarray(r, np.float64), np.asarray(b, np.uint8)
        self._ctx._check(self._L.edison_ftrain_set_dropout(self._h, _np_ptr(ra), _np_ptr(ba), len(r), int(seed) & (2 ** 64 - 1)))

    def dropout(self):
        """edison_ftrain_dropout_get: dict(rates, before_pool, seed, call, on)."""
        ra, ba = np.zeros(self.n_layers, np.float64), np.zeros(self.n_layers, np.uint8)
        seed, call = ctypes.c_uint64(), ctypes.c_uint64()
        self._ctx._check(self._L.edison_ftrain_dropout_get(self._h, _np_ptr(ra), _np_ptr(ba), ctypes.byref(seed), ctypes.byref(call)))
        return dict(rates=[float(v) for v in ra], before_pool=[int(v) for v in ba], seed=seed.value, call=call.value, on=bool((ra > 0).any()))

    @property
    def dropout_call(self):
        """The call counter: the mask of the next training call is a function of (seed, this); a training call advances it by one."""
        return self.dropout()["call"]

    @dropout_call.setter
    def dropout_call(self, call):
        self._ctx._check(self._L.edison_ftrain_set_dropout_call(self._h, int(call)))

    # -- BatchNorm
    def set_batchnorm(self, has_bn, momentum=BN_MOMENTUM, eps=BN_EPS, max_rows=None, unbiased=False):
        """edison_ftrain_set_batchnorm: has_bn per conv / dense record, 1 where conv + bias is followed by BatchNorm (KERAS_BATCHNORM's
        form; never the last record, and no record of the network may have a pad). Batch statistics over every row of a training call
        and the whole conv map; the moving statistics move by `momentum` (unbiased=True: by var N / (N - 1), torch's rule). A training
        call takes at most max_rows rows (None: 1024). From here on weights() / set_weights() are the master weights, gamma and beta
        train beside them, and the context runs the folded inference-mode network, which model() and export() give. Once per trainer."""
        hb = np.ascontiguousarray([1 if v else 0 for v in has_bn], dtype=np.uint8)
        self._ctx._check(self._L.edison_ftrain_set_batchnorm(self._h, _np_ptr(hb), len(hb), float(momentum), float(eps),
                                                             0 if max_rows is None else int(max_rows), FTRAIN_BN_UNBIASED if unbiased else 0))
        self._ctx._fnet_trainer = self          # the device weights are the folded ones now: W / sqrt(1 + eps)

    def batchnorm(self):
        """edison_ftrain_batchnorm_get: dict(on: set_batchnorm was called, whatever it marked (the library reports max_rows 0 until then), has_bn, momentum, eps, max_rows, unbiased, batch: utterances per tile of a training call)."""
        hb = np.zeros(self.n_layers, np.uint8)
        m, e, rows, fl, batch = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64(), ctypes.c_uint32(), ctypes.c_int32()
        self._ctx._check(self._L.edison_ftrain_batchnorm_get(self._h, _np_ptr(hb), ctypes.byref(m), ctypes.byref(e), ctypes.byref(rows), ctypes.byref(fl),
                                                             ctypes.byref(batch)))
        return dict(on=rows.value > 0, has_bn=[int(v) for v in hb], momentum=m.value, eps=e.value, max_rows=rows.value,
                    unbiased=bool(fl.value & FTRAIN_BN_UNBIASED), batch=batch.value)

    def _bn_records(self):
        return [i for i, v in enumerate(self.batchnorm()["has_bn"]) if v]

    def bn_state(self):
        """Per conv / dense record None, or dict(gamma, beta, mean, var) float32 [out_c]: the moving statistics."""
        out = [None] * self.n_layers
        for i in self._bn_records():
            a = {k: np.zeros(self.layout[i]["out_c"], np.float32) for k in ("gamma", "beta", "mean", "var")}
            self._ctx._check(self._L.edison_ftrain_bn_get(self._h, i, *[_np_ptr(a[k]) for k in ("gamma", "beta", "mean", "var")]))
            out[i] = a
        return out

    def set_bn_state(self, state):
        """bn_state's inverse: per record None (unchanged) or a dict with any of gamma, beta, mean, var; refolds the network."""
        if len(state) != self.n_layers:
            raise ValueError("%d records, the network has %d" % (len(state), self.n_layers))
        for i, st in enumerate(state):
            if st is None:
                continue
            a = {k: np.ascontiguousarray(st[k], dtype=np.float32).reshape(-1) for k in ("gamma", "beta", "mean", "var") if st.get(k) is not None}
            if any(v.shape[0] != self.layout[i]["out_c"] for v in a.values()):
                raise ValueError("record %d has %d channels" % (i, self.layout[i]["out_c"]))
            self._ctx._check(self._L.edison_ftrain_bn_set(self._h, i, *[_np_ptr(a.get(k)) for k in ("gamma", "beta", "mean", "var")]))
            self._ctx._fnet_trainer = self

    def bn_batch_stats(self):
        """The last training call's batch statistics: per record None or dict(mean, var) float32 [out_c]."""
        out = [None] * self.n_layers
        for i in self._bn_records():
            a = {k: np.zeros(self.layout[i]["out_c"], np.float32) for k in ("mean", "var")}
            self._ctx._check(self._L.edison_ftrain_bn_batch_get(self._h, i, _np_ptr(a["mean"]), _np_ptr(a["var"])))
            out[i] = a
        return out

    def bn_gradients(self):
        """The last training call's gradient of gamma and beta: per record None or dict(gamma, beta) float32 [out_c]."""
        out = [None] * self.n_layers
        for i in self._bn_records():
            a = {k: np.zeros(self.layout[i]["out_c"], np.float32) for k in ("gamma", "beta")}
            self._ctx._check(self._L.edison_ftrain_bn_grad_get(self._h, i, _np_ptr(a["gamma"]), _np_ptr(a["beta"])))
            out[i] = a
        return out

    def folded_weights(self):
        """The loaded network's device weights as [dict(w, b)]: with BatchNorm on the folded inference-mode network, else weights()."""
        w = np.zeros(self.w_floats, np.float32)
        self._ctx._check(self._L.edison_ftrain_folded_get(self._h, _np_ptr(w)))
        return unpack(w, self.layout)

    # -- the gradient
    def grad(self, x, y, training=True):
        """Host inputs [n][in_n] float32 and labels [n] (class indices; one outside [0, n_out) is an EdisonError) -> dict(loss [n],
        argmax [n]). The gradient stays on the device: gradient() / gradients() fetch it, step() applies it. With dropout set a call
        applies the current counter's mask and advances the counter; training=False (EDISON_FTRAIN_EVAL) does neither."""
        f = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, self.in_n)
        lab = np.ascontiguousarray(y, dtype=np.int32).reshape(-1)
        if lab.shape[0] != f.shape[0]:
            raise ValueError("%d inputs, %d labels" % (f.shape[0], lab.shape[0]))
        loss = np.zeros(f.shape[0], np.float32)
        am = np.zeros(f.shape[0], np.int32)
        if training:
            self._ctx._check(self._L.edison_ftrain_grad(self._h, _np_ptr(f), _np_ptr(lab), f.shape[0], _np_ptr(loss), _np_ptr(am)))
        else:
            self._ctx._check(self._L.edison_ftrain_grad_ex(self._h, _np_ptr(f), _np_ptr(lab), f.shape[0], _np_ptr(loss), _np_ptr(am), FTRAIN_EVAL))
        return dict(loss=loss, argmax=am)

    def grad_t(self, x, y, n=None, loss=None, argmax=None, training=True):
        """edison_ftrain_grad_dev on torch device tensors (x float32 [n][in_n], y int32 [n], contiguous; loss float32 [n] and argmax
        int32 [n] optional), enqueued on the context's stream behind whatever produced them. A label outside [0, n_out) contributes
        nothing and is counted in info()["ignored"]. training: as grad's."""
        n = int(x.shape[0] if n is None else n)
        if training:
            self._ctx._check(self._L.edison_ftrain_grad_dev(self._h, _t_ptr(x), _t_ptr(y), n, _t_ptr(loss), _t_ptr(argmax)))
        else:
            self._ctx._check(self._L.edison_ftrain_grad_dev_ex(self._h, _t_ptr(x), _t_ptr(y), n, _t_ptr(loss), _t_ptr(argmax), FTRAIN_EVAL))

    def gradient(self):
        """The last call's gradient, packed float32 [w_floats] (synchronises)."""
        g = np.zeros(self.w_floats, np.float32)
        self._ctx._check(self._L.edison_ftrain_grad_get(self._h, _np_ptr(g)))
        return g

    def gradients(self):
        """The last call's gradient as [dict(w [out][kh][kw][in], b [out])] per conv / dense record."""
        return unpack(self.gradient(), self.layout)

    def logits(self, n):
        """The last gradient call's logits float32 [n][n_out] (n: that call's); edison_fnet_batch's bit for bit."""
        z = np.zeros((int(n), self.n_out), np.float32)
        self._ctx._check(self._L.edison_ftrain_logits_get(self._h, _np_ptr(z)))
        return z

    # -- the optimiser
    def set_opt(self, kind="adam", b1=0.9, b2=0.999, eps=1e-7, rho=None):
        """Adam (Keras's constants by default), kind "sgd": w -= lr g, or kind "adadelta" with rho and eps (a = rho a + (1 - rho) g g,
        u = g sqrt(d + eps) / sqrt(a + eps), w -= lr u, d = rho d + (1 - rho) u u; Keras's learning rate for it is ADADELTA_LR = 1.0).
        Adadelta's rho has no default here: Keras's is unpinned (ADADELTA_RHO is what is remembered), so set_opt("adadelta", rho=...)
        states it and a bare set_opt("adadelta") stays the ValueError it was before the kind existed. rho belongs to Adadelta alone."""
        kinds = dict(adam=ADAM, sgd=SGD, adadelta=ADADELTA)
        if kind not in kinds:
            raise ValueError("kind is 'adam', 'sgd' or 'adadelta'")
        if (kind == "adadelta") != (rho is not None):
            raise ValueError("kind 'adadelta' takes rho (train.ADADELTA_RHO is Keras's, unpinned), and no other kind does")
        if kind == "adadelta":
            b1, b2 = rho, 0.0
        self._ctx._check(self._L.edison_ftrain_set_opt(self._h, kinds[kind], float(b1), float(b2), float(eps)))

    def step(self, lr=LEARNING_RATE):
        """One optimiser step with the last gradient, in place on the context's loaded network."""
        self._ctx._check(self._L.edison_ftrain_step(self._h, float(lr)))
        self._ctx._fnet_trainer = self          # the context's copy of the blob is behind the device weights now

    def reset(self):
        """Zero Adam's moments, its step count, the ignored-row counter and dropout's call counter."""
        self._ctx._check(self._L.edison_ftrain_reset(self._h))

    # -- the weights
    def packed_weights(self):
        w = np.zeros(self.w_floats, np.float32)
        self._ctx._check(self._L.edison_ftrain_weights_get(self._h, _np_ptr(w)))
        return w

    def set_packed_weights(self, packed):
        w = np.ascontiguousarray(packed, dtype=np.float32).reshape(-1)
        if w.shape[0] != self.w_floats:
            raise ValueError("%d floats, the network has %d" % (w.shape[0], self.w_floats))
        self._ctx._check(self._L.edison_ftrain_weights_set(self._h, _np_ptr(w)))
        self._ctx._fnet_trainer = self

    def weights(self):
        """The trained weights now: [dict(w [out][kh][kw][in], b [out])] float32 per conv / dense record, the model dict's layout. With
        BatchNorm on these are the master weights; folded_weights() are what the context runs."""
        return unpack(self.packed_weights(), self.layout)

    def set_weights(self, tensors):
        """weights()' inverse: every record's w and b onto the device; the packed array's padding stays what it is."""
        self.set_packed_weights(pack(tensors, self.layout, base=self.packed_weights()))

    def model(self):
        """The cube_import model dict of the network with the device weights now (with BatchNorm: folded into the convolutions, as
        X-CUBE-AI would see it): cube_import.build_blob(trainer.model(), trainer.model()["keywords"]) is the trained .ednf."""
        m = dict(self._model, layers=[dict(L) for L in self._model["layers"]])
        for L, t in zip(conv_records(m), self.folded_weights()):
            L["w"], L["b"] = t["w"], t["b"]
        return m

    def export(self):
        """The trained .ednf: cube_import.build_blob of model() with the network's keywords. The context keeps it as the loaded
        network's blob, which Context.quantize reads the weights from."""
        m = self.model()
        blob = cube_import.build_blob(m, m.get("keywords"))
        self._ctx._fnet_blob, self._ctx._fnet_trainer = blob, None
        return blob

    def fit(self, x, y, epochs, batch_size=BATCH_SIZE, val=None, seed=0, lr=LEARNING_RATE, max_steps=None, callbacks=True):
        """Train on x [n][in_n] and class indices y [n]: per epoch the rows in epoch_order(n, seed, epoch), batches of batch_size (the
        last one short), one gradient call and one Adam step each. val = (x, y): after every epoch its loss and accuracy, and on that
        loss the reference's two callbacks (callbacks=False: none). max_steps ends training after that many steps, inside an epoch if
        need be. Returns the history: loss, acc (the means over each epoch's batches, as Keras), val_loss, val_acc, lr per epoch, steps,
        stopped_early."""
        return fit(self, x, y, epochs, batch_size=batch_size, val=val, seed=seed, lr=lr, max_steps=max_steps, callbacks=callbacks)

    # -- whole epochs on a data set on the device
    def epoch(self, data, order, batch_size=BATCH_SIZE, lr=LEARNING_RATE, max_steps=None):
        """edison_ftrain_epoch: the rows order[i] of `data` (a DeviceData) in batches of batch_size, a gradient call and a step each, one
        synchronisation -> dict(loss_sum, hits, seen, steps)."""
        o = np.asarray(order).reshape(-1)
        if o.shape[0] and (o.min() < -2 ** 31 or o.max() >= 2 ** 31):
            raise ValueError("an index of order does not fit int32")
        o = np.ascontiguousarray(o, dtype=np.int32)
        out = _lib.FtrainEpoch()
        self._ctx._check(self._L.edison_ftrain_epoch(self._h, data._h, _np_ptr(o), o.shape[0], int(batch_size), float(lr),
                                                     -1 if max_steps is None else int(max_steps), ctypes.byref(out)))
        if out.steps:
            self._ctx._fnet_trainer = self          # the context's copy of the blob is behind the device weights now
        return dict(loss_sum=out.loss_sum, hits=out.hits, seen=out.seen, steps=out.steps)

    def evaluate(self, data):
        """edison_ftrain_data_eval: every row of `data` through EDISON_FTRAIN_EVAL calls -> dict(loss_sum, hits, seen, steps = 0)."""
        out = _lib.FtrainEpoch()
        self._ctx._check(self._L.edison_ftrain_data_eval(self._h, data._h, ctypes.byref(out)))
        return dict(loss_sum=out.loss_sum, hits=out.hits, seen=out.seen, steps=out.steps)

    def epoch_rows(self):
        """edison_ftrain_epoch_rows: dict(loss [n], argmax [n]) of the last epoch or evaluate call, in the order the rows were run."""
        n = ctypes.c_int64()
        self._ctx._check(self._L.edison_ftrain_epoch_rows(self._h, None, None, ctypes.byref(n)))
        loss, am = np.zeros(n.value, np.float32), np.zeros(n.value, np.int32)
        self._ctx._check(self._L.edison_ftrain_epoch_rows(self._h, _np_ptr(loss), _np_ptr(am), None))
        return dict(loss=loss, argmax=am)

    def fit_data(self, data, epochs, batch_size=BATCH_SIZE, val=None, seed=0, lr=LEARNING_RATE, max_steps=None, callbacks=True):
        """fit on a DeviceData (Context.train_data): the same epoch_order, callbacks and history, with each epoch's inner loop one
        edison_ftrain_epoch call and the validation (val: a DeviceData) one edison_ftrain_data_eval call."""
        return fit_data(self, data, epochs, batch_size=batch_size, val=val, seed=seed, lr=lr, max_steps=max_steps, callbacks=callbacks)

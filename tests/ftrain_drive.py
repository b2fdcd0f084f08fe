"""The one driver of the float32 trainer's GPU tests (test_gpu_ftrain, _pad, _tiles, _dropout, _bn, _data). Test
infrastructure, not a test; tests/test_ftrain_drive_cpu.py checks its pure pieces. The rows and their references are
tests/ftrain_rows.py's, the mathematics tests/ftrain_ref.py's.

  same_bits       the one array comparison: shape, dtype and bits (stream_drive.same's strictness, as a truth value)
  poisoned, case, loaded   a network with 1e6 in all its weight padding, built once per process
  data, rows      the inputs of a row; rows is the prefix-stable draw of the multi-tile tests
  check_plan, check_gradient, check_call, check_fold   one gradient call held to the restated plan, to float64, in every way, and
                  a multi-tile call as the exact fold of its tiles
  step_errors, step_checked   one step against its float64 replay from the GPU's own gradient
  own_context     the body of the files' module-scoped ctx / fresh fixtures
  kws_files, kws_trained, kws_audio, kws_quantized   the shared parts of the `kws train` then `kws quantize` tests
  fit_kw, check_fit_learns, follows_replay   the shared parts of the fit tests"""
import hashlib
import io
import os
import types

import numpy as np

import fnet_host
import fnet_plan
import fnet_rows
import ftrain_ref
import ftrain_rows
import stream_drive
from edison_amd import cube_import, train

EPS = 2.0 ** -24
POISON = np.float32(1.0e6)


# ---- small pieces -------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """Bit for bit: the same shape, the same dtype, float32 compared as uint32 (-0.0 is not +0.0, a NaN equals its own bit pattern)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(stream_drive.bits(a), stream_drive.bits(b))


def pow2_at_least(v):
    return 1 << max(int(v) - 1, 0).bit_length()


def own_context():
    """The body of a module-scoped fixture: a context of the module's own, closed behind its last test."""
    from edison_amd.context import Context
    c = Context(0)
    yield c
    c.close()


# ---- networks with poisoned padding ---------------------------------------------------------------------------------------------------
def poisoned(blob, value=1.0e6):
    """(the blob with `value` in every padding k row, padding channel and padding bias of its weights, the mask of the packed array's
    real entries)."""
    model = cube_import.read_blob(blob)
    lay, n = train.layout(model)
    w = np.frombuffer(blob, "<f4", n, len(blob) - 4 * n).copy()
    real = train.pack([dict(w=np.ones(r["shape"], np.float32), b=np.ones(r["out_c"], np.float32)) for r in lay], lay) != 0
    w[~real] = value
    return blob[:len(blob) - 4 * n] + w.astype("<f4").tobytes(), real


_CASES, _POISONED, _ROWS = {}, {}, {}


def case(name):
    """(model, blob with poisoned padding, mask of the packed array's real entries) of "cube_kws" (tests/golden/cube_kws.ednf), a row of
    ftrain_rows.PAD_ROWS or any other row of fnet_rows, built once."""
    if name not in _CASES:
        if name in ftrain_rows.PAD_ROWS:
            model, blob = ftrain_rows.pad_model(name), ftrain_rows.pad_blob(name)
        else:
            if name == "cube_kws":
                with open(stream_drive.FIXTURE, "rb") as f:
                    blob = f.read()
            else:
                blob = fnet_rows.blob(name)
            model = cube_import.read_blob(blob)
        _CASES[name] = (model,) + poisoned(blob)
    return _CASES[name]


def loaded(ctx, c):
    """A case dict of ftrain_rows (bn_case, drop_case) loaded with poisoned padding, poisoned once -> (the case, the mask of the packed
    array's real entries)."""
    if c["blob"] not in _POISONED:
        _POISONED[c["blob"]] = poisoned(c["blob"])
    bad, real = _POISONED[c["blob"]]
    ctx.fnet_load(bad)
    return c, real


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _labels(model, n):
    return (np.arange(n) % int(np.prod(fnet_host.conv_records(model)[-1]["out"]))).astype(np.int32)


def data(name, model, n):
    """(x [n][in_n], labels i % n_out): the shipped network's fixture rows in turn, relu_logits' all-negative set, else
    ftrain_ref.inputs."""
    in_n = int(np.prod(model["in_shape"]))
    if name == "cube_kws":
        g = np.load(os.path.join(ftrain_rows.GOLDEN, "cube_golden.npz"))
        fixture = np.stack([g["net_in_" + str(k)] for k in g["names"]]).astype(np.float32)
        x = fixture[np.arange(n) % len(fixture)]
    elif name == "relu_logits":
        assert fnet_rows.SWEEP[name][0]["sets"] == ["neg", "n1"]
        x = np.ascontiguousarray(fnet_rows.inputs(name, 2 * n, in_n)[0::2])      # its all-negative inputs: every ReLU logit is zero
    else:
        x = ftrain_ref.inputs(name, n, in_n)
    return x, _labels(model, n)


def rows(name, model, n, exact=False):
    """The first n rows and labels of a row's draw, made once for the largest n asked so far (a prefix of a longer draw is the
    shorter draw). exact=False: data's, the sets n1, zero and neg. exact=True, for the scaling argument of check_fold: N(0, 1) rows
    only -- the neg set saturates the softmax, its dz reaches down to 1e-37 and dz / N leaves the normal range --, and for the shipped
    network the fixture rows, which repeat, each with N(0, 1 % of its own sigma) noise, so that no two tiles are equal. Fixed seeds."""
    key = (name, exact)
    if key not in _ROWS or len(_ROWS[key][1]) < n:
        rng = np.random.default_rng(586 + sum(map(ord, name)))
        if exact and name != "cube_kws":
            x, y = rng.normal(0, 1, (n, int(np.prod(model["in_shape"])))).astype(np.float32), _labels(model, n)
        else:
            x, y = data(name, model, n)
            if exact:
                x = (x + rng.normal(0, 1, x.shape) * 0.01 * x.std(axis=1, keepdims=True)).astype(np.float32)
        _ROWS[key] = (x, y)
    x, y = _ROWS[key]
    return x[:n], y[:n]


def tile_labels(y, b, n1):
    """int32 [tiles][n1] for the small calls of check_fold: tile j's own labels of y first, -1 fillers behind."""
    n_tiles = (len(y) + b - 1) // b
    labels = np.full((n_tiles, n1), -1, np.int32)
    for j in range(n_tiles):
        own = y[j * b:(j + 1) * b]
        labels[j, :len(own)] = own
    return labels


# ---- one gradient call ------------------------------------------------------------------------------------------------------------------
def check_plan(blob, info):
    """The trainer's batch and LDS bytes are the restated plan's (ftrain_ref.train_batch: ftrain_size_lds and the lowering loop)."""
    p = fnet_plan.plan(blob)
    assert info["batch"] == ftrain_ref.train_batch(p) and info["lds_bytes"] == ftrain_ref.train_lds_bytes(p, info["batch"]), (info, p["batch"])
    return p


def check_gradient(name, tr, model, real, x, y, ref, n_total=None):
    """Every tensor of the gradient within ftrain_ref.bounds of the float64 reference, the padding +0.0f."""
    got = tr.gradients()
    packed = tr.gradient()
    assert not packed[~real].view(np.uint32).any(), "%s: a padding entry of the gradient is not +0.0f" % name
    per = ftrain_ref.bounds(model, x, y, ref, n_total)[0]
    for i, (g, g64, allowed) in enumerate(zip(got, ref["grads"], per)):
        for k in ("w", "b"):
            bound, e32 = allowed[k]
            err = ftrain_ref.tensor_error(g[k], g64[k])
            line = "%s n=%d record %d %s: gpu %.3g  e32 %.3g  bound %.3g" % (name, len(y), i, k, err, e32, bound)
            print(line)
            assert err <= bound, line


def check_call(ctx, tr, name, model, real, x, y, w0):
    """One host-form gradient call held in every way: logits and argmax edison_fnet_batch's bits, loss and every tensor by the float64
    bounds, padding +0.0f, a repeat the same bits, nothing else moved. Returns the packed gradient."""
    n = len(y)
    ref = ftrain_ref.loss_grad(model, x, y)
    before = ctx.fnet(x)
    r = tr.grad(x, y)
    assert same_bits(tr.logits(n), before["logits"]), (name, n)
    assert np.array_equal(r["argmax"], before["argmax"])
    lb, le = ftrain_ref.bounds(model, x, y, ref)[1]
    lerr = ftrain_ref.tensor_error(r["loss"], ref["loss"])
    print("%s n=%d loss: gpu %.3g  e32 %.3g  bound %.3g" % (name, n, lerr, le, lb))
    assert lerr <= lb, (name, n, lerr, lb)
    check_gradient(name, tr, model, real, x, y, ref)
    g = tr.gradient()
    r2 = tr.grad(x, y)
    assert same_bits(tr.gradient(), g), (name, n)
    assert same_bits(r2["loss"], r["loss"]) and same_bits(tr.logits(n), before["logits"])
    assert same_bits(tr.packed_weights(), w0)
    after = ctx.fnet(x)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    return g


def check_fold(ctx, tr, name, model, real, per_wg):
    """A call of N rows, the smallest power of two >= per_wg x grid x batch, held as every call is; then each of its tiles alone among
    fillers labelled -1 in a device-form call of n' rows on the same trainer: the big call's gradient is ftrain_ref.fold_tiles of
    those terms times n' / N, element for element (the argument is tests/test_gpu_ftrain_tiles.py's docstring)."""
    import torch
    info = tr.info()
    b, G, w = info["batch"], info["grid"], info["w_floats"]
    N = pow2_at_least(per_wg * G * b)
    n1 = pow2_at_least(b)                                               # rows of a small call: tile j's, then fillers
    n_tiles = (N + b - 1) // b
    assert n_tiles >= per_wg * G and n1 <= G * b and N >= 2 * n1
    x, y = rows(name, model, N + n1, exact=True)                        # n1 more finite rows behind the last tile: its fillers
    assert np.isfinite(x).all()
    w0 = tr.packed_weights()
    big = check_call(ctx, tr, name, model, real, x[:N], y[:N], w0)
    labels = tile_labels(y[:N], b, n1)
    fillers = int((labels < 0).sum())
    dev = torch.device("cuda", 0)
    xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev)
    torch.cuda.synchronize()                                            # the context's own stream takes them from here
    ignored0 = tr.info()["ignored"]
    T = np.empty((n_tiles, w), np.float32)
    smallest, digests = np.inf, set()
    for j in range(n_tiles):
        tr.grad_t(xt[j * b:j * b + n1], yt[j], n1)
        T[j] = tr.gradient()
        nz = np.abs(T[j][T[j] != 0])
        smallest = min(smallest, float(nz.min()) if nz.size else np.inf)
        digests.add(hashlib.blake2b(T[j].tobytes(), digest_size=16).digest())
        if j == 0:
            assert tr.info()["ignored"] - ignored0 == n1 - b
    assert tr.info()["ignored"] - ignored0 == fillers == n_tiles * n1 - N
    scale = n1 / N
    print("%s: batch %d, grid %d, N %d, %d tiles, small calls of %d rows, smallest term %.3g x %g" % (name, b, G, N, n_tiles, n1, smallest, scale))
    assert len(digests) == n_tiles, "two tiles give the same gradient: a swapped order would not show"
    assert np.isfinite(T).all() and smallest * scale > 2.0 ** -100
    assert not T[:, ~real].view(np.uint32).any()
    want = ftrain_ref.fold_tiles(T, G, scale)
    diff = np.flatnonzero(~(want == big))
    assert diff.size == 0, "%s: %d of %d gradient entries are not the fold of the tiles' (first at %d: call %r, fold %r)" % (
        name, diff.size, w, diff[0], big[diff[0]], want[diff[0]])
    assert not big[~real].view(np.uint32).any()
    assert same_bits(tr.packed_weights(), w0)


def sgd_step_checked(tr, real, x, y, lr):
    """step_checked for plain SGD; and the step as a whole within 2 x 2^-24 of the largest weight."""
    s = step_checked(tr, real, x, y, [None], lr, "sgd")
    assert np.abs(s.got[real] - (s.before.astype(np.float64) - lr * s.g)[real]).max() <= 2 * EPS * np.abs(s.before[real]).max()


def fnet_logits_of(c, blob, x):
    c.fnet_load(blob)
    return c.fnet(x)["logits"]


def fnet_logits_of_weights(c, tr, x):
    """The logits a trainer's own forward half gives on its weights now."""
    tr.grad(x, np.zeros(len(x), np.int32))
    return tr.logits(len(x))


# ---- one step -------------------------------------------------------------------------------------------------------------------------
def tensors(layout):
    """(lo, hi) of every tensor of the packed array: a record's w, then its b."""
    for r in layout:
        nb = r["k_pad"] * r["n_pad"]
        yield r["w_at"], r["w_at"] + nb
        yield r["w_at"] + nb, r["w_at"] + nb + r["n_pad"]


def step_errors(layout, real, got, want):
    """Per element of the packed array |got - want| / max |want| over the element's tensor (a record's w or its b), real entries
    only; 0 at the padding."""
    err = np.zeros(len(got))
    for lo, hi in tensors(layout):
        m = real[lo:hi]
        err[lo:hi][m] = np.abs(got[lo:hi][m] - want[lo:hi][m]) / np.abs(want[lo:hi][m]).max()
    return err


def step_checked(tr, real, x, y, replays, lr, what, bound=4 * EPS):
    """One gradient call and one step; every replay in `replays` (ftrain_ref.Adam, ftrain_ref.Adadelta, or None for SGD) takes the step
    in float64 from the weights the GPU stepped from with the GPU's own gradient, its moments running on in float64. The first replay
    is the statement of what the GPU does: every tensor within `bound` of it by step_errors; and the padding is still 1e6 (zero
    gradient, zero moments). Returns before (float32), g (float64), got, and errs, step_errors' array of every replay."""
    before = tr.packed_weights()
    tr.grad(x, y)
    g = tr.gradient().astype(np.float64)
    tr.step(lr)
    got = tr.packed_weights()
    errs = []
    for opt in replays:
        want = [before.astype(np.float64)]
        if opt is None:
            want[0] -= lr * g
        else:
            opt.step(want, [g], lr)
        errs.append(step_errors(tr.layout, real, got, want[0]))
    for lo, hi in tensors(tr.layout):
        err = errs[0][lo:hi].max()
        print("%s tensor at %d: %.3g (bound %.3g)" % (what, lo, err, bound))
        assert err <= bound, (what, lo, err)
    assert (got[~real] == POISON).all()
    return types.SimpleNamespace(before=before, g=g, got=got, errs=errs)


# ---- fit ------------------------------------------------------------------------------------------------------------------------------
def fit_kw():
    return dict(epochs=100, batch_size=ftrain_rows.FIT_BATCH, seed=0, lr=ftrain_rows.FIT_LR, max_steps=ftrain_rows.FIT_STEPS)


def check_fit_learns(ctx, tr_kwargs, model, blob, x, y):
    """40 Adam steps by fit_kw on (x, y): the train loss falls below half its first value, the accuracy reaches 0.9, and the last loss
    is the float64 replay's to 1e-3."""
    ctx.fnet_load(blob)
    with ctx.trainer(**tr_kwargs) as tr:
        hist = tr.fit(x, y, **fit_kw())
        assert hist["steps"] == 40 and tr.info()["steps"] == 40
        acc = (ctx.fnet(x)["argmax"] == y).mean()
    replay = train.fit(ftrain_ref.HostTrainer(model), x, y, **fit_kw())
    print("loss %.5f -> %.5f (float64 replay %.5f), accuracy %.3f" % (hist["loss"][0], hist["loss"][-1], replay["loss"][-1], acc))
    assert hist["loss"][-1] < 0.5 * hist["loss"][0] and acc >= 0.9
    assert abs(hist["loss"][-1] - replay["loss"][-1]) <= 1e-3 * replay["loss"][-1]
    assert len(hist["loss"]) == len(replay["loss"]) == 14


def follows_replay(hist, replay):
    """The loss and validation loss of every epoch are the float64 replay's to 1e-3."""
    assert len(hist["loss"]) == len(replay["loss"])
    for k in ("loss", "val_loss"):
        for got, want in zip(hist[k], replay[k]):
            assert abs(got - want) <= 1e-3 * want, (hist[k], replay[k])


# ---- kws train, then kws quantize -------------------------------------------------------------------------------------------------------
def kws_files(tmp_path, model, x, y, keywords):
    """Writes net.ednf, x.npy and y.npy -> (kws_train.run's three path arguments, the val pair: the training set again)."""
    with open(tmp_path / "net.ednf", "wb") as f:
        f.write(cube_import.build_blob(model, keywords))
    np.save(tmp_path / "x.npy", x)
    np.save(tmp_path / "y.npy", y)
    args = [str(tmp_path / "net.ednf"), str(tmp_path / "x.npy"), str(tmp_path / "y.npy")]
    return args, (args[1], args[2])


def kws_trained(ctx, tmp_path, args, val, epochs=5, **kw):
    """kws train on kws_files' set of 96 rows at batch 32, lr 0.01, into out.ednf, and what every such run leaves: the file is the
    returned blob, three steps and one validation entry per epoch, the closing line. Returns (blob, history, printed text, trained model)."""
    from edison_amd.kws import kws_train
    out = io.StringIO()
    blob, hist = kws_train.run(*args, str(tmp_path / "out.ednf"), epochs=epochs, batch=32, lr=0.01, val=val, ctx=ctx, out=out, **kw)
    assert (tmp_path / "out.ednf").read_bytes() == blob and hist["steps"] == 3 * epochs and len(hist["val_loss"]) == epochs
    assert "after %d steps" % (3 * epochs) in out.getvalue()
    return blob, hist, out.getvalue(), cube_import.read_blob(blob)


def kws_audio(n_samples, n=6, seed=8):
    return np.clip(np.random.default_rng(seed).normal(0, 3000, (n, n_samples)), -32768, 32767).astype(np.int16)


def kws_quantized(ctx, tmp_path, audio=None, **kw):
    """kws quantize of out.ednf on six recordings (kws_audio at the configured geometry's length unless given): q.ednn is the
    returned blob, one float class per recording."""
    from edison_amd import config as cfg
    from edison_amd.kws import kws_quantize
    from edison_amd.kws.geometry import KwsGeometry
    if audio is None:
        audio = kws_audio(KwsGeometry.from_config(net_input_scale=cfg.net_input_scale).n_samples)
    np.save(tmp_path / "audio.npy", audio)
    qblob, rep = kws_quantize.run(str(tmp_path / "out.ednf"), str(tmp_path / "audio.npy"), str(tmp_path / "q.ednn"), ctx=ctx, out=io.StringIO(), **kw)
    assert (tmp_path / "q.ednn").read_bytes() == qblob and len(rep["float_argmax"]) == len(audio) == 6

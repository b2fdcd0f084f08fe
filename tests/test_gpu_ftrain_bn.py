"""GPU tests (-m gpu) of BatchNorm in the float32 trainer (edison_ftrain_set_batchnorm, Trainer.set_batchnorm, kws train --batchnorm;
DESIGN.md section 19c) against tests/ftrain_ref.py: on two consecutive training calls the loss, the logits and every gradient tensor (w,
b of records without BatchNorm, dgamma, dbeta) against the float64 restatement by section 19's metric and bound -- per tensor
max |g - g64| / max |g64|, allowed 4 x the same error of torch's CPU float32 autograd on the same call, floored at
8 x 2^-24 x sqrt(terms), terms counting N -- the +0.0f bias gradient of BatchNorm records and of all padding, repeatability, the batch
and the moving statistics, row counts around the tile and beyond the grid, the fold and the eval call bit for bit, Adam steps, the
refusals, fit and the CLI. tests/test_fbn_cpu.py shows the bound's precondition on the very inputs used here. Every network is loaded
with 1e6 in all its weight padding (ftrain_drive.poisoned)."""
import ctypes
import io

import numpy as np
import pytest

import fnet_host
import fnet_rows
import ftrain_ref
import ftrain_rows
from edison_amd import _lib, cube_import, train
from ftrain_drive import (EPS, POISON, case, check_gradient, data, fit_kw, follows_replay, kws_files, kws_quantized, kws_trained, loaded, own_context, poisoned,
                          same_bits)
from ftrain_rows import bn_case

pytestmark = pytest.mark.gpu

ULP4 = 4 * EPS


@pytest.fixture(scope="module")
def ctx(built_lib):
    yield from own_context()


@pytest.fixture(scope="module")
def fresh(built_lib):
    yield from own_context()


def trainer_of(ctx, name, **kw):
    """A trainer on the loaded row `name` with its BatchNorm records, its dropout and, where the row sets gamma and beta, its state."""
    c = bn_case(name)
    tr = ctx.trainer()
    tr.set_batchnorm(c["bn"], **kw)
    if c["dropout"] is not None:
        tr.set_dropout(c["dropout"], seed=c["seed"])
    if ftrain_rows.BN_ROWS[name].get("neg"):
        tr.set_bn_state(c["state0"])
    return tr


def last_error(ctx):
    return (ctx._L.edison_last_error(ctx._h) or b"").decode()


def within(got, want, what):
    """4 x 2^-24 of the tensor's maximum."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print("%s: %.3g of its maximum (allowed %.3g)" % (what, err / scale if scale else err, ULP4))
    assert err <= ULP4 * scale, (what, err, scale)


def check_bn_call(name, call, tr, r, real, ref, bounds):
    """One training call's loss, logits, gradients and their padding against the restatement. Returns the bits to repeat."""
    per, (lb, le), (zb, ze) = bounds
    z = tr.logits(len(r["loss"]))
    for what, got, want, bound, e32 in (("loss", r["loss"], ref["loss"], lb, le), ("logits", z, ref["logits"], zb, ze)):
        err = ftrain_ref.tensor_error(got, want)
        line = "%s call %d %s: gpu %.3g  e32 %.3g  bound %.3g" % (name, call, what, err, e32, bound)
        print(line)
        assert err <= bound, line
    assert np.array_equal(r["argmax"], np.argmax(z, axis=1))
    packed = tr.gradient()
    assert not packed[~real].view(np.uint32).any(), "%s: a padding entry of the gradient is not +0.0f" % name
    bng = tr.bn_gradients()
    for i, (g, g64, b64, rec) in enumerate(zip(tr.gradients(), ref["grads"], ref["bn"], per)):
        checks = [("w", g["w"], g64["w"])]
        if b64 is None:
            assert bng[i] is None
            checks.append(("b", g["b"], g64["b"]))
        else:
            assert not g["b"].view(np.uint32).any(), "%s record %d: the bias gradient of a BatchNorm record is not +0.0f" % (name, i)
            checks += [("gamma", bng[i]["gamma"], b64["gamma"]), ("beta", bng[i]["beta"], b64["beta"])]
        for k, got, want in checks:
            err = ftrain_ref.tensor_error(got, want)
            line = "%s call %d record %d %s: gpu %.3g  e32 %.3g  bound %.3g" % (name, call, i, k, err, rec[k][1], rec[k][0])
            print(line)
            assert err <= rec[k][0], line
    return r["loss"], z, packed, bng


def check_stats(name, call, tr, ref, after):
    batch, state = tr.bn_batch_stats(), tr.bn_state()
    for i, b64 in enumerate(ref["bn"]):
        if b64 is None:
            assert batch[i] is None and state[i] is None
            continue
        for k in ("mean", "var"):
            within(batch[i][k], b64[k], "%s call %d record %d batch %s" % (name, call, i, k))
            within(state[i][k], after[i][k], "%s call %d record %d moving %s" % (name, call, i, k))


@pytest.mark.parametrize("name", ftrain_rows.BN_ROWS)
def test_two_training_calls_against_the_restatement(ctx, name):
    c, real = loaded(ctx, bn_case(name))
    x, y = c["x"], c["y"]
    with trainer_of(ctx, name) as tr:
        bn = tr.batchnorm()
        assert bn["on"] and bn["has_bn"] == c["bn"] and bn["momentum"] == 0.99 and bn["eps"] == 1e-3 and bn["max_rows"] == 1024 and not bn["unbiased"]
        assert 1 <= bn["batch"] <= tr.info()["batch"]
        if name == "shipped":
            assert bn["batch"] == 7 and len(y) == 9                             # two tiles
        elif name != "bn_dense":
            assert bn["batch"] < len(y)
        w0 = tr.packed_weights()
        kept = {}
        for call in (0, 1):
            ref, after = ftrain_rows.bn_reference(name, call)
            kept[call] = check_bn_call(name, call, tr, tr.grad(x, y), real, ref, ftrain_rows.bn_bounds(name, call))
        if c["dropout"] is not None:
            assert tr.dropout_call == 2 and not same_bits(kept[0][1], kept[1][1])    # another mask
            tr.dropout_call = 1
        # the same call again: the same bits (the moving statistics move, nothing else reads them)
        r = tr.grad(x, y)
        assert same_bits(r["loss"], kept[1][0]) and same_bits(tr.logits(len(y)), kept[1][1]) and same_bits(tr.gradient(), kept[1][2])
        for a, b in zip(tr.bn_gradients(), kept[1][3]):
            assert (a is None and b is None) or (same_bits(a["gamma"], b["gamma"]) and same_bits(a["beta"], b["beta"]))
        assert same_bits(tr.packed_weights(), w0)                              # a gradient call moves no weight


@pytest.mark.parametrize("name", ftrain_rows.BN_ROWS)
def test_batch_and_moving_statistics_of_two_training_calls(ctx, name):
    """Batch mean / variance and the moving statistics after each of the two calls, within 4 x 2^-24 of the tensor's maximum of the
    float64 restatement's. The shipped row's deepest BatchNorm record is the hard one: its z has come through three convolutions and
    three normalisations and N is only 27. With one float32 MFMA chain over the whole of K its batch variance was 5.07e-07 of its
    maximum away; with the chains of 16 k that edb_conv_tile sums in double it is 1.11e-07 (allowed 2.38e-07)."""
    c, _ = loaded(ctx, bn_case(name))
    with trainer_of(ctx, name) as tr:
        for call in (0, 1):
            ref, after = ftrain_rows.bn_reference(name, call)
            tr.grad(c["x"], c["y"])
            check_stats(name, call, tr, ref, after)


@pytest.mark.parametrize("name", ["bn_p1", "bn_trunc"])
def test_the_unbiased_flag_moves_the_variance_by_torchs_rule(ctx, name):
    c, _ = loaded(ctx, bn_case(name))
    with trainer_of(ctx, name, unbiased=True, momentum=0.9) as tr:
        assert tr.batchnorm()["unbiased"] and tr.batchnorm()["momentum"] == 0.9
        state = c["state0"]
        for call in (0, 1):
            ref, _ = ftrain_rows.bn_reference(name, call)                                  # the weights do not move: the batch statistics are the same
            tr.grad(c["x"], c["y"])
            state = ftrain_ref.moved(state, ref["bn"], momentum=0.9, unbiased=True)
        biased = ftrain_ref.moved(ftrain_ref.moved(c["state0"], ref["bn"], momentum=0.9), ref["bn"], momentum=0.9)
        for i, st in enumerate(tr.bn_state()):
            if st is None:
                continue
            within(st["var"], state[i]["var"], "%s record %d moving var, unbiased" % (name, i))
            within(st["mean"], state[i]["mean"], "%s record %d moving mean" % (name, i))
            assert np.abs(state[i]["var"] - biased[i]["var"]).max() > 100 * ULP4 * np.abs(state[i]["var"]).max()     # the flag is visible


def drawn(c, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (n, c["x"].shape[1])).astype(np.float32)
    n_out = int(np.prod(fnet_host.conv_records(c["model"])[-1]["out"]))
    return x, (np.arange(n) % n_out).astype(np.int32)


def check_rows(ctx, name, tr, c, real, x, y):
    """A call of other rows than the case's: reference, bound and precondition computed here."""
    model, n = c["model"], len(y)
    bn = dict(state=c["state0"])
    ref = ftrain_ref.loss_grad(model, x, y, bn=bn, detail=True)
    r32 = ftrain_ref.loss_grad(model, x, y, bn=bn, dtype=np.float32, detail=True)
    for L, d32, d64 in zip(fnet_host.conv_records(model), r32["detail"], ref["detail"]):       # the bound's precondition on these rows
        assert np.array_equal(d32["first"], d64["first"]) and (not L["relu"] or np.array_equal(d32["y"] > 0, d64["y"] > 0))
    per = ftrain_ref.bounds(model, x, y, ref, bn=bn)[0]
    tr.grad(x, y)
    packed = tr.gradient()
    assert not packed[~real].view(np.uint32).any()
    bng = tr.bn_gradients()
    for i, (g, g64, b64) in enumerate(zip(tr.gradients(), ref["grads"], ref["bn"])):
        checks = [("w", g["w"], g64["w"])]
        if b64 is None:
            checks.append(("b", g["b"], g64["b"]))
        else:
            assert not g["b"].view(np.uint32).any()
            checks += [(k, bng[i][k], b64[k]) for k in ("gamma", "beta")]
            bs = tr.bn_batch_stats()[i]
            within(bs["mean"], b64["mean"], "%s n=%d record %d batch mean" % (name, n, i))
            within(bs["var"], b64["var"], "%s n=%d record %d batch var" % (name, n, i))
        for k, got, want in checks:
            err, (bound, e32) = ftrain_ref.tensor_error(got, want), per[i][k]
            line = "%s n=%d record %d %s: gpu %.3g  e32 %.3g  bound %.3g" % (name, n, i, k, err, e32, bound)
            print(line)
            assert err <= bound, line
    return packed


@pytest.mark.parametrize("name", ["bn_p1", "bn_trunc"])
def test_row_counts_around_the_tile(ctx, name):
    c, real = loaded(ctx, bn_case(name))
    with ctx.trainer() as probe:
        probe.set_batchnorm(c["bn"])
        b = probe.batchnorm()["batch"]
    assert b >= 3
    for n in (2, b - 1, b, b + 1, 3 * b + 2):
        loaded(ctx, bn_case(name))                                              # a fresh load: a BatchNorm trainer folds into the loaded network
        with ctx.trainer(batchnorm=c["bn"]) as tr:
            x, y = drawn(c, n, 900 + n)
            check_rows(ctx, name, tr, c, real, x, y)


def test_more_tiles_than_workgroups_and_the_cap(ctx):
    c, real = loaded(ctx, bn_case("bn_p1"))
    with ctx.trainer() as probe:
        probe.set_batchnorm(c["bn"])
        b, grid = probe.batchnorm()["batch"], probe.info()["grid"]
    cap = 2 * grid * b + b + 1
    loaded(ctx, bn_case("bn_p1"))
    with ctx.trainer(batchnorm=dict(has_bn=c["bn"], max_rows=cap)) as tr:
        assert tr.batchnorm()["max_rows"] == cap
        x, y = drawn(c, cap, 77)
        first = check_rows(ctx, "bn_p1", tr, c, real, x, y)
        tr.grad(x, y)
        assert same_bits(tr.gradient(), first)
        x1, y1 = drawn(c, cap + 1, 78)
        with pytest.raises(_lib.EdisonError) as e:
            tr.grad(x1, y1)
        assert e.value.code == _lib.E_ARGUMENT and str(cap) in str(e.value) and "max_rows" in str(e.value)
        assert same_bits(tr.gradient(), first)                                 # the refused call left the gradient


def random_state(c, seed):
    rng = np.random.default_rng(seed)
    return [None if st is None else dict(gamma=rng.normal(0, 1, len(st["gamma"])).astype(np.float32), beta=rng.normal(0, 1, len(st["gamma"])).astype(np.float32),
                                         mean=rng.normal(0, 1, len(st["gamma"])).astype(np.float32), var=rng.uniform(0.2, 3, len(st["gamma"])).astype(np.float32))
            for st in c["state0"]]


@pytest.mark.parametrize("name", ["bn_pool21_neg", "bn_mixed"])
def test_the_fold_and_the_eval_call(ctx, fresh, name):
    c, real = loaded(ctx, bn_case(name))
    x, y = c["x"], c["y"]
    with trainer_of(ctx, name) as tr:
        state = random_state(c, 5)
        tr.set_bn_state(state)
        got = tr.bn_state()
        for a, b in zip(got, state):
            assert (a is None and b is None) or all(same_bits(a[k], b[k]) for k in a)
        z = ctx.fnet(x)["logits"]
        fresh.fnet_load(cube_import.build_blob(tr.model()))
        assert same_bits(z, fresh.fnet(x)["logits"])                           # the context runs the folded network
        want = ftrain_ref.fold(tr.weights(), state)
        for i, (g, w64) in enumerate(zip(tr.folded_weights(), want)):
            within(g["w"], w64["w"], "%s record %d folded w" % (name, i))
            within(g["b"], w64["b"], "%s record %d folded b" % (name, i))
        # an eval call: the folded network's logits, no statistic moved, and no gradient to fetch or step
        r = tr.grad(x, y, training=False)
        assert same_bits(tr.logits(len(y)), z) and np.array_equal(r["argmax"], ctx.fnet(x)["argmax"])
        for a, b in zip(tr.bn_state(), state):
            assert (a is None and b is None) or all(same_bits(a[k], b[k]) for k in a)
        w0 = tr.packed_weights()
        for call in (tr.gradient, tr.step, tr.bn_gradients):
            with pytest.raises(_lib.EdisonError) as e:
                call()
            assert e.value.code == _lib.E_ARGUMENT and "EVAL" in str(e.value)
        assert same_bits(tr.packed_weights(), w0) and tr.info()["steps"] == 0
        tr.grad(x, y)                                                          # a training call: there is a gradient again
        assert np.isfinite(tr.gradient()).all()
        tr.step(0.01)
        assert tr.info()["steps"] == 1 and not same_bits(tr.packed_weights(), w0)
        # set_weights writes the master weights and refolds
        tr.set_packed_weights(w0)
        fresh.fnet_load(cube_import.build_blob(tr.model()))
        assert same_bits(ctx.fnet(x)["logits"], fresh.fnet(x)["logits"])


@pytest.mark.parametrize("name", ["bn_mixed", "shipped"])
def test_three_adam_steps_follow_the_host_trainer_on_the_gpus_gradients(ctx, fresh, name):
    c, real = loaded(ctx, bn_case(name))
    x, y = c["x"], c["y"]
    host = ftrain_ref.HostTrainer(c["model"], c["dropout"], seed=c["seed"], has_bn=c["bn"])
    with trainer_of(ctx, name) as tr:
        for step in range(3):
            tr.grad(x, y)
            host._g = [dict(w=g["w"], b=g["b"]) for g in tr.gradients()]
            host._gbn = tr.bn_gradients()
            host.step(0.01)
            tr.step(0.01)
            state = tr.bn_state()
            for i, (g, h) in enumerate(zip(tr.weights(), host.weights)):
                within(g["w"], h["w"], "%s step %d record %d w" % (name, step, i))
                within(g["b"], h["b"], "%s step %d record %d b" % (name, step, i))
                if state[i] is not None:
                    within(state[i]["gamma"], host.state[i]["gamma"], "%s step %d record %d gamma" % (name, step, i))
                    within(state[i]["beta"], host.state[i]["beta"], "%s step %d record %d beta" % (name, step, i))
        assert tr.info()["steps"] == 3
        # the master array's padding is the blob's poison, untouched
        assert same_bits(tr.packed_weights()[~real], np.full(int((~real).sum()), POISON))
        fresh.fnet_load(cube_import.build_blob(tr.model()))
        assert same_bits(ctx.fnet(x)["logits"], fresh.fnet(x)["logits"])       # the context runs the refolded network
        # reset zeroes the moments of gamma and beta too, and leaves the moving statistics
        before = tr.bn_state()
        tr.reset()
        assert tr.info()["steps"] == 0
        for a, b in zip(tr.bn_state(), before):
            assert (a is None and b is None) or all(same_bits(a[k], b[k]) for k in a)


def test_refusals(ctx):
    L = ctx._L
    c, _ = loaded(ctx, bn_case("bn_p1"))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def code(tr, has_bn, n=None, momentum=0.99, eps=1e-3, rows=0, flags=0):
        hb = np.asarray(has_bn, np.uint8)
        return L.edison_ftrain_set_batchnorm(tr._h, ptr(hb), len(hb) if n is None else n, momentum, eps, rows, flags)

    with ctx.trainer() as tr:
        assert not tr.batchnorm()["on"]
        assert code(tr, [1, 1]) == _lib.E_ARGUMENT and "logits" in last_error(ctx)            # BatchNorm on the last record
        assert code(tr, [1, 0], n=1) == _lib.E_ARGUMENT and code(tr, [1, 0, 0]) == _lib.E_ARGUMENT
        for m in (1.0, -0.1, float("nan"), 1.5):
            assert code(tr, [1, 0], momentum=m) == _lib.E_ARGUMENT and "momentum" in last_error(ctx)
        for e in (0.0, -1e-3, float("nan"), float("inf")):
            assert code(tr, [1, 0], eps=e) == _lib.E_ARGUMENT and "eps" in last_error(ctx)
        assert code(tr, [1, 0], flags=2) == _lib.E_ARGUMENT
        assert not tr.batchnorm()["on"]
        g = np.zeros(5, np.float32)
        assert L.edison_ftrain_bn_get(tr._h, 0, ptr(g), None, None, None) == _lib.E_ARGUMENT   # BatchNorm is not on
        tr.set_batchnorm([1, 0], max_rows=20, unbiased=True)
        assert code(tr, [1, 0]) == _lib.E_ARGUMENT and "new trainer" in last_error(ctx)       # a second set_batchnorm
        assert L.edison_ftrain_bn_get(tr._h, 1, ptr(g), None, None, None) == _lib.E_ARGUMENT   # a record without BatchNorm
        assert L.edison_ftrain_bn_get(tr._h, 2, ptr(g), None, None, None) == _lib.E_ARGUMENT
        assert L.edison_ftrain_bn_grad_get(tr._h, 1, ptr(g), None) == _lib.E_ARGUMENT
        before = tr.bn_state()
        bad = np.full(5, -1e-3, np.float32)
        assert L.edison_ftrain_bn_set(tr._h, 0, None, None, None, ptr(bad)) == _lib.E_ARGUMENT and "variance" in last_error(ctx)
        bad = np.full(5, np.nan, np.float32)
        assert L.edison_ftrain_bn_set(tr._h, 0, ptr(bad), None, None, None) == _lib.E_ARGUMENT
        assert all(same_bits(tr.bn_state()[0][k], before[0][k]) for k in before[0])
        x, y = drawn(c, 21, 3)
        with pytest.raises(_lib.EdisonError) as e:
            tr.grad(x, y)
        assert e.value.code == _lib.E_ARGUMENT and "max_rows = 20" in str(e.value)
        tr.grad(x[:20], y[:20])
        tr.grad(x, y, training=False)                                           # an eval call is not capped
    cd, _ = loaded(ctx, bn_case("bn_dense"))
    with ctx.trainer(batchnorm=dict(has_bn=cd["bn"], unbiased=True)) as tr:
        with pytest.raises(_lib.EdisonError) as e:
            tr.grad(cd["x"][:1], cd["y"][:1])                                  # N = 1 with the unbiased flag
        assert e.value.code == _lib.E_ARGUMENT and "N < 2" in str(e.value)
        tr.grad(cd["x"], cd["y"])
    # a list that marks no record still turns the BatchNorm trainer on: master weights, the fold, once per trainer
    loaded(ctx, bn_case("bn_p1"))
    with ctx.trainer(batchnorm=[0, 0]) as tr:
        assert tr.batchnorm()["on"] and tr.batchnorm()["has_bn"] == [0, 0] and tr.bn_state() == [None, None]
        assert code(tr, [1, 0]) == _lib.E_ARGUMENT and "new trainer" in last_error(ctx)
    # a network with a pad
    ctx.fnet_load(ftrain_rows.pad_blob(ftrain_rows.PAD_FIT_ROW))
    with ctx.trainer(padded=True) as tr:
        nl = tr.n_layers
        with pytest.raises(_lib.EdisonError) as e:
            tr.set_batchnorm([1] + [0] * (nl - 1))
        assert e.value.code == _lib.E_NO_IMPL and "record" in str(e.value) and "pad" in str(e.value)
        assert not tr.batchnorm()["on"]


def test_a_trainer_without_batchnorm_is_unchanged(ctx):
    name = "pool21_trunc_h"
    model, blob, real = case(name)
    x, y = data(name, model, 17)
    ctx.fnet_load(blob)
    bits = []
    for _ in range(2):
        with ctx.trainer() as tr:
            r = tr.grad(x, y)
            bits.append((r["loss"], tr.logits(17), tr.gradient()))
            assert not tr.batchnorm()["on"] and tr.bn_state() == [None, None]
    assert all(same_bits(a, b) for a, b in zip(*bits))
    assert same_bits(bits[0][1], ctx.fnet(x)["logits"])
    ref = ftrain_ref.loss_grad(model, x, y)
    with ctx.trainer() as tr:
        tr.grad(x, y)
        check_gradient(name, tr, model, real, x, y, ref)


def test_fit_with_batchnorm_and_dropout_follows_the_float64_replay(ctx):
    """Three noisy class patterns on pool21_trunc_h's shape, BatchNorm behind the conv and dropout 0.25 before its pool, 40 Adam steps
    at batch 32, lr 0.01: the loss history is the float64 HostTrainer replay's to 1e-3 per epoch and the accuracy 1.0; validation runs
    the folded network."""
    x, y = ftrain_rows.fit_set()
    model = fnet_rows.model(ftrain_rows.FIT_ROW)
    ctx.fnet_load(poisoned(fnet_rows.blob(ftrain_rows.FIT_ROW))[0])
    bn, dropout = [1, 0], [(0.25, 1), 0]
    kw = dict(fit_kw(), val=(x, y), callbacks=False)
    with ctx.trainer(dropout=dropout, seed=3, batchnorm=bn) as tr:
        hist = tr.fit(x, y, **kw)
        assert hist["steps"] == 40 and tr.info()["steps"] == 40 and tr.dropout_call == 40
        out = ctx.fnet(x)
        acc = (out["argmax"] == y).mean()
        r = tr.grad(x, y, training=False)
        assert hist["val_acc"][-1] == (r["argmax"] == y).mean() == acc
    host = ftrain_ref.HostTrainer(model, dropout, seed=3, has_bn=bn)
    replay = train.fit(host, x, y, **kw)
    print("loss %s\nreplay %s\nval %s\nreplay %s\naccuracy %.3f" % (np.round(hist["loss"], 5), np.round(replay["loss"], 5), np.round(hist["val_loss"], 5),
                                                                    np.round(replay["val_loss"], 5), acc))
    assert host.call == 40
    follows_replay(hist, replay)
    assert hist["loss"][-1] < 0.5 * hist["loss"][0]
    assert acc == 1.0


def test_kws_train_with_batchnorm_then_kws_quantize(ctx, tmp_path):
    """kws train --batchnorm-arch kws_conv --dropout-arch kws_conv on the shipped geometry with fresh weights, then kws quantize."""
    from edison_amd.kws import kws_train
    model = bn_case("shipped")["model"]
    x, y = ftrain_rows.kws_set()
    keywords = ["k%d" % i for i in range(10)]
    args, val = kws_files(tmp_path, model, x, y, keywords)
    blob, hist, _, trained = kws_trained(ctx, tmp_path, args, val, epochs=3, dropout_arch="kws_conv", batchnorm_arch="kws_conv")
    assert hist["loss"][-1] < hist["loss"][0]
    plain, _ = kws_train.run(*args, str(tmp_path / "plain.ednf"), epochs=3, batch=32, lr=0.01, val=val, ctx=ctx, out=io.StringIO(), dropout_arch="kws_conv")
    assert plain != blob and len(plain) == len(blob)                        # BatchNorm took part, and the format did not change
    assert kws_train.main(["train"] + args + [str(tmp_path / "cli.ednf"), "--epochs", "1", "--batch", "32", "--batchnorm-arch", "kws_conv",
                                              "--dropout-arch", "kws_conv", "--bn-momentum", "0.9"]) == 0
    assert trained["keywords"] == keywords
    kws_quantized(ctx, tmp_path)

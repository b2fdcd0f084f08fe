"""GPU tests (-m gpu) of dropout in the float32 trainer (edison_ftrain_set_dropout, Trainer.set_dropout, kws train --dropout; DESIGN.md
section 19b) against tests/fdrop_ref.py and tests/ftrain_ref.py: the logits bit for bit against the host model with the mask, the loss and every gradient
tensor against the float64 restatement with the mask by section 19's metric and bound -- per tensor max |g - g64| / max |g64|, allowed
4 x the same error of torch's CPU float32 autograd with the same mask, floored at 8 x 2^-24 x sqrt(terms) -- the counter, the eval flag,
the mask's independence of the tiling exactly, the refusals, fit and the CLI. tests/test_fdrop_cpu.py shows the bound's precondition
on the very inputs used here. Every network is loaded with 1e6 in all its weight padding (ftrain_drive.poisoned)."""
import ctypes
import io
import struct

import numpy as np
import pytest

import fdrop_ref as fd
import fnet_plan
import fnet_rows
import ftrain_ref
import ftrain_rows
from edison_amd import _lib, train
from ftrain_drive import fit_kw, follows_replay, kws_files, kws_quantized, kws_trained, loaded, own_context, poisoned, same_bits
from ftrain_rows import drop_case

pytestmark = pytest.mark.gpu

N = ftrain_rows.N_ROWS


@pytest.fixture(scope="module")
def ctx(built_lib):
    yield from own_context()


def plain_bits(ctx, c):
    """What a fresh trainer on which dropout was never set gives on the row: (loss, logits, gradient)."""
    with ctx.trainer(padded=True) as tr:
        r = tr.grad(c["x"], c["y"])
        return r["loss"], tr.logits(N), tr.gradient(), tr.info()


@pytest.mark.parametrize("name", ftrain_rows.DROP_ROWS)
def test_logits_loss_gradient_counter_eval_flag_and_zero_rates(ctx, name):
    c, real = loaded(ctx, drop_case(name))
    model, x, y = c["model"], c["x"], c["y"]
    loss0, z0, g0, info0 = plain_bits(ctx, c)
    with ctx.trainer(padded=True) as tr:
        shape = {k: tr.info()[k] for k in ("batch", "lds_bytes", "grid")}
        assert tr.dropout() == dict(rates=[0.0] * tr.n_layers, before_pool=[0] * tr.n_layers, seed=0, call=0, on=False)
        tr.set_dropout(c["dropout"], seed=c["seed"])
        d = tr.dropout()
        want_r, want_b = train.dropout_spec(c["dropout"])
        assert d["rates"] == want_r and d["before_pool"] == want_b and d["seed"] == c["seed"] and d["call"] == 0 and d["on"]
        assert {k: tr.info()[k] for k in shape} == shape == {k: info0[k] for k in shape}      # the LDS plan does not know about dropout
        assert shape["batch"] < N                                                              # more than one tile
        w0 = tr.packed_weights()
        first = {}
        for call in (0, 1):
            assert tr.dropout_call == call
            r = tr.grad(x, y)
            assert tr.dropout_call == call + 1                                                 # one training call, one step of the counter
            want = fd.forward32(model, x, c["sp"], c["seed"], call)[-1]
            z = tr.logits(N)
            assert same_bits(z, want), "%s call %d: %d of %d logits differ from the host model with the mask" % (
                name, call, int((z.view(np.uint32) != want.view(np.uint32)).sum()), z.size)
            ref = ftrain_rows.drop_reference(name, call)
            assert np.array_equal(r["argmax"], np.argmax(want, axis=1))
            per, (lb, le), _ = ftrain_ref.bounds(model, x, y, ref, dropout=(c["sp"], c["seed"], call))
            lerr = ftrain_ref.tensor_error(r["loss"], ref["loss"])
            print("%s call %d loss: gpu %.3g  e32 %.3g  bound %.3g" % (name, call, lerr, le, lb))
            assert lerr <= lb, (name, call, lerr, lb)
            packed = tr.gradient()
            assert not packed[~real].view(np.uint32).any(), "%s: a padding entry of the gradient is not +0.0f" % name
            for i, (g, g64, allowed) in enumerate(zip(tr.gradients(), ref["grads"], per)):
                for k in ("w", "b"):
                    bound, e32 = allowed[k]
                    err = ftrain_ref.tensor_error(g[k], g64[k])
                    line = "%s call %d record %d %s: gpu %.3g  e32 %.3g  bound %.3g" % (name, call, i, k, err, e32, bound)
                    print(line)
                    assert err <= bound, line
            first[call] = (r["loss"], z, packed)
        assert not np.array_equal(first[0][1], first[1][1])                                    # the next counter value: another mask
        assert not same_bits(first[0][1], z0)                                                  # and neither is the network without dropout
        # the counter set back: the same call, the same bits
        tr.dropout_call = 0
        r = tr.grad(x, y)
        assert same_bits(r["loss"], first[0][0]) and same_bits(tr.logits(N), first[0][1]) and same_bits(tr.gradient(), first[0][2])
        assert tr.dropout_call == 1
        # the eval flag: a trainer without dropout, bit for bit, and the counter stays
        r = tr.grad(x, y, training=False)
        assert same_bits(r["loss"], loss0) and same_bits(tr.logits(N), z0) and same_bits(tr.gradient(), g0)
        assert tr.dropout_call == 1
        assert same_bits(z0, ctx.fnet(x)["logits"])
        # reset puts the counter back
        tr.reset()
        assert tr.dropout_call == 0 and tr.dropout()["on"]
        # all rates zero: off, those bits too
        tr.set_dropout([0] * tr.n_layers, seed=c["seed"])
        assert not tr.dropout()["on"]
        r = tr.grad(x, y)
        assert same_bits(r["loss"], loss0) and same_bits(tr.logits(N), z0) and same_bits(tr.gradient(), g0)
        assert tr.dropout_call == 0
        assert same_bits(tr.packed_weights(), w0)                                              # nothing moved the weights
        assert {k: tr.info()[k] for k in shape} == shape


def test_mid_pads_batch_runs_both_tile_instantiations_in_two_to_four_tiles(ctx):
    c, _ = loaded(ctx, drop_case("mid_pads_batch"))
    p = fnet_plan.plan(c["blob"])
    with ctx.trainer(padded=True, dropout=c["dropout"], seed=c["seed"]) as tr:
        b = tr.info()["batch"]
        assert [L["pad"] for L in p["layers"]] == [False, True, True, False] and 2 <= -(-N // b) <= 4
        assert tr.dropout()["on"] and tr.dropout()["seed"] == c["seed"]


def test_the_mask_does_not_depend_on_the_tiling_exactly(ctx):
    """batch5 at its training batch 2, N = 1024 rows in device form: 512 tiles on at most 256 workgroups. The full call against the
    fold of 512 calls of the same 1024 rows at the same counter, call j with only tile j's rows labelled (every other row -1: the
    ordinals and n are the same, the other tiles contribute +0). ftrain_ref.fold_tiles of those terms is the full call's gradient
    element for element: a mask that depended on the tile, the workgroup or the lane that computes it would not fold."""
    import torch
    c, real = loaded(ctx, drop_case("batch5"))
    n = 1024
    rng = np.random.default_rng(77)
    x = rng.normal(0, 1, (n, int(np.prod(c["model"]["in_shape"])))).astype(np.float32)
    with ctx.trainer(padded=True, dropout=c["dropout"], seed=c["seed"]) as tr:
        info = tr.info()
        b, G, w = info["batch"], info["grid"], info["w_floats"]
        assert b == 2
        n_tiles = n // b
        y = (np.arange(n) % tr.n_out).astype(np.int32)
        labels = np.full((n_tiles, n), -1, np.int32)
        for j in range(n_tiles):
            labels[j, j * b:(j + 1) * b] = y[j * b:(j + 1) * b]
        dev = torch.device("cuda", 0)
        xt, yt, lt = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(labels).to(dev)
        torch.cuda.synchronize()
        counter = 5
        tr.dropout_call = counter
        tr.grad_t(xt, yt, n)
        big, z = tr.gradient(), tr.logits(n)
        assert tr.dropout_call == counter + 1
        T = np.empty((n_tiles, w), np.float32)
        for j in range(n_tiles):
            tr.dropout_call = counter
            tr.grad_t(xt, lt[j], n)
            T[j] = tr.gradient()
        assert same_bits(tr.logits(n), z)                                                      # the labels do not move the masks
        assert same_bits(z[:N], fd.forward32(c["model"], x[:N], c["sp"], c["seed"], counter)[-1])
        assert np.isfinite(T).all() and not T[:, ~real].view(np.uint32).any()
        want = ftrain_ref.fold_tiles(T, G, 1)
        nonzero = int(np.count_nonzero(big[real]))
        diff = np.flatnonzero(~(want == big))
        print("batch %d, grid %d, %d tiles; %d of %d real gradient entries are non-zero" % (b, G, n_tiles, nonzero, int(real.sum())))
        assert diff.size == 0, "%d of %d gradient entries are not the fold of the tiles' (%d of %d real entries non-zero; first at %d: call %r, fold %r)" % (
            diff.size, w, nonzero, int(real.sum()), diff[0], big[diff[0]], want[diff[0]])
        assert nonzero > int(real.sum()) // 2, (nonzero, int(real.sum()))
        assert not big[~real].view(np.uint32).any()


def test_refusals_leave_the_previous_setting(ctx):
    c, _ = loaded(ctx, drop_case("pool21_before"))
    L = ctx._L
    with ctx.trainer(padded=True) as tr:
        tr.set_dropout(c["dropout"], seed=9)
        tr.dropout_call = 4
        before = tr.dropout()

        def refused(rates, before_pool=(1, 0), n=None):
            ra, ba = np.asarray(rates, np.float64), np.asarray(before_pool, np.uint8)
            code = L.edison_ftrain_set_dropout(tr._h, ra.ctypes.data_as(ctypes.c_void_p), ba.ctypes.data_as(ctypes.c_void_p), len(rates) if n is None else n, 3)
            assert code == _lib.E_ARGUMENT, (rates, n, code)
            assert tr.dropout() == before

        refused([0.25, 0.0], n=1)                                              # wrong n_records
        refused([0.25, 0.0, 0.0], (1, 0, 0))
        refused([1.0, 0.0])
        refused([-0.1, 0.0])
        refused([float("nan"), 0.0])
        refused([0.25, 0.25])                                                  # a rate on the last record: its output is the logits
        with pytest.raises(_lib.EdisonError) as e:
            tr.set_dropout([0.25, 0.5])
        assert e.value.code == _lib.E_ARGUMENT and "logits" in str(e.value)
        assert L.edison_ftrain_set_dropout_call(tr._h, 1 << 60) == _lib.E_ARGUMENT and tr.dropout() == before
        x = np.ascontiguousarray(c["x"])
        y = np.ascontiguousarray(c["y"])
        loss, am = np.zeros(N, np.float32), np.zeros(N, np.int32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for flags in (2, 3, 0x80000000):                                       # a flag bit other than EVAL
            assert L.edison_ftrain_grad_ex(tr._h, ptr(x), ptr(y), N, ptr(loss), ptr(am), flags) == _lib.E_ARGUMENT
            assert L.edison_ftrain_grad_dev_ex(tr._h, None, None, 0, None, None, flags) == _lib.E_ARGUMENT
        assert tr.dropout() == before
        assert L.edison_ftrain_grad_ex(tr._h, ptr(x), ptr(y), N, ptr(loss), ptr(am), train.FTRAIN_EVAL) == 0 and tr.dropout() == before
        assert L.edison_ftrain_grad_ex(tr._h, ptr(x), ptr(y), N, ptr(loss), ptr(am), 0) == 0 and tr.dropout_call == 5


def test_fit_follows_the_float64_replay_and_validates_without_dropout(ctx):
    """Three noisy class patterns on stride2_same's shape, dropout 0.25 behind the conv, 40 Adam steps at batch 32, lr 0.01: the loss
    history is the float64 HostTrainer replay's to 1e-3 (section 19's tolerance), the final accuracy at least the replay's, and the
    validation entries those of a dropout-free evaluation of the same weights."""
    x, y = ftrain_rows.pad_fit_set()
    model = ftrain_rows.pad_model(ftrain_rows.PAD_FIT_ROW)
    ctx.fnet_load(poisoned(fnet_rows.blob(ftrain_rows.PAD_FIT_ROW))[0])
    dropout = [(0.25, 1), 0]
    kw = dict(fit_kw(), val=(x, y), callbacks=False)
    with ctx.trainer(padded=True, dropout=dropout, seed=3) as tr:
        hist = tr.fit(x, y, **kw)
        assert hist["steps"] == 40 and tr.info()["steps"] == 40 and tr.dropout_call == 40    # validation did not advance the counter
        acc = (ctx.fnet(x)["argmax"] == y).mean()
        r = tr.grad(x, y, training=False)
        assert hist["val_loss"][-1] == float(np.sum(r["loss"], dtype=np.float64)) / len(y)
        assert hist["val_acc"][-1] == (r["argmax"] == y).mean() == acc
    with ctx.trainer(padded=True) as plain:                                    # a trainer that never heard of dropout, the same weights
        r0 = plain.grad(x, y)
        assert same_bits(r0["loss"], r["loss"]) and np.array_equal(r0["argmax"], r["argmax"])
    host = ftrain_ref.HostTrainer(model, dropout, seed=3)
    replay = train.fit(host, x, y, **kw)
    racc = (host.grad(x, y, training=False)["argmax"] == y).mean()
    print("loss %s\nreplay %s\naccuracy %.3f (replay %.3f)" % (np.round(hist["loss"], 5), np.round(replay["loss"], 5), acc, racc))
    assert len(hist["loss"]) == 14 and host.call == 40
    follows_replay(hist, replay)
    assert acc >= racc


def test_kws_train_with_dropout_then_kws_quantize(ctx, tmp_path):
    """kws train --dropout-arch tiny_conv on tiny_conv at 31 x 13 x 1, 5 epochs, then kws quantize of what it wrote."""
    from edison_amd.kws import kws_train
    model = ftrain_rows.pad_model("tiny_conv")
    x, y = ftrain_rows.kws_set()
    keywords = ["k%d" % i for i in range(10)]
    args, val = kws_files(tmp_path, model, x, y, keywords)
    blob, hist, _, trained = kws_trained(ctx, tmp_path, args, val, dropout_arch="tiny_conv")
    assert hist["loss"][-1] < hist["loss"][0]
    plain, _ = kws_train.run(*args, str(tmp_path / "plain.ednf"), epochs=5, batch=32, lr=0.01, val=val, ctx=ctx, out=io.StringIO())
    assert plain != blob                                                    # the masks took part
    again, _ = kws_train.run(*args, str(tmp_path / "again.ednf"), epochs=5, batch=32, lr=0.01, val=val, ctx=ctx, out=io.StringIO(), dropout=[0.25, 0],
                             before_pool=[0, 0])
    assert again == blob                                                    # --dropout 0.25,0 is the arch's placement; same seed, same masks
    for bad in (dict(dropout_arch="no_such"), dict(dropout_arch="tiny_conv", dropout=[0.25, 0]), dict(before_pool=[0, 0])):
        with pytest.raises(ValueError):
            kws_train.run(*args, str(tmp_path / "bad.ednf"), epochs=1, ctx=ctx, out=io.StringIO(), **bad)
    assert kws_train.main(["train"] + args + [str(tmp_path / "bad.ednf"), "--dropout", "x"]) == 1
    assert trained["keywords"] == keywords and struct.unpack_from("<i", blob, 4)[0] == 2
    kws_quantized(ctx, tmp_path)

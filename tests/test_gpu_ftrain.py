"""GPU tests (-m gpu) of training the float32 network (edison_ftrain_*, Context.trainer, kws train) against
tests/ftrain_ref.py, the float64 restatement on the float32 weights.

The gradient bound is measured, not chosen: per tensor the metric is max |g - g64| / max |g64|; torch's CPU float32 autograd of the same
network gets e32 by that metric at run time, and the GPU is allowed 4 e32 -- both are float32 sums of the same terms in different orders
(MFMA four-deep chains and the slab reduce against torch's loops), a factor 4 covers the order, not a wrong term -- floored at
8 x 2^-24 x sqrt(terms summed) so that a tensor where torch happens to be exact does not set a bound of zero. The loss per row is
held the same way, its terms the k rows along the network plus the logits.

Every network is loaded with 1e6 in the padding k rows, padding channels and padding biases of its blob: the packed gradient's padding
must still be exactly +0.0f and a step must leave the weights' padding what it was.

Calls of more tiles than workgroups are tests/test_gpu_ftrain_tiles.py's; the machinery (case, data, poisoned, check_call,
step_checked) is tests/ftrain_drive.py's.

Measured on an MI355X, shipped network, n = 8 (GPU error / e32 per tensor, w then b): see DESIGN.md section 19."""
import numpy as np
import pytest

import fnet_host as fh
import fnet_plan as fpl
import fnet_rows as fr
import ftrain_ref
import ftrain_rows
import stream_drive
from edison_amd import _lib, cube_import, train
from ftrain_drive import (EPS, case, check_call, check_fit_learns, check_gradient, check_plan, data, fnet_logits_of, fnet_logits_of_weights, kws_audio,
                          kws_files, kws_quantized, kws_trained, own_context, poisoned, same_bits, sgd_step_checked, step_checked)

pytestmark = pytest.mark.gpu

ROWS = ["ladder_k5", "pool21_trunc_h", "pool12_trunc_w", "pool22_trunc_hw", "pool41_tail", "inc3_oc64_oc65_s21", "oc40_s32_span_h", "n_out_210",
        "relu_logits", "conv_last_map", "layers16", "batch5", "synth_pool12_relu", "cube_kws"]
ALL_N = ("pool21_trunc_h", "inc3_oc64_oc65_s21", "batch5")      # rows that run n over {1, batch - 1, batch, batch + 1, 3 batch + 2}
LOWERED = ("batch5",)                                  # rows whose dY does not fit the LDS at the network's own batch


@pytest.fixture(scope="module")
def ctx(built_lib):
    yield from own_context()


@pytest.fixture(scope="module")
def fresh(built_lib):
    """A second context: a fresh load of an exported network."""
    yield from own_context()


@pytest.mark.parametrize("name", ROWS)
def test_logits_loss_gradient_padding_repeat_and_no_side_effect(ctx, name):
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    with ctx.trainer() as tr:
        info = tr.info()
        b = info["batch"]
        assert info["w_floats"] == len(real) and info["lds_bytes"] <= 160 * 1024 and info["grid"] >= 1 and info["steps"] == 0
        p = check_plan(blob, info)
        assert (b < p["batch"]) == (name in LOWERED), (name, b, p["batch"])
        ns = sorted({1, max(b - 1, 1), b, b + 1, 3 * b + 2}) if name in ALL_N else [b + 1]
        w0 = tr.packed_weights()
        for n in ns:
            x, y = data(name, model, n)
            g = check_call(ctx, tr, name, model, real, x, y, w0)
            if name == "relu_logits":
                assert not g.any() and np.allclose(tr.grad(x, y)["loss"], np.log(6.0), rtol=1e-6)


@pytest.mark.parametrize("pool", ftrain_ref.TIE_POOLS, ids=lambda p: "pool%d%d" % p)
def test_tied_pool_windows_send_the_gradient_to_their_first_element(ctx, pool):
    """Pool windows of 2 and of 4 elements without ReLU whose maxima tie exactly, the first of them at every element that can tie
    (ftrain_ref.tie_case; tests/test_fgrad_cpu.py shows that sending a tied window's gradient to another of its maxima moves dW by
    more than 1e-2 of its largest entry): the gradient is held to the float64 restatement by the bounds of every other row."""
    model, x, y = ftrain_ref.tie_case(pool)
    name = "tie_pool%d%d" % tuple(pool)
    blob, real = poisoned(cube_import.build_blob(model))
    ctx.fnet_load(blob)
    with ctx.trainer() as tr:
        assert tr.info()["batch"] < len(y)                                  # more than one tile
        check_plan(blob, tr.info())
        check_call(ctx, tr, name, model, real, x, y, tr.packed_weights())


def test_adam_steps_in_place_and_the_exported_network(ctx, fresh):
    name = "pool21_trunc_h"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    x, y = data(name, model, 17)
    lr = 0.01
    with ctx.trainer() as tr:
        adam = ftrain_ref.Adam()
        for step in range(3):
            s = step_checked(tr, real, x, y, [adam], lr, "step %d" % (step + 1))
            assert np.abs(s.got[real] - s.before.astype(np.float64)[real]).max() > 0.5 * lr * 0.9    # the step is lr-sized: Adam's first steps
        assert tr.info()["steps"] == 3
        # the context runs the new weights, and they are the exported network's
        new = ctx.fnet(x)
        exported = cube_import.build_blob(tr.model())
        fresh.fnet_load(exported)
        again = fresh.fnet(x)
        assert same_bits(new["logits"], again["logits"])
        assert not np.array_equal(new["logits"], fnet_logits_of(fresh, blob, x))
        assert tr.export() == exported
        # plain SGD, and reset
        tr.set_opt("sgd")
        sgd_step_checked(tr, real, x, y, 0.1)
        tr.reset()
        assert tr.info()["steps"] == 0


def test_a_network_the_step_kernel_takes_in_two_passes(ctx):
    """dense16_wide has 558 928 packed floats; ed_launch_ftrain_step caps the grid at 8 blocks of 256 threads a CU, so on up to 272 CUs
    its tail is the stride loop's second pass. One gradient at n = batch + 1 against float64, then three Adam steps and one SGD step
    against the float64 restatement over every element, the second pass's reported apart."""
    name = "dense16_wide"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    with ctx.trainer() as tr:
        info = tr.info()
        check_plan(blob, info)
        second = fr.STEP_PASS * info["grid"]
        assert info["w_floats"] == len(real) == 558928 and info["w_floats"] > second, "the packed weights fit one pass of the step kernel on this device"
        assert real[second:].sum() > 1000
        n = info["batch"] + 1
        x, y = data(name, model, n)
        g = check_call(ctx, tr, name, model, real, x, y, tr.packed_weights())
        assert np.count_nonzero(g[second:]) > 1000                      # the second pass has gradients to apply
        adam = ftrain_ref.Adam()
        for step, (opt, lr) in enumerate([(adam, 0.001)] * 3 + [(None, 0.01)]):
            if opt is None:
                tr.set_opt("sgd")
            s = step_checked(tr, real, x, y, [opt], lr, "step %d" % (step + 1))
            err = s.errs[0]
            print("step %d (%s): first pass %.3g, second pass (from element %d) %.3g, bound %.3g" % (
                step + 1, "sgd" if opt is None else "adam", err[:second].max(), second, err[second:].max(), 4 * EPS))
            moved = s.got != s.before
            assert moved[:second].any() and moved[second:].sum() > 1000
        assert tr.info()["steps"] == 4


def test_adam_away_from_its_defaults_over_ten_steps(ctx):
    """b1 = 0.5, b2 = 0.9, eps = 1e-2 at lr = 0.01, ten steps, each on other rows. The bound is the three-step test's 4 x 2^-24 of the
    tensor's maximum: half an ulp of the weight plus an lr-sized update whose relative error is a few 2^-24 per step of drift in m and
    v. At these constants eps is no rounding matter: the same replay at eps = 1e-7 misses the GPU's weights by more than the bound at
    every step."""
    name = "pool21_trunc_h"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    xs, ys = data(name, model, 170)
    lr = 0.01
    with ctx.trainer() as tr:
        check_plan(blob, tr.info())
        tr.set_opt("adam", b1=0.5, b2=0.9, eps=1e-2)
        adam, adam7 = ftrain_ref.Adam(0.5, 0.9, 1e-2), ftrain_ref.Adam(0.5, 0.9, 1e-7)
        worst = 0.0
        for step in range(10):
            s = step_checked(tr, real, xs[17 * step:17 * step + 17], ys[17 * step:17 * step + 17], [adam, adam7], lr, "step %2d" % (step + 1))
            err, err7 = s.errs[0].max(), s.errs[1].max()
            print("step %2d: %.3g (bound %.3g); the replay at eps 1e-7: %.3g" % (step + 1, err, 4 * EPS, err7))
            assert err7 > 4 * EPS, (step, err7)
            worst = max(worst, err)
        print("largest error over ten steps: %.3g" % worst)
        assert tr.info()["steps"] == 10


def test_a_step_at_lr_zero_moves_the_moments_only(ctx):
    name = "pool21_trunc_h"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    xs, ys = data(name, model, 34)
    with ctx.trainer() as tr:
        adam, skipped = ftrain_ref.Adam(), ftrain_ref.Adam()
        s = step_checked(tr, real, xs[:17], ys[:17], [adam], 0.0, "lr = 0")
        assert same_bits(s.got, s.before) and tr.info()["steps"] == 1
        # the next step is the replay's that took the step at lr = 0 too; one that left it out is an lr-sized update away
        s = step_checked(tr, real, xs[17:], ys[17:], [adam, skipped], 0.01, "after lr = 0")
        err, err_skipped = s.errs[0].max(), s.errs[1].max()
        print("after lr = 0: %.3g (bound %.3g); a replay without that step: %.3g" % (err, 4 * EPS, err_skipped))
        assert err_skipped > 4 * EPS and tr.info()["steps"] == 2


def test_refused_optimiser_arguments_leave_the_state(ctx):
    """set_opt with b1 = 1, b2 = -0.1, eps = 0 or a kind that does not exist, and step with a negative, NaN or infinite rate: each
    EDISON_E_ARGUMENT, and the weights, the step count and the constants set before are what they were -- the next step is the
    replay's at those constants."""
    import ctypes
    name = "pool21_trunc_h"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    x, y = data(name, model, 17)
    with ctx.trainer() as tr:
        tr.set_opt("adam", b1=0.5, b2=0.9, eps=1e-2)
        adam = ftrain_ref.Adam(0.5, 0.9, 1e-2)
        step_checked(tr, real, x, y, [adam], 0.01, "before the refusals")
        w1 = tr.packed_weights()
        for kw in (dict(b1=1.0), dict(b2=-0.1), dict(eps=0.0), dict(b1=float("nan")), dict(eps=-1e-7)):
            with pytest.raises(_lib.EdisonError) as e:
                tr.set_opt("adam", **kw)
            assert e.value.code == _lib.E_ARGUMENT and "Adam takes" in str(e.value), kw
        code = tr._L.edison_ftrain_set_opt(tr._h, 7, ctypes.c_double(0.9), ctypes.c_double(0.999), ctypes.c_double(1e-7))
        assert code == _lib.E_ARGUMENT
        with pytest.raises(ValueError):
            tr.set_opt("adadelta")
        for lr in (-1.0, float("nan"), float("inf"), float("-inf")):
            with pytest.raises(_lib.EdisonError) as e:
                tr.step(lr)
            assert e.value.code == _lib.E_ARGUMENT and "learning rate" in str(e.value), lr
        assert tr.info()["steps"] == 1 and same_bits(tr.packed_weights(), w1)
        step_checked(tr, real, x, y, [adam], 0.01, "after the refusals")
        assert tr.info()["steps"] == 2
        assert np.array_equal(ctx.fnet(x)["logits"], fnet_logits_of_weights(ctx, tr, x))


def test_a_call_of_no_rows(ctx):
    name = "pool21_trunc_h"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    x, y = data(name, model, 17)
    with ctx.trainer() as tr:
        tr.set_opt("sgd")
        tr.grad(x, y)
        assert tr.gradient()[real].any()
        r = tr.grad(np.zeros((0, tr.in_n), np.float32), np.zeros(0, np.int32))
        assert r["loss"].shape == (0,) and r["argmax"].shape == (0,) and r["loss"].dtype == np.float32
        assert not tr.gradient().view(np.uint32).any()                      # every entry +0.0f
        z = tr.logits(0)
        assert z.shape == (0, tr.n_out)
        w0 = tr.packed_weights()
        tr.step(0.1)
        assert same_bits(tr.packed_weights(), w0) and tr.info()["steps"] == 1
        # and the trainer goes on: the call after it is the call before it
        tr.grad(x, y)
        g = tr.gradient()
    with ctx.trainer() as again:
        again.grad(x, y)
        assert same_bits(again.gradient(), g)


def test_a_small_call_after_a_large_one(ctx):
    """After 2 grid batch + 1 rows every workgroup's slab holds a sum; a call of one row launches one workgroup and a call of
    batch + 1 rows two, and only their slabs are summed: the bits are a fresh trainer's for the same rows."""
    name = "pool21_trunc_h"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    with ctx.trainer() as tr:
        info = tr.info()
        b, G = info["batch"], info["grid"]
        x, y = data(name, model, 2 * G * b + 1)
        tr.grad(x, y)
        assert tr.gradient()[real].any()
        got = []
        for n in (1, b + 1):
            r = tr.grad(x[:n], y[:n])
            got.append((n, r, tr.gradient(), tr.logits(n)))
    with ctx.trainer() as again:
        for n, r, g, z in got:
            r2 = again.grad(x[:n], y[:n])
            assert same_bits(again.gradient(), g), n
            assert same_bits(r2["loss"], r["loss"]) and np.array_equal(r2["argmax"], r["argmax"])
            assert same_bits(again.logits(n), z)
            assert not g[~real].view(np.uint32).any()


def test_set_weights_round_trip(ctx, fresh):
    name = "inc3_oc64_oc65_s21"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    x, y = data(name, model, 9)
    old = ctx.fnet(x)["logits"]
    with ctx.trainer() as tr:
        rng = np.random.default_rng(19)
        new = [dict(w=(t["w"] * 1.25 + rng.normal(0, 0.01, t["w"].shape)).astype(np.float32),
                    b=(t["b"] - rng.normal(0, 0.05, t["b"].shape)).astype(np.float32)) for t in tr.weights()]
        tr.set_weights(new)
        packed = tr.packed_weights()
        assert (packed[~real] == np.float32(1.0e6)).all()                   # the padding stays what it was
        assert np.array_equal(packed[real], train.pack(new, tr.layout)[real])
        for a, t in zip(tr.weights(), new):
            assert np.array_equal(a["w"], t["w"]) and np.array_equal(a["b"], t["b"])
        now = ctx.fnet(x)["logits"]                                         # the context runs the new weights ...
        assert not np.array_equal(now, old)
        fresh.fnet_load(cube_import.build_blob(tr.model()))                 # ... the ones a fresh load of the exported network runs
        assert same_bits(fresh.fnet(x)["logits"], now)
        tr.grad(x, y)
        assert same_bits(tr.logits(len(y)), now)
        with pytest.raises(ValueError):
            tr.set_packed_weights(packed[:-1])
        with pytest.raises(ValueError):
            tr.set_weights(new[:-1])
        # set_packed_weights takes the whole array, padding included
        tr.set_packed_weights(np.where(real, packed, np.float32(0)))
        assert not tr.packed_weights()[~real].any()
        assert same_bits(ctx.fnet(x)["logits"], now)


def test_refusals_and_the_ignored_counter(ctx):
    pytest.importorskip("torch")
    # a padded network, by name
    ctx.fnet_load(fr.blob("sym3x3"))
    with pytest.raises(_lib.EdisonError) as e:
        ctx.trainer()
    assert e.value.code == _lib.E_NO_IMPL and "record 0" in str(e.value) and "pad" in str(e.value)
    name = "pool21_trunc_h"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    n = 9
    x, y = data(name, model, n)
    tr = ctx.trainer()
    # a host label of n_out and of -1: refused before any launch, the gradient of the call before stays
    tr.grad(x, y)
    g0 = tr.gradient()
    for bad in (3, -1):
        yb = y.copy()
        yb[4] = bad
        with pytest.raises(_lib.EdisonError) as e:
            tr.grad(x, yb)
        assert e.value.code == _lib.E_ARGUMENT and "label" in str(e.value)
    assert np.array_equal(tr.gradient(), g0)
    # the device form: such rows contribute nothing and are counted
    yb = y.copy()
    yb[2], yb[7] = 3, -1
    good = np.array([i for i in range(n) if i not in (2, 7)])
    with stream_drive.torch_stream(ctx) as (torch, dev):
        xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(yb).to(dev)
        loss, am = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        tr.grad_t(xt, yt, n, loss=loss, argmax=am)
        assert tr.info()["ignored"] == 2
        ref = ftrain_ref.loss_grad(model, x[good], y[good], n_total=n)
        check_gradient(name, tr, model, real, x[good], y[good], ref, n_total=n)
        lh = loss.cpu().numpy()
        assert lh[2] == 0 and lh[7] == 0 and (lh[good] > 0).all()
        assert np.array_equal(am.cpu().numpy(), ctx.fnet(x)["argmax"])
        tr.reset()
        assert tr.info()["ignored"] == 0
    # a trainer after a reload
    ctx.fnet_load(blob)
    for call in (lambda: tr.grad(x, y), tr.gradient, lambda: tr.step(0.01), tr.info, tr.packed_weights, tr.reset, lambda: tr.set_opt("sgd")):
        with pytest.raises(_lib.EdisonError) as e:
            call()
        assert e.value.code == _lib.E_NO_MODEL and "another float network was loaded" in str(e.value)
    tr.close()
    with ctx.trainer() as again:
        again.grad(x, y)
        assert np.array_equal(again.gradient(), g0)


def test_a_network_that_fills_the_lds_trains_or_is_refused_by_name(ctx):
    ctx.fnet_load(fr.blob("batch1_lds_max"))
    try:
        with ctx.trainer() as tr:
            assert tr.info()["batch"] == 1 and tr.info()["lds_bytes"] <= 160 * 1024
            check_plan(fr.blob("batch1_lds_max"), tr.info())
    except _lib.EdisonError as e:
        assert e.code == _lib.E_NO_IMPL and "LDS" in str(e)
        assert ftrain_ref.train_batch(fpl.plan(fr.blob("batch1_lds_max"))) == 0


def test_fit_learns_the_synthetic_set(ctx):
    """40 Adam steps at batch 32, lr 0.01, seed 0 on three noisy class patterns: the train loss falls below half its first value and the
    accuracy reaches 0.9 (conditions the float64 replay meets with room: tests/test_fgrad_cpu.py), and the last loss is the replay's."""
    x, y = ftrain_rows.fit_set()
    model = fr.model(ftrain_rows.FIT_ROW)
    check_fit_learns(ctx, dict(), model, cube_import.build_blob(model), x, y)


def test_kws_train_then_kws_quantize(ctx, tmp_path):
    x, y = ftrain_rows.fit_set()
    model = fr.model(ftrain_rows.FIT_ROW)
    args, val = kws_files(tmp_path, model, x, y, ["a", "b", "c"])
    blob, hist, text, trained = kws_trained(ctx, tmp_path, args, val)
    assert "epoch   5" in text and "val_loss" in text
    assert trained["keywords"] == ["a", "b", "c"]
    assert not np.array_equal(fh.conv_records(trained)[0]["w"], fh.conv_records(model)[0]["w"])
    assert np.array_equal(ctx.fnet(x)["logits"], fnet_logits_of(ctx, blob, x))      # the context ran the trained weights already
    # kws quantize takes it: 11 frames x 6 coefficients are the network's 11 x 6 x 1 input
    kws_quantized(ctx, tmp_path, kws_audio(11 * 1024), geometry="frame_count=11,num_mfcc=6,n_samples=11264")

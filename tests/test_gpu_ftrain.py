"""GPU tests (-m gpu) of training the float32 network (edison_ftrain_*, Context.trainer, kws train) against
tests/ftrain_ref.py, the float64 restatement on the float32 weights.

The gradient bound is measured, not chosen: per tensor the metric is max |g - g64| / max |g64|; torch's CPU float32 autograd of the same
network gets e32 by that metric at run time, and the GPU is allowed 4 e32 -- both are float32 sums of the same terms in different orders
(MFMA four-deep chains and the slab reduce against torch's loops), a factor 4 covers the order, not a wrong term -- floored at
8 x 2^-24 x sqrt(terms summed) so that a tensor where torch happens to be exact does not set a bound of zero. The loss per row is
held the same way, its terms the k rows along the network plus the logits.

Every network is loaded with 1e6 in the padding k rows, padding channels and padding biases of its blob: the packed gradient's padding
must still be exactly +0.0f and a step must leave the weights' padding what it was.

Calls of more tiles than workgroups are tests/test_gpu_ftrain_tiles.py's; the helpers here (case, data, poisoned,
check_gradient, check_plan) are shared with it.

Measured on an MI355X, shipped network, n = 8 (GPU error / e32 per tensor, w then b): see DESIGN.md section 19."""
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN

import fnet_host as fh
import fnet_plan as fpl
import fnet_rows as fr
import ftrain_ref
import ftrain_rows
from edison_amd import _lib, cube_import, train

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "cube_kws.ednf")
ROWS = ["ladder_k5", "pool21_trunc_h", "pool12_trunc_w", "pool22_trunc_hw", "pool41_tail", "inc3_oc64_oc65_s21", "oc40_s32_span_h", "n_out_210",
        "relu_logits", "conv_last_map", "layers16", "batch5", "synth_pool12_relu", "cube_kws"]
ALL_N = ("pool21_trunc_h", "inc3_oc64_oc65_s21", "batch5")      # rows that run n over {1, batch - 1, batch, batch + 1, 3 batch + 2}
LOWERED = ("batch5",)                                  # rows whose dY does not fit the LDS at the network's own batch
EPS = 2.0 ** -24


def check_plan(blob, info):
    """The trainer's batch and LDS bytes are the restated plan's (ftrain_ref.train_batch: ftrain_size_lds and the lowering loop)."""
    p = fpl.plan(blob)
    assert info["batch"] == ftrain_ref.train_batch(p) and info["lds_bytes"] == ftrain_ref.train_lds_bytes(p, info["batch"]), (info, p["batch"])
    return p


@pytest.fixture(scope="module")
def ctx(built_lib):
    from edison_amd.context import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh(built_lib):
    """A second context: a fresh load of an exported network."""
    from edison_amd.context import Context
    c = Context(0)
    yield c
    c.close()


def poisoned(blob, value=1.0e6):
    """The blob with `value` in every padding k row, padding channel and padding bias of its weights."""
    model = cube_import.read_blob(blob)
    lay, n = train.layout(model)
    w = np.frombuffer(blob, "<f4", n, len(blob) - 4 * n).copy()
    real = train.pack([dict(w=np.ones(r["shape"], np.float32), b=np.ones(r["out_c"], np.float32)) for r in lay], lay) != 0
    w[~real] = value
    return blob[:len(blob) - 4 * n] + w.astype("<f4").tobytes(), real


_CASES = {}


def case(name):
    """(model, blob with poisoned padding, mask of the packed array's real entries) of a row, built once."""
    if name not in _CASES:
        if name == "cube_kws":
            with open(FIXTURE, "rb") as f:
                blob = f.read()
        else:
            blob = fr.blob(name)
        bad, real = poisoned(blob)
        _CASES[name] = (cube_import.read_blob(blob), bad, real)
    return _CASES[name]


def data(name, model, n):
    in_n = int(np.prod(model["in_shape"]))
    if name == "cube_kws":
        g = np.load(os.path.join(GOLDEN, "cube_golden.npz"))
        rows = np.stack([g["net_in_" + str(k)] for k in g["names"]]).astype(np.float32)
        x = rows[np.arange(n) % len(rows)]
    elif name == "relu_logits":
        assert fr.SWEEP[name][0]["sets"] == ["neg", "n1"]
        x = np.ascontiguousarray(fr.inputs(name, 2 * n, in_n)[0::2])      # its all-negative inputs: every ReLU logit is zero
    else:
        x = ftrain_ref.inputs(name, n, in_n)
    n_out = int(np.prod(fh.conv_records(model)[-1]["out"]))
    return x, (np.arange(n) % n_out).astype(np.int32)


def check_gradient(name, tr, model, real, x, y, ref, n_total=None, report=None):
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
            if report is not None:
                report.append(line)
            assert err <= bound, line


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
            ref = ftrain_ref.loss_grad(model, x, y)
            before = ctx.fnet(x)
            r = tr.grad(x, y)
            # 1. the logits, bit for bit; the argmax is edison_fnet_batch's
            assert np.array_equal(tr.logits(n).view(np.uint32), before["logits"].view(np.uint32)), (name, n)
            assert np.array_equal(r["argmax"], before["argmax"])
            # 2. the loss per row
            lb, le = ftrain_ref.bounds(model, x, y, ref)[1]
            lerr = ftrain_ref.tensor_error(r["loss"], ref["loss"])
            print("%s n=%d loss: gpu %.3g  e32 %.3g  bound %.3g" % (name, n, lerr, le, lb))
            assert lerr <= lb, (name, n, lerr, lb)
            # 3. every tensor's gradient, 4. the padding
            check_gradient(name, tr, model, real, x, y, ref)
            if name == "relu_logits":
                assert not tr.gradient().any() and np.allclose(r["loss"], np.log(6.0), rtol=1e-6)
            # 5. the same call again: the same bits
            g1 = tr.gradient()
            r2 = tr.grad(x, y)
            assert np.array_equal(tr.gradient().view(np.uint32), g1.view(np.uint32)), (name, n)
            assert np.array_equal(r2["loss"].view(np.uint32), r["loss"].view(np.uint32))
            # 6. nothing else moved
            assert np.array_equal(tr.packed_weights().view(np.uint32), w0.view(np.uint32))
            after = ctx.fnet(x)
            assert all(np.array_equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("pool", ftrain_ref.TIE_POOLS, ids=lambda p: "pool%d%d" % p)
def test_tied_pool_windows_send_the_gradient_to_their_first_element(ctx, pool):
    """Pool windows of 2 and of 4 elements without ReLU whose maxima tie exactly, the first of them at every element that can tie
    (ftrain_ref.tie_case; tests/test_fgrad_cpu.py shows that sending a tied window's gradient to another of its maxima moves dW by
    more than 1e-2 of its largest entry): the gradient is held to the float64 restatement by the bounds of every other row."""
    model, x, y = ftrain_ref.tie_case(pool)
    name = "tie_pool%d%d" % tuple(pool)
    blob, real = poisoned(cube_import.build_blob(model))
    ctx.fnet_load(blob)
    ref = ftrain_ref.loss_grad(model, x, y)
    before = ctx.fnet(x)
    with ctx.trainer() as tr:
        assert tr.info()["batch"] < len(y)                                  # more than one tile
        check_plan(blob, tr.info())
        r = tr.grad(x, y)
        assert np.array_equal(tr.logits(len(y)).view(np.uint32), before["logits"].view(np.uint32))
        assert np.array_equal(r["argmax"], before["argmax"])
        check_gradient(name, tr, model, real, x, y, ref)


def test_adam_steps_in_place_and_the_exported_network(ctx, fresh):
    name = "pool21_trunc_h"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    x, y = data(name, model, 17)
    lr = 0.01
    with ctx.trainer() as tr:
        adam = ftrain_ref.Adam()
        for step in range(3):
            w_before = tr.packed_weights().astype(np.float64)
            tr.grad(x, y)
            g = tr.gradient().astype(np.float64)
            tr.step(lr)
            # the float64 restatement fed the GPU's own gradient and the weights the GPU stepped from; m and v run on in float64
            want = [w_before.copy()]
            adam.step(want, [g], lr)
            got = tr.packed_weights()
            for r in tr.layout:
                nb = r["k_pad"] * r["n_pad"]
                for lo, hi in ((r["w_at"], r["w_at"] + nb), (r["w_at"] + nb, r["w_at"] + nb + r["n_pad"])):
                    m = real[lo:hi]
                    err = np.abs(got[lo:hi][m] - want[0][lo:hi][m]).max() / np.abs(want[0][lo:hi][m]).max()
                    print("step %d tensor at %d: %.3g (bound %.3g)" % (step + 1, lo, err, 4 * EPS))
                    assert err <= 4 * EPS, (step, lo, err)
            assert (got[~real] == np.float32(1.0e6)).all()          # zero gradient, zero m and v: the padding stays what it was
            assert np.abs(got[real] - w_before[real]).max() > 0.5 * lr * 0.9    # and the step is lr-sized: Adam's first steps
        assert tr.info()["steps"] == 3
        # the context runs the new weights, and they are the exported network's
        new = ctx.fnet(x)
        exported = cube_import.build_blob(tr.model())
        fresh.fnet_load(exported)
        again = fresh.fnet(x)
        assert np.array_equal(new["logits"].view(np.uint32), again["logits"].view(np.uint32))
        assert not np.array_equal(new["logits"], fnet_logits_of(fresh, blob, x))
        assert tr.export() == exported
        # plain SGD, and reset
        tr.set_opt("sgd")
        w_before = tr.packed_weights().astype(np.float64)
        tr.grad(x, y)
        g = tr.gradient().astype(np.float64)
        tr.step(0.1)
        got = tr.packed_weights()
        assert np.abs(got[real] - (w_before - 0.1 * g)[real]).max() <= 2 * EPS * np.abs(w_before[real]).max()
        tr.reset()
        assert tr.info()["steps"] == 0


def fnet_logits_of(c, blob, x):
    c.fnet_load(blob)
    return c.fnet(x)["logits"]


def step_errors(tr, real, got, want):
    """Per element of the packed array |got - want| / max |want| over the element's tensor (a record's w or its b), real entries
    only; 0 at the padding."""
    err = np.zeros(len(got))
    for r in tr.layout:
        nb = r["k_pad"] * r["n_pad"]
        for lo, hi in ((r["w_at"], r["w_at"] + nb), (r["w_at"] + nb, r["w_at"] + nb + r["n_pad"])):
            m = real[lo:hi]
            err[lo:hi][m] = np.abs(got[lo:hi][m] - want[lo:hi][m]) / np.abs(want[lo:hi][m]).max()
    return err


def grad_and_step(tr, x, y, lr, replays):
    """One gradient call and one step; every replay in `replays` (ftrain_ref.Adam, or None for SGD) takes the step in float64 from the
    weights the GPU stepped from with the GPU's own gradient. Returns (the GPU's weights, each replay's weights, the weights before)."""
    w_before = tr.packed_weights()
    tr.grad(x, y)
    g = tr.gradient().astype(np.float64)
    tr.step(lr)
    wants = []
    for opt in replays:
        want = [w_before.astype(np.float64)]
        if opt is None:
            want[0] -= lr * g
        else:
            opt.step(want, [g], lr)
        wants.append(want[0])
    return tr.packed_weights(), wants, w_before


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
        ref = ftrain_ref.loss_grad(model, x, y)
        before = ctx.fnet(x)
        r = tr.grad(x, y)
        assert np.array_equal(tr.logits(n).view(np.uint32), before["logits"].view(np.uint32))
        assert np.array_equal(r["argmax"], before["argmax"])
        lb = ftrain_ref.bounds(model, x, y, ref)[1][0]
        assert ftrain_ref.tensor_error(r["loss"], ref["loss"]) <= lb
        check_gradient(name, tr, model, real, x, y, ref)
        assert np.count_nonzero(tr.gradient()[second:]) > 1000          # the second pass has gradients to apply
        adam = ftrain_ref.Adam()
        for step, (opt, lr) in enumerate([(adam, 0.001)] * 3 + [(None, 0.01)]):
            if opt is None:
                tr.set_opt("sgd")
            got, (want,), w_before = grad_and_step(tr, x, y, lr, [opt])
            err = step_errors(tr, real, got, want)
            print("step %d (%s): first pass %.3g, second pass (from element %d) %.3g, bound %.3g" % (
                step + 1, "sgd" if opt is None else "adam", err[:second].max(), second, err[second:].max(), 4 * EPS))
            assert err.max() <= 4 * EPS, (step, int(err.argmax()), err.max())
            assert (got[~real] == np.float32(1.0e6)).all()
            moved = got != w_before
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
            got, (want, want7), _ = grad_and_step(tr, xs[17 * step:17 * step + 17], ys[17 * step:17 * step + 17], lr, [adam, adam7])
            err, err7 = step_errors(tr, real, got, want).max(), step_errors(tr, real, got, want7).max()
            print("step %2d: %.3g (bound %.3g); the replay at eps 1e-7: %.3g" % (step + 1, err, 4 * EPS, err7))
            assert err <= 4 * EPS, (step, err)
            assert err7 > 4 * EPS, (step, err7)
            assert (got[~real] == np.float32(1.0e6)).all()
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
        got, _, w_before = grad_and_step(tr, xs[:17], ys[:17], 0.0, [adam])
        assert np.array_equal(got.view(np.uint32), w_before.view(np.uint32)) and tr.info()["steps"] == 1
        # the next step is the replay's that took the step at lr = 0 too; one that left it out is an lr-sized update away
        got, (want, want_skipped), _ = grad_and_step(tr, xs[17:], ys[17:], 0.01, [adam, skipped])
        err, err_skipped = step_errors(tr, real, got, want).max(), step_errors(tr, real, got, want_skipped).max()
        print("after lr = 0: %.3g (bound %.3g); a replay without that step: %.3g" % (err, 4 * EPS, err_skipped))
        assert err <= 4 * EPS and err_skipped > 4 * EPS and tr.info()["steps"] == 2


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
        got, (want,), _ = grad_and_step(tr, x, y, 0.01, [adam])
        assert step_errors(tr, real, got, want).max() <= 4 * EPS
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
        assert tr.info()["steps"] == 1 and np.array_equal(tr.packed_weights().view(np.uint32), w1.view(np.uint32))
        got, (want,), _ = grad_and_step(tr, x, y, 0.01, [adam])
        err = step_errors(tr, real, got, want).max()
        assert err <= 4 * EPS and tr.info()["steps"] == 2, err
        assert np.array_equal(ctx.fnet(x)["logits"], fnet_logits_of_weights(ctx, tr, x))


def fnet_logits_of_weights(c, tr, x):
    """The logits a trainer's own forward half gives on its weights now."""
    tr.grad(x, np.zeros(len(x), np.int32))
    return tr.logits(len(x))


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
        assert np.array_equal(tr.packed_weights().view(np.uint32), w0.view(np.uint32)) and tr.info()["steps"] == 1
        # and the trainer goes on: the call after it is the call before it
        tr.grad(x, y)
        g = tr.gradient()
    with ctx.trainer() as again:
        again.grad(x, y)
        assert np.array_equal(again.gradient().view(np.uint32), g.view(np.uint32))


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
            assert np.array_equal(again.gradient().view(np.uint32), g.view(np.uint32)), n
            assert np.array_equal(r2["loss"].view(np.uint32), r["loss"].view(np.uint32)) and np.array_equal(r2["argmax"], r["argmax"])
            assert np.array_equal(again.logits(n).view(np.uint32), z.view(np.uint32))
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
        assert np.array_equal(fresh.fnet(x)["logits"].view(np.uint32), now.view(np.uint32))
        tr.grad(x, y)
        assert np.array_equal(tr.logits(len(y)).view(np.uint32), now.view(np.uint32))
        with pytest.raises(ValueError):
            tr.set_packed_weights(packed[:-1])
        with pytest.raises(ValueError):
            tr.set_weights(new[:-1])
        # set_packed_weights takes the whole array, padding included
        tr.set_packed_weights(np.where(real, packed, np.float32(0)))
        assert not tr.packed_weights()[~real].any()
        assert np.array_equal(ctx.fnet(x)["logits"].view(np.uint32), now.view(np.uint32))


def test_refusals_and_the_ignored_counter(ctx):
    torch = pytest.importorskip("torch")
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
    dev = torch.device("cuda", 0)
    xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(yb).to(dev)
    loss, am = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    ctx.use_torch_stream()
    try:
        tr.grad_t(xt, yt, n, loss=loss, argmax=am)
        assert tr.info()["ignored"] == 2
        ref = ftrain_ref.loss_grad(model, x[good], y[good], n_total=n)
        check_gradient(name, tr, model, real, x[good], y[good], ref, n_total=n)
        lh = loss.cpu().numpy()
        assert lh[2] == 0 and lh[7] == 0 and (lh[good] > 0).all()
        assert np.array_equal(am.cpu().numpy(), ctx.fnet(x)["argmax"])
        tr.reset()
        assert tr.info()["ignored"] == 0
    finally:
        ctx.use_own_stream()
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
    ctx.fnet_load(cube_import.build_blob(model))
    kw = dict(epochs=100, batch_size=ftrain_rows.FIT_BATCH, seed=0, lr=ftrain_rows.FIT_LR, max_steps=ftrain_rows.FIT_STEPS)
    with ctx.trainer() as tr:
        hist = tr.fit(x, y, **kw)
        assert hist["steps"] == 40 and tr.info()["steps"] == 40
        acc = (ctx.fnet(x)["argmax"] == y).mean()
    replay = train.fit(ftrain_ref.HostTrainer(model), x, y, **kw)
    print("loss %.5f -> %.5f (float64 replay %.5f), accuracy %.3f" % (hist["loss"][0], hist["loss"][-1], replay["loss"][-1], acc))
    assert hist["loss"][-1] < 0.5 * hist["loss"][0] and acc >= 0.9
    assert abs(hist["loss"][-1] - replay["loss"][-1]) <= 1e-3 * replay["loss"][-1]
    assert len(hist["loss"]) == len(replay["loss"]) == 14


def test_kws_train_then_kws_quantize(ctx, tmp_path):
    from edison_amd.kws import kws_quantize, kws_train
    x, y = ftrain_rows.fit_set()
    model = fr.model(ftrain_rows.FIT_ROW)
    with open(tmp_path / "net.ednf", "wb") as f:
        f.write(cube_import.build_blob(model, ["a", "b", "c"]))
    np.save(tmp_path / "x.npy", x)
    np.save(tmp_path / "y.npy", y)
    out = io.StringIO()
    blob, hist = kws_train.run(str(tmp_path / "net.ednf"), str(tmp_path / "x.npy"), str(tmp_path / "y.npy"), str(tmp_path / "out.ednf"), epochs=5,
                               batch=32, lr=0.01, val=(str(tmp_path / "x.npy"), str(tmp_path / "y.npy")), ctx=ctx, out=out)
    assert (tmp_path / "out.ednf").read_bytes() == blob and hist["steps"] == 15 and len(hist["val_loss"]) == 5
    assert "epoch   5" in out.getvalue() and "val_loss" in out.getvalue() and "after 15 steps" in out.getvalue()
    trained = cube_import.read_blob(blob)
    assert trained["keywords"] == ["a", "b", "c"]
    assert not np.array_equal(fh.conv_records(trained)[0]["w"], fh.conv_records(model)[0]["w"])
    assert np.array_equal(ctx.fnet(x)["logits"], fnet_logits_of(ctx, blob, x))      # the context ran the trained weights already
    # kws quantize takes it: 11 frames x 6 coefficients are the network's 11 x 6 x 1 input
    rng = np.random.default_rng(8)
    np.save(tmp_path / "audio.npy", np.clip(rng.normal(0, 3000, (6, 11 * 1024)), -32768, 32767).astype(np.int16))
    qblob, rep = kws_quantize.run(str(tmp_path / "out.ednf"), str(tmp_path / "audio.npy"), str(tmp_path / "q.ednn"),
                                  geometry="frame_count=11,num_mfcc=6,n_samples=11264", ctx=ctx, out=io.StringIO())
    assert (tmp_path / "q.ednn").read_bytes() == qblob and len(rep["float_argmax"]) == 6

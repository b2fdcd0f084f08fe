"""GPU checks of training from scratch on a device-resident data set (edison_ftrain_data_*, edison_ftrain_epoch, Adadelta; DESIGN.md
section 19d): the gather and the store bit for bit against batch-by-batch gradient calls, the features computed from audio against
Context.kws_float's, the reduction against the per-row arrays, Trainer.fit_data against Trainer.fit bit for bit, a get_model network
learning the synthetic set, the Adadelta kernel against its float64 restatement (ftrain_ref.Adadelta), the refusals and the command line."""
import io

import numpy as np
import pytest

import fnet_host as fh
import fnet_rows as fr
import ftrain_drive
import ftrain_ref
import ftrain_rows
from edison_amd import _lib, cube_import, train
from ftrain_drive import EPS, fit_kw, kws_audio, kws_quantized, own_context, same_bits, sgd_step_checked, step_checked
from ftrain_rows import SCRATCH_ARCH, SCRATCH_STEPS, scratch_model

pytestmark = pytest.mark.gpu

SMALL_GEOMETRY = "frame_count=11,num_mfcc=6,n_samples=11264"       # test_kws_train_then_kws_quantize's: 11 x 6 features


@pytest.fixture(scope="module")
def ctx(built_lib):
    yield from own_context()


@pytest.fixture(scope="module")
def fresh(built_lib):
    yield from own_context()


def fc_case(in_shape, classes, n, seed=11):
    """(blob of get_model's single_fc, x [n][in_n] N(0, 1), y = i % classes)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (n, int(np.prod(in_shape)))).astype(np.float32)
    return cube_import.build_blob(train.get_model("single_fc", in_shape, classes, seed=1)), x, (np.arange(n) % classes).astype(np.int32)


def small_geometry():
    from edison_amd import config as cfg
    from edison_amd.kws.kws_eval import parse_geometry
    return parse_geometry(SMALL_GEOMETRY, net_input_scale=cfg.net_input_scale)


def small_audio():
    return kws_audio(11 * 1024)


# ---- the gather and the store ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_shape,classes", [((5, 3, 1), 3), ((31, 13, 1), 10)])
def test_an_epoch_at_lr_zero_is_the_gradient_calls_batch_by_batch(ctx, in_shape, classes):
    n = 23
    blob, x, y = fc_case(in_shape, classes, n)
    ctx.fnet_load(blob)
    rng = np.random.default_rng(5)
    orders = [rng.permutation(n), rng.integers(0, n, 31), np.array([7])]
    with ctx.train_data(x, y) as data, ctx.trainer() as tr, ctx.trainer() as other:
        assert data.n == n and data.in_n == x.shape[1] == tr.in_n
        gx, gy = data.rows()
        assert same_bits(gx, x) and np.array_equal(gy, y)
        w0 = tr.packed_weights()
        steps = 0
        for order in orders:
            for bs in (5, 23, 64):
                r = tr.epoch(data, order, bs, lr=0.0)
                rows = tr.epoch_rows()
                want_steps = -(-len(order) // bs)
                steps += want_steps
                assert r["seen"] == len(order) == len(rows["loss"]) == len(rows["argmax"]) and r["steps"] == want_steps
                for b0 in range(0, len(order), bs):
                    pick = order[b0:b0 + bs]
                    want = other.grad(x[pick], y[pick])
                    assert same_bits(rows["loss"][b0:b0 + bs], want["loss"]), (len(order), bs, b0)
                    assert np.array_equal(rows["argmax"][b0:b0 + bs], want["argmax"]), (len(order), bs, b0)
                assert r["hits"] == int((rows["argmax"] == y[order]).sum())
                total = float(np.sum(rows["loss"].astype(np.float64)))
                assert abs(r["loss_sum"] - total) <= len(order) * 2.0 ** -52 * float(np.abs(rows["loss"]).astype(np.float64).sum())
        assert tr.info()["steps"] == steps and same_bits(tr.packed_weights(), w0)      # lr 0: the weights stay, Adam's t runs
        # max_steps ends the epoch early; no rows, no steps
        r = tr.epoch(data, orders[0], 5, lr=0.0, max_steps=2)
        assert (r["seen"], r["steps"]) == (10, 2) and len(tr.epoch_rows()["loss"]) == 10
        for r in (tr.epoch(data, orders[0], 5, lr=0.0, max_steps=0), tr.epoch(data, [], 5, lr=0.0)):
            assert r == dict(loss_sum=0.0, hits=0, seen=0, steps=0) and len(tr.epoch_rows()["loss"]) == 0
        # a larger set, then a smaller one, in the same store
        for m in (40, 7):
            bx = np.random.default_rng(m).normal(0, 1, (m, x.shape[1])).astype(np.float32)
            by = (np.arange(m)[::-1] % classes).astype(np.int32)
            data.set(bx, by)
            gx, gy = data.rows()
            assert data.n == m and same_bits(gx, bx) and np.array_equal(gy, by)
            order = np.arange(m)[::-1]
            tr.epoch(data, order, 16, lr=0.0)
            want = other.grad(bx[order[:16]], by[order[:16]])
            assert same_bits(tr.epoch_rows()["loss"][:16], want["loss"])
        with pytest.raises(ValueError):
            data.set(bx, -by - 1)                                   # a label outside [0, 2^31)
        bad = by.copy()
        bad[3] = -2
        assert ctx._L.edison_ftrain_data_set(data._h, bx.ctypes.data, bad.ctypes.data, m) == _lib.E_ARGUMENT
        assert data.n == 7 and np.array_equal(data.rows()[1], by)   # refused: the contents stay


def test_a_data_set_from_torch_device_tensors(ctx):
    import torch
    blob, x, y = fc_case((5, 3, 1), 3, 23)
    ctx.fnet_load(blob)
    with train.DeviceData(ctx, 15) as data, ctx.train_data(x, y) as host, ctx.trainer() as tr:
        data.set_t(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
        torch.cuda.synchronize()
        gx, gy = data.rows()
        assert data.n == 23 and same_bits(gx, x) and np.array_equal(gy, y)
        assert tr.evaluate(data) == tr.evaluate(host)


# ---- from audio ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True])
def test_features_from_audio_are_kws_floats(ctx, q15):
    g, audio = small_geometry(), small_audio()
    labels = (np.arange(6) % 3).astype(np.int32)
    ctx.fnet_load(cube_import.build_blob(train.get_model("single_fc", (11, 6, 1), 3)))
    want = ctx.kws_float(audio, geometry=g, q15=q15)["feat"]
    assert want.shape == (6, 66) and np.abs(want).max() > 0
    for chunk in (16384, 4):                                         # one chunk; chunks of 4 + 2
        with ctx.train_data(audio=audio, y=labels, geometry=g, q15=q15, chunk=chunk) as data:
            gx, gy = data.rows()
            assert data.n == 6 and data.in_n == 66
            assert same_bits(gx, want), chunk
            assert np.array_equal(gy, labels)
    with train.DeviceData(ctx, 66) as data:
        from dataclasses import replace
        with pytest.raises(_lib.EdisonError) as e:
            data.set_audio(audio, labels, geometry=replace(g, num_mfcc=5), q15=q15)
        assert e.value.code == _lib.E_SIZE and "55" in str(e.value) and "66" in str(e.value)
        assert data.n == 0
        with pytest.raises(_lib.EdisonError) as e:                   # the geometry's own errors
            data.set_audio(audio, labels, geometry=replace(g, frame_step=0), q15=False)
        assert e.value.code == _lib.E_ARGUMENT


# ---- the reduction ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_eval_sums_the_rows_in_double_in_a_fixed_order(ctx, n):
    blob, x, y = fc_case((5, 3, 1), 3, n, seed=n)
    ctx.fnet_load(blob)
    with ctx.train_data(3.0 * x, y) as data, ctx.trainer() as tr:
        w0, info0 = tr.packed_weights(), tr.info()
        r = tr.evaluate(data)
        rows = tr.epoch_rows()
        assert r["seen"] == n == len(rows["loss"]) and r["steps"] == 0
        assert r["hits"] == int((rows["argmax"] == y).sum())
        total = float(np.sum(rows["loss"].astype(np.float64)))
        bound = n * 2.0 ** -52 * float(np.abs(rows["loss"]).astype(np.float64).sum())
        print("n %d: loss_sum %.17g, numpy %.17g, bound %.3g" % (n, r["loss_sum"], total, bound))
        assert abs(r["loss_sum"] - total) <= bound and r["loss_sum"] > 0
        again = tr.evaluate(data)
        assert np.float64(again["loss_sum"]).view(np.uint64) == np.float64(r["loss_sum"]).view(np.uint64) and again == r
        for b0 in range(0, n, 4096):                                 # 4097 crosses the 4096-row chunk
            want = tr.grad(3.0 * x[b0:b0 + 4096], y[b0:b0 + 4096], training=False)
            assert same_bits(rows["loss"][b0:b0 + 4096], want["loss"]) and np.array_equal(rows["argmax"][b0:b0 + 4096], want["argmax"])
        assert same_bits(tr.packed_weights(), w0) and tr.info() == info0


# ---- fit_data is fit -------------------------------------------------------------------------------------------------------------------
def two_conv_model():
    """A two-conv network on the synthetic set's 11 x 6 x 1 input, of test_gpu_ftrain_bn.py's kind: conv, pool (2, 1); conv; dense."""
    recs = fr._records((11, 6, 1), [("conv", 4, (3, 3), (1, 1), (2, 1), 1), ("conv", 6, (2, 2), (1, 1), (1, 1), 1), ("dense", 3, 0)], pad_keys=False)
    rng = np.random.default_rng(99)
    for L in recs:
        oc, (kh, kw), ic = L["out"][2], L["k"], L["inp"][2]
        L["w"] = (rng.normal(0, 1, (oc, kh, kw, ic)) / np.sqrt(kh * kw * ic)).astype(np.float32)
        L["b"] = rng.normal(0, 0.1, oc).astype(np.float32)
    recs.append(dict(type=cube_import.T_SOFTMAX, inp=recs[-1]["out"], out=recs[-1]["out"]))
    return dict(in_shape=(11, 6, 1), layers=recs)


FIT_TRAINERS = {
    "plain": (lambda: fr.model(ftrain_rows.FIT_ROW), dict()),
    "dropout": (lambda: fr.model(ftrain_rows.FIT_ROW), dict(dropout=[0.25, 0], seed=3)),
    "batchnorm_dropout": (two_conv_model, dict(dropout=[(0.25, 1), 0.25, 0], seed=3, batchnorm=dict(has_bn=[1, 1, 0], max_rows=5))),
}


@pytest.mark.parametrize("kind", sorted(FIT_TRAINERS))
def test_fit_data_is_fit(ctx, fresh, kind):
    make, targs = FIT_TRAINERS[kind]
    blob = cube_import.build_blob(make())
    assert len(fh.conv_records(make())) == len(targs.get("dropout", [0, 0]))
    x, y = ftrain_rows.fit_set()
    x, y, vx, vy = x[:23], y[:23], x[40:49], y[40:49]
    for extra in (dict(), dict(max_steps=7)):
        kw = dict(epochs=3, batch_size=5, seed=4, lr=0.01, callbacks=True, **extra)
        ctx.fnet_load(blob)
        fresh.fnet_load(blob)
        with ctx.trainer(**targs) as a, fresh.trainer(**targs) as b, fresh.train_data(x, y) as data, fresh.train_data(vx, vy) as val:
            ha = a.fit(x, y, val=(vx, vy), **kw)
            hb = b.fit_data(data, val=val, **kw)
            assert ha["steps"] == hb["steps"] == (7 if extra else 15) == a.info()["steps"] == b.info()["steps"]
            assert same_bits(a.packed_weights(), b.packed_weights())
            assert not np.array_equal(a.packed_weights(), train.pack([dict(w=L["w"], b=L["b"]) for L in train.conv_records(make())], a.layout))
            assert a.dropout()["call"] == b.dropout()["call"] == (ha["steps"] if "dropout" in targs else 0)
            for sa, sb in zip(a.bn_state(), b.bn_state()):
                assert (sa is None) == (sb is None)
                for k in sa or ():
                    assert same_bits(sa[k], sb[k]), k
            for k in ("acc", "val_acc", "lr", "steps", "stopped_early"):
                assert ha[k] == hb[k], (k, ha[k], hb[k])
            assert len(ha["loss"]) == len(hb["loss"]) == (2 if extra else 3) == len(hb["val_loss"])
            for k in ("loss", "val_loss"):
                for va, vb in zip(ha[k], hb[k]):
                    assert abs(va - vb) <= 1e-12 * abs(va), (k, ha[k], hb[k])
            # the context runs the trained network, and the export is the host loop's
            assert same_bits(ctx.fnet(vx)["logits"], fresh.fnet(vx)["logits"])
            assert a.export() == b.export()


# ---- it learns from scratch --------------------------------------------------------------------------------------------------------------
def test_a_get_model_network_learns_the_synthetic_set_through_fit_data(ctx):
    """test_fit_learns_the_synthetic_set's set and conditions, the network built by get_model (single_fc at 40 steps: the float64 host
    trainer meets them there, tests/test_ftrain_zoo_cpu.py) and trained through fit_data."""
    x, y = ftrain_rows.fit_set()
    assert (SCRATCH_ARCH, SCRATCH_STEPS) == ("single_fc", ftrain_rows.FIT_STEPS)
    model = scratch_model()
    ctx.fnet_load(cube_import.build_blob(model))
    kw = fit_kw()
    with ctx.train_data(x, y) as data, ctx.trainer() as tr:
        hist = tr.fit_data(data, **kw)
        assert hist["steps"] == SCRATCH_STEPS == tr.info()["steps"]
        acc = (ctx.fnet(x)["argmax"] == y).mean()
    replay = train.fit(ftrain_ref.HostTrainer(model), x, y, **kw)
    print("loss %.5f -> %.5f (float64 replay %.5f), accuracy %.3f" % (hist["loss"][0], hist["loss"][-1], replay["loss"][-1], acc))
    assert hist["loss"][-1] < 0.5 * hist["loss"][0] and acc >= 0.9
    assert len(hist["loss"]) == len(replay["loss"])


# ---- Adadelta ----------------------------------------------------------------------------------------------------------------------------
def test_adadelta_steps_against_the_float64_restatement(ctx):
    name = "pool21_trunc_h"
    model, blob, real = ftrain_drive.case(name)
    ctx.fnet_load(blob)
    x, y = ftrain_drive.data(name, model, 17)
    with ctx.trainer() as tr:
        tr.set_opt("adadelta", rho=0.95, eps=1e-7)
        replay = ftrain_ref.Adadelta(0.95, 1e-7)
        for step in range(3):
            s = step_checked(tr, real, x, y, [replay], 1.0, "step %d" % (step + 1))
            moved = np.abs(s.got[real] - s.before.astype(np.float64)[real])
            assert moved.max() > 1e-4 and moved.max() < 0.1          # sqrt(eps / (1 - rho)) a step at first, growing slowly
        assert tr.info()["steps"] == 3
        # reset zeroes both averages: the next step is a first step again
        tr.reset()
        assert tr.info()["steps"] == 0
        step_checked(tr, real, x, y, [ftrain_ref.Adadelta(0.95, 1e-7)], 1.0, "after reset")
        # other constants
        tr.reset()
        tr.set_opt("adadelta", rho=0.5, eps=1e-4)
        replay = ftrain_ref.Adadelta(0.5, 1e-4)
        for step in range(2):
            step_checked(tr, real, x, y, [replay], 0.5, "rho 0.5 step %d" % (step + 1))
        # refused settings leave the previous kind and constants
        for bad in (dict(rho=1.0), dict(rho=-0.1), dict(rho=float("nan")), dict(rho=0.95, eps=0.0), dict(rho=0.95, eps=-1e-7),
                    dict(rho=0.95, eps=float("inf"))):
            with pytest.raises(_lib.EdisonError) as e:
                tr.set_opt("adadelta", **bad)
            assert e.value.code == _lib.E_ARGUMENT, bad
        assert ctx._L.edison_ftrain_set_opt(tr._h, 3, 0.9, 0.999, 1e-7) == _lib.E_ARGUMENT
        with pytest.raises(_lib.EdisonError):
            tr.set_opt("adam", b1=1.0)
        for args, kw in ((("adadelta",), {}), (("adam",), dict(rho=0.9)), (("sgd",), dict(rho=0.9)), (("rmsprop",), {})):
            with pytest.raises(ValueError):                          # rho is stated for Adadelta and belongs to no other kind
                tr.set_opt(*args, **kw)
        step_checked(tr, real, x, y, [replay], 0.5, "after refusals")      # still Adadelta at rho 0.5, its state running on
        tr.set_opt("sgd")
        with pytest.raises(_lib.EdisonError):
            tr.set_opt("adadelta", rho=1.0)
        sgd_step_checked(tr, real, x, y, 0.1)                        # still SGD


def test_adadelta_steps_gamma_and_beta_of_a_batchnorm_trainer(ctx):
    """gamma and beta against the float64 restatement fed the GPU's gradients, to 8 x 2^-24 of each tensor's maximum (floored at 1e-3).
    Why 8 and not the weights' 4: beta starts at 0, so after the first step it IS -u and the whole error is u's, not the rounding of
    w - lr u at w's size: u = g sqrt(d + eps) / sqrt(a + eps) takes up to nine float32 roundings (two of them under a square root)
    and the float values of rho, 1 - rho and eps, each at most 2^-24 relative: below 6 x 2^-24 together, 8 with room."""
    c = ftrain_rows.bn_case("bn_p1")
    ctx.fnet_load(c["blob"])
    with ctx.trainer(batchnorm=c["bn"]) as tr:
        tr.set_opt("adadelta", rho=0.95)
        replay = {k: ftrain_ref.Adadelta() for k in ("gamma", "beta")}
        for step in range(2):
            before = tr.bn_state()[0]
            tr.grad(c["x"], c["y"])
            g = tr.bn_gradients()[0]
            tr.step(1.0)
            after = tr.bn_state()[0]
            for k in ("gamma", "beta"):
                want = [before[k].astype(np.float64)]
                replay[k].step(want, [g[k].astype(np.float64)], 1.0)
                scale = max(np.abs(want[0]).max(), 1e-3)             # beta starts at 0: its first step is sqrt(eps / (1 - rho)) = 1.4e-3
                err = np.abs(after[k] - want[0]).max() / scale
                print("step %d %s: %.3g (bound %.3g)" % (step + 1, k, err, 8 * EPS))
                assert err <= 8 * EPS and not np.array_equal(after[k], before[k])
            assert np.array_equal(after["mean"], tr.bn_state()[0]["mean"])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_weights_the_counters_and_the_store(ctx):
    blob = cube_import.build_blob(two_conv_model())
    x, y = ftrain_rows.fit_set()
    x, y = x[:23], y[:23]
    ctx.fnet_load(blob)
    with ctx.trainer(dropout=[0.25, 0, 0], seed=2, batchnorm=dict(has_bn=[1, 0, 0], max_rows=5)) as tr, ctx.train_data(x, y) as data, \
            ctx.train_data(x[:, :15], y) as narrow, ctx.train_data(x, y + 1) as labelled:
        tr.epoch(data, np.arange(10), 5, lr=0.01)                    # two steps: counters that are not zero
        w0, info0, call0, bn0 = tr.packed_weights(), tr.info(), tr.dropout()["call"], tr.bn_state()
        assert info0["steps"] == 2 and call0 == 2

        def refused(code, words, call):
            with pytest.raises(_lib.EdisonError) as e:
                call()
            assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
            assert same_bits(tr.packed_weights(), w0) and tr.info() == info0 and tr.dropout()["call"] == call0
            assert all(same_bits(bn0[0][k], tr.bn_state()[0][k]) for k in bn0[0])
            for d, (wx, wy) in ((data, (x, y)), (labelled, (x, y + 1))):
                gx, gy = d.rows()
                assert same_bits(gx, wx) and np.array_equal(gy, wy)

        refused(_lib.E_ARGUMENT, ["max_rows = 5"], lambda: tr.epoch(data, np.arange(23), 6, lr=0.01))
        refused(_lib.E_ARGUMENT, ["batch"], lambda: tr.epoch(data, np.arange(23), 0, lr=0.01))
        refused(_lib.E_ARGUMENT, ["order[2] = 23"], lambda: tr.epoch(data, [0, 1, 23], 5, lr=0.01))
        refused(_lib.E_ARGUMENT, ["order[0] = -1"], lambda: tr.epoch(data, [-1], 5, lr=0.01))
        refused(_lib.E_ARGUMENT, ["label 3", "row 2"], lambda: tr.epoch(labelled, [0, 1, 3, 2], 5, lr=0.01))      # y + 1: row 2's label is 3
        refused(_lib.E_ARGUMENT, ["label 3", "row 2"], lambda: tr.evaluate(labelled))
        refused(_lib.E_SIZE, ["15", "66"], lambda: tr.epoch(narrow, np.arange(23), 5, lr=0.01))
        refused(_lib.E_SIZE, ["15", "66"], lambda: tr.evaluate(narrow))
        refused(_lib.E_ARGUMENT, ["learning rate"], lambda: tr.epoch(data, np.arange(23), 5, lr=-1.0))
        assert tr.epoch(labelled, [0, 1, 3], 5, lr=0.0)["seen"] == 3  # rows whose labels the network has are fine
        # another network: the trainer is stale, the data sets are not
        w1 = tr.packed_weights()
        ctx.fnet_load(blob)
        for call in (lambda: tr.epoch(data, np.arange(23), 5, lr=0.01), lambda: tr.evaluate(data), lambda: tr.epoch_rows()):
            with pytest.raises(_lib.EdisonError) as e:
                call()
            assert e.value.code == _lib.E_NO_MODEL
        with ctx.trainer() as new:
            assert same_bits(new.packed_weights(), train.pack([dict(w=L["w"], b=L["b"]) for L in train.conv_records(two_conv_model())], new.layout))
            assert new.evaluate(data)["seen"] == 23 and not np.array_equal(w1, new.packed_weights())


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_kws_train_from_scratch_resident_then_kws_quantize(ctx, tmp_path):
    from edison_amd import config as cfg
    from edison_amd.kws import kws_train
    from edison_amd.kws.geometry import KwsGeometry
    rng = np.random.default_rng(12)
    y = (np.arange(64) % 10).astype(np.int32)
    x = (rng.normal(0, 1, (10, 403))[y] + rng.normal(0, 0.3, (64, 403))).astype(np.float32)
    np.save(tmp_path / "x.npy", x.reshape(64, 31, 13, 1))
    np.save(tmp_path / "y.npy", y)
    out = io.StringIO()
    blob, hist = kws_train.run(None, str(tmp_path / "x.npy"), str(tmp_path / "y.npy"), str(tmp_path / "out.ednf"), epochs=1, batch=32, ctx=ctx, out=out,
                               arch="kws_conv", batchnorm_arch="kws_conv", dropout_arch="kws_conv", resident=True)
    assert (tmp_path / "out.ednf").read_bytes() == blob and hist["steps"] == 2 and "after 2 steps" in out.getvalue()
    trained = cube_import.read_blob(blob)
    start = train.get_model("kws_conv")
    assert [L["out"] for L in train.conv_records(trained)] == [L["out"] for L in train.conv_records(start)]
    assert not np.array_equal(train.conv_records(trained)[0]["w"], train.conv_records(start)[0]["w"])
    ctx.fnet_load(str(tmp_path / "out.ednf"))
    assert ctx.fnet_info()["n_out"] == 10 and ctx.fnet(x)["logits"].shape == (64, 10)
    g = KwsGeometry.from_config(net_input_scale=cfg.net_input_scale)
    kws_quantized(ctx, tmp_path, np.clip(rng.normal(0, 3000, (6, g.n_samples)), -32768, 32767).astype(np.int16))     # this test's own draw


def test_kws_train_from_audio_with_adadelta_then_kws_quantize(ctx, tmp_path):
    from edison_amd.kws import kws_train
    audio = small_audio()
    np.save(tmp_path / "audio.npy", audio)
    np.save(tmp_path / "y.npy", (np.arange(6) % 3).astype(np.int32))
    args = ["train", str(tmp_path / "audio.npy"), str(tmp_path / "y.npy")]
    opts = ["--arch", "single_fc", "--in-shape", "11,6,1", "--classes", "3", "--audio", "--geometry", SMALL_GEOMETRY, "--epochs", "2", "--batch", "4",
            "--val", str(tmp_path / "audio.npy"), str(tmp_path / "y.npy")]
    assert kws_train.main(args + [str(tmp_path / "out.ednf")] + opts) == 0
    assert kws_train.main(args + [str(tmp_path / "ada.ednf")] + opts + ["--opt", "adadelta", "--rho", "0.9"]) == 0
    adam, ada = (tmp_path / "out.ednf").read_bytes(), (tmp_path / "ada.ednf").read_bytes()
    start = cube_import.build_blob(train.get_model("single_fc", (11, 6, 1), 3))
    assert len(adam) == len(ada) == len(start) and adam != start and ada != start and adam != ada
    ctx.fnet_load(adam)
    assert ctx.fnet_info()["n_out"] == 3
    kws_quantized(ctx, tmp_path, audio, geometry=SMALL_GEOMETRY)
    assert kws_train.main(args + [str(tmp_path / "bad.ednf")] + opts[:6] + ["--audio", "--geometry", "frame_count=11,num_mfcc=5,n_samples=11264"]) == 1

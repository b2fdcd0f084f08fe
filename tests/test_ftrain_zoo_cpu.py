"""CPU checks of training from scratch: train.get_model's eight architectures against the shapes the tests
already compute, their initialisation, the blob round trip; the Adadelta restatements (ftrain_ref) against torch and each other; the
float64 host trainer learning the synthetic set from a get_model network; the new options of ``kws train``."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import cube_synth
import fnet_rows as fr
import ftrain_ref
import ftrain_rows
from edison_amd import cube_import, train
from edison_amd.kws import kws_train

SHAPE_KEYS = ("inp", "out", "k", "s", "p", "relu", "cpad", "ppad")
SCRATCH_ARCH, SCRATCH_STEPS, scratch_model = ftrain_rows.SCRATCH_ARCH, ftrain_rows.SCRATCH_STEPS, ftrain_rows.scratch_model


def shapes(model):
    return [tuple(tuple(int(v) for v in np.ravel(L[k])) for k in SHAPE_KEYS) for L in train.conv_records(model)]


@pytest.mark.parametrize("name", fr.ZOO)
def test_the_padded_architectures_are_the_ones_the_tests_import(name):
    want = cube_import.read_blob(cube_synth.import_sources(*cube_synth.cube_sources((31, 13, 1), fr.zoo_specs(name))))
    m = train.get_model(name)
    assert shapes(m) == shapes(want)
    assert m["in_shape"] == tuple(want["in_shape"]) and m["layers"][-1]["type"] == cube_import.T_SOFTMAX


def test_kws_conv_is_the_shipped_network():
    with open(os.path.join(GOLDEN, "cube_kws.ednf"), "rb") as f:
        want = cube_import.read_blob(f.read())
    m = train.get_model("kws_conv")
    assert shapes(m) == shapes(want) and len(train.conv_records(m)) == len(train.conv_records(want)) == 5
    assert [L["p"] for L in train.conv_records(m)] == [(2, 1), (2, 1), (1, 1), (1, 1), (1, 1)]


@pytest.mark.parametrize("name", train.ARCHS)
def test_every_architecture_has_its_tables_rows_and_survives_the_blob(name):
    m = train.get_model(name, seed=3)
    recs = train.conv_records(m)
    assert len(recs) == len(train.KERAS_DROPOUT[name]) == len(train.KERAS_BATCHNORM[name])
    assert [L["type"] for L in m["layers"]] == [cube_import.T_CONV] * len(recs) + [cube_import.T_SOFTMAX]
    back = cube_import.read_blob(cube_import.build_blob(m))
    assert shapes(back) == shapes(m) and tuple(back["in_shape"]) == m["in_shape"] and back["n_out"] == 10
    for a, b in zip(train.conv_records(back), recs):
        assert a["w"].dtype == b["w"].dtype == np.float32 and a["w"].shape == b["w"].shape
        assert np.array_equal(a["w"].view(np.uint32), b["w"].view(np.uint32)) and np.array_equal(a["b"].view(np.uint32), b["b"].view(np.uint32))


def test_archs_are_the_tables_keys_and_other_shapes_build():
    assert set(train.ARCHS) == set(train.KERAS_DROPOUT) == set(train.KERAS_BATCHNORM) and len(train.ARCHS) == 8
    m = train.get_model("single_fc", (5, 3, 1), 3)
    assert shapes(m) == [((1, 1, 15), (1, 1, 3), (1, 1), (1, 1), (1, 1), (0,), (0, 0, 0, 0), (0, 0, 0, 0))] and m["in_shape"] == (5, 3, 1)
    m = train.get_model("low_latency_conv", (20, 9, 1), 4)            # its first kernel is as wide as the input is high
    assert train.conv_records(m)[0]["k"] == (8, 20) and train.conv_records(m)[-1]["out"] == (1, 1, 4)
    for bad in (dict(arch="no_such"), dict(arch="kws_conv", in_shape=(8, 8, 1)), dict(arch="tiny_conv", num_classes=0)):
        with pytest.raises(ValueError):
            train.get_model(**bad)


@pytest.mark.parametrize("name", train.ARCHS)
def test_the_initialisation_is_glorot_uniform_with_zero_biases(name):
    m, again, other = train.get_model(name, seed=5), train.get_model(name, seed=5), train.get_model(name, seed=6)
    zoo = train._zoo(name, (31, 13, 1), 10)
    for r, (L, A, O) in enumerate(zip(*[train.conv_records(v) for v in (m, again, other)])):
        (kh, kw), ic, oc = L["k"], L["inp"][2], L["out"][2]
        dense = zoo[r][0] == "dense"
        fan_in, fan_out = (kh * kw * ic, oc) if dense else (kh * kw * ic, kh * kw * oc)
        limit = np.sqrt(6.0 / (fan_in + fan_out))
        assert not dense or (L["inp"][:2] == L["k"] == (1, 1) and L["relu"] == 0)      # behind Flatten: k = (h, w) of a 1 x 1 x n input
        assert L["w"].dtype == np.float32 and L["w"].shape == (oc, kh, kw, ic)
        assert np.abs(L["w"]).max() <= np.float32(limit)
        if L["w"].size >= 1000:
            assert np.abs(L["w"]).max() > 0.9 * limit and abs(float(L["w"].mean())) < 0.1 * limit
        assert L["b"].dtype == np.float32 and L["b"].shape == (oc,) and (L["b"].view(np.uint32) == 0).all()      # +0.0
        assert np.array_equal(L["w"].view(np.uint32), A["w"].view(np.uint32))
        assert not np.array_equal(L["w"], O["w"])
    w = [L["w"] for L in train.conv_records(m)]
    assert len(w) < 2 or not np.array_equal(w[0].ravel()[:8], w[1].ravel()[:8])       # every record its own stream


# ---- Adadelta -----------------------------------------------------------------------------------------------------------------------
def adadelta_case(steps):
    rng = np.random.default_rng(41)
    w0 = rng.normal(0, 0.5, 300)
    gs = [rng.normal(0, 1, 300) * 10.0 ** rng.integers(-4, 1, 300) for _ in range(steps)]
    return w0, gs


def test_the_adadelta_restatement_is_torchs():
    import torch
    w0, gs = adadelta_case(5)
    p = torch.nn.Parameter(torch.tensor(w0, dtype=torch.float64))
    opt = torch.optim.Adadelta([p], lr=1.0, rho=0.95, eps=1e-7)
    ref, w = ftrain_ref.Adadelta(0.95, 1e-7), [w0.copy()]
    for g in gs:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        ref.step(w, [g], 1.0)
        want = p.detach().numpy()
        err = np.abs(w[0] - want).max() / np.abs(want).max()
        assert err <= 1e-12, err
    assert np.abs(w[0] - w0).max() > 1e-3            # it moved


def test_the_float32_arithmetic_of_the_kernel_meets_the_gpu_tests_bound():
    w0, gs = adadelta_case(3)
    ref, k32 = ftrain_ref.Adadelta(0.95, 1e-7), ftrain_ref.Adadelta32(0.95, 1e-7)
    w32 = [w0.astype(np.float32)]
    for i, g in enumerate(gs):
        g32 = g.astype(np.float32)
        # as the GPU test: the float64 restatement steps from the float32 weights with the float32 gradient, its state runs on in float64
        want = [w32[0].astype(np.float64)]
        ref.step(want, [g32.astype(np.float64)], 1.0)
        k32.step(w32, [g32], 1.0)
        err = ftrain_ref.tensor_error(w32[0], want[0])
        print("step %d: %.3g (bound %.3g)" % (i + 1, err, 4 * ftrain_ref.EPS32))
        assert err <= 4 * ftrain_ref.EPS32


# ---- from scratch, in float64 ----------------------------------------------------------------------------------------------------------
def test_the_host_trainer_learns_the_synthetic_set_from_a_get_model_network():
    """test_fit_learns_the_synthetic_set's set and conditions on a freshly initialised network: the GPU test's architecture and steps."""
    x, y = ftrain_rows.fit_set()
    model = scratch_model()
    host = ftrain_ref.HostTrainer(model)
    hist = train.fit(host, x, y, epochs=100, batch_size=ftrain_rows.FIT_BATCH, seed=0, lr=ftrain_rows.FIT_LR, max_steps=SCRATCH_STEPS)
    acc = (host.grad(x, y)["argmax"] == y).mean()
    print("%s, %d steps: loss %.5f -> %.5f, accuracy %.3f" % (SCRATCH_ARCH, hist["steps"], hist["loss"][0], hist["loss"][-1], acc))
    assert hist["steps"] == SCRATCH_STEPS
    assert hist["loss"][-1] < 0.5 * hist["loss"][0] and acc >= 0.9


# ---- fit and fit_data: one epoch loop ----------------------------------------------------------------------------------------------------
FIT_SETTINGS = {
    "validation_and_callbacks": dict(batch_size=32, epochs=3, val=True, steps=9, epochs_run=3),
    "short_last_batch": dict(batch_size=40, epochs=2, steps=6, epochs_run=2),                     # 40 + 40 + 16 rows
    "max_steps_inside_the_second_epoch": dict(batch_size=32, epochs=3, max_steps=4, steps=4, epochs_run=2),
}


@pytest.mark.parametrize("setting", sorted(FIT_SETTINGS))
def test_fit_data_is_fit_on_the_host(setting):
    """train.fit_data on a HostData gives train.fit's history, == on the float lists: the same epoch loop around a trainer whose epoch
    and evaluate loop over grad and step in fit's order and sum as fit sums."""
    kw = dict(FIT_SETTINGS[setting])
    steps, epochs_run, with_val = kw.pop("steps"), kw.pop("epochs_run"), kw.pop("val", False)
    x, y = ftrain_rows.fit_set()
    m = fr.model(ftrain_rows.FIT_ROW)
    val = (x[60:], y[60:]) if with_val else None
    a, b = ftrain_ref.HostTrainer(m), ftrain_ref.HostTrainer(m)
    ha = train.fit(a, x, y, val=val, seed=0, lr=ftrain_rows.FIT_LR, **kw)
    hb = train.fit_data(b, ftrain_ref.HostData(x, y), val=ftrain_ref.HostData(*val) if with_val else None, seed=0, lr=ftrain_rows.FIT_LR, **kw)
    assert ha == hb, (ha, hb)
    assert set(ha) == {"loss", "acc", "val_loss", "val_acc", "lr", "steps", "stopped_early"}
    assert ha["steps"] == steps and len(ha["loss"]) == len(ha["acc"]) == len(ha["lr"]) == epochs_run
    assert len(ha["val_loss"]) == len(ha["val_acc"]) == (epochs_run if with_val else 0)
    assert all(np.array_equal(s[k], t[k]) for s, t in zip(a.weights, b.weights) for k in ("w", "b"))
    assert ha["loss"][-1] < ha["loss"][0]


class Replayed:
    """A trainer that replays fixed numbers through both interfaces: training loss 1.25 a row, validation loss 0.5 a row, every
    prediction class 0."""

    def __init__(self):
        self.lrs = []

    def grad(self, x, y, **kw):
        return dict(loss=np.full(len(y), 0.5 if x.shape[1] == 2 else 1.25), argmax=np.zeros(len(y), np.int32))   # the validation set is marked by its width

    def step(self, lr):
        self.lrs.append(lr)

    def epoch(self, data, order, batch, lr, max_steps):
        steps = (len(order) + batch - 1) // batch
        self.lrs += [lr] * steps
        return dict(loss_sum=1.25 * len(order), hits=int((data.y[order] == 0).sum()), seen=len(order), steps=steps)

    def evaluate(self, data):
        return dict(loss_sum=0.5 * data.n, hits=int((data.y == 0).sum()), seen=data.n, steps=0)


def test_a_constant_validation_loss_halves_the_rate_every_epoch_and_stops_after_eleven():
    """The callbacks' paths through the shared loop, from their code: the first epoch sets the best loss; ReduceLROnPlateau (patience 1)
    halves the rate after every later epoch; EarlyStopping (patience 10) stops on the tenth epoch in a row that does not improve."""
    n, lr0 = 7, 0.01
    x, y = np.arange(n, dtype=np.float32).reshape(n, 1), (np.arange(n) % 2).astype(np.int32)
    vx, vy = np.zeros((3, 2), np.float32), np.array([0, 1, 0], np.int32)
    a, b = Replayed(), Replayed()
    ha = train.fit(a, x, y, epochs=20, batch_size=3, val=(vx, vy), seed=4, lr=lr0)
    hb = train.fit_data(b, ftrain_ref.HostData(x, y), epochs=20, batch_size=3, val=ftrain_ref.HostData(vx, vy), seed=4, lr=lr0)
    for h, t in ((ha, a), (hb, b)):
        assert len(h["loss"]) == len(h["val_loss"]) == 11 and h["stopped_early"] and h["steps"] == 33
        assert h["lr"] == [lr0 * 2.0 ** -max(k - 1, 0) for k in range(11)]
        assert t.lrs == [v for v in h["lr"] for _ in range(3)]
        assert h["loss"] == [1.25] * 11 and h["val_loss"] == [0.5] * 11 and h["acc"] == [4 / 7] * 11 and h["val_acc"] == [2 / 3] * 11
    assert ha == hb


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_kws_train_parses_the_new_options(monkeypatch):
    seen = {}

    def fake_run(*args, **kw):
        seen.clear()
        seen.update(kw, args=args)

    monkeypatch.setattr(kws_train, "run", fake_run)
    three = ["train", "x.npy", "y.npy", "o.ednf"]
    assert kws_train.main(three + ["--arch", "kws_conv"]) == 0
    assert seen["args"] == (None, "x.npy", "y.npy", "o.ednf") and seen["arch"] == "kws_conv" and seen["classes"] == 10 and seen["in_shape"] is None
    assert seen["resident"] is False and seen["audio"] is False and seen["opt"] == "adam" and seen["rho"] is None
    assert seen["batchnorm_arch"] is None and seen["dropout_arch"] is None            # --arch alone turns neither on
    assert kws_train.main(three + ["--arch", "single_fc", "--classes", "3", "--in-shape", "11,6,1", "--audio", "--geometry", "frame_count=11",
                                   "--opt", "adadelta", "--rho", "0.9", "--resident"]) == 0
    assert seen["classes"] == 3 and seen["in_shape"] == (11, 6, 1) and seen["audio"] is True and seen["geometry"] == "frame_count=11"
    assert seen["opt"] == "adadelta" and seen["rho"] == 0.9 and seen["resident"] is True and seen["lr"] is None
    assert kws_train.main(["train", "n.ednf"] + three[1:] + ["--opt", "sgd", "--resident"]) == 0
    assert seen["args"] == ("n.ednf", "x.npy", "y.npy", "o.ednf") and seen["arch"] is None and seen["opt"] == "sgd"
    seen.clear()
    for bad in (["train", "n.ednf"] + three[1:] + ["--arch", "kws_conv"],            # four positionals beside --arch
                three,                                                                  # three without it
                three + ["--arch", "no_such"], three + ["--arch", "kws_conv", "--opt", "rmsprop"],
                three + ["--arch", "kws_conv", "--rho", "0.9"], three + ["--arch", "kws_conv", "--opt", "adam", "--rho", "0.9"],
                three + ["--arch", "kws_conv", "--opt", "adadelta", "--rho", "1.0"], three + ["--arch", "kws_conv", "--in-shape", "11,6"],
                three + ["--arch", "kws_conv", "--classes", "x"], three + ["--arch", "kws_conv", "--geometry", "frame_count=11"],
                three + ["--arch"]):
        assert kws_train.main(bad) == 1, bad
        assert not seen
    monkeypatch.undo()
    for bad in (dict(arch="no_such"), dict(arch="kws_conv", opt="rmsprop"), dict(arch="kws_conv", rho=0.9), dict(arch="kws_conv", net="n.ednf"),
                dict(net="n.ednf", classes=3), dict(net="n.ednf", in_shape=(11, 6, 1)), dict()):
        kw = dict(net=None, x_path="x.npy", y_path="y.npy", out_path="o.ednf")
        kw.update(bad)
        with pytest.raises(ValueError):                  # decided before anything touches the GPU or a file
            kws_train.run(**kw)


def test_the_usage_names_the_new_options():
    from edison_amd import main
    for word in ("--arch", "--resident", "--audio", "--opt", "--rho"):
        assert word in kws_train.USAGE and word in main.USAGE and word in kws_train.__doc__


def test_the_new_kernels_use_no_scratch():
    import re
    import subprocess
    from edison_amd import build as B
    r = subprocess.run([B._hipcc(), "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize", "-O3", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(B.CSRC, "fnet_data_kernels.hip"), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    vgprs = [int(v) for v in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    assert len(names) == len(vgprs) == len(scratch) == len(spills) == 5, r.stderr[-2000:]      # three gathers, the reduction, Adadelta
    for n, v, s, sp in zip(names, vgprs, scratch, spills):
        assert s == 0 and sp == 0 and v <= 64, (n, v, s, sp)
    for word in ("ed_fdata_gather_kernel", "ed_fdata_reduce_kernel", "ed_ftrain_adadelta_kernel"):
        assert any(word in n for n in names), word
    assert "fnet_data_kernels.hip" in B.HIP_SOURCES and "fnet_data.h" in B.HEADERS

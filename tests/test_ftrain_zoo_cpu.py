"""CPU checks of training from scratch: train.get_model's eight architectures against the shapes the tests
already compute, their initialisation, the blob round trip; the Adadelta restatements (fdata_ref) against torch and each other; the
float64 host trainer learning the synthetic set from a get_model network; the new options of ``kws train``."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import fdata_ref
import fgrad_ref
import fnet_pad
import fnet_sweep as fs
from edison_amd import cube_import, train
from edison_amd.kws import kws_train

SHAPE_KEYS = ("inp", "out", "k", "s", "p", "relu", "cpad", "ppad")
# the from-scratch fit tests (here in float64, tests/test_gpu_ftrain_data.py on the GPU): the architecture and the steps at which the
# float64 host trainer meets test_fit_learns_the_synthetic_set's conditions on fgrad_ref.fit_set()
SCRATCH_ARCH, SCRATCH_STEPS = "single_fc", fgrad_ref.FIT_STEPS


def shapes(model):
    return [tuple(tuple(int(v) for v in np.ravel(L[k])) for k in SHAPE_KEYS) for L in train.conv_records(model)]


def scratch_model():
    return train.get_model(SCRATCH_ARCH, fs.model(fgrad_ref.FIT_ROW)["in_shape"], fgrad_ref.FIT_CLASSES)


@pytest.mark.parametrize("name", fnet_pad.ZOO)
def test_the_padded_architectures_are_the_ones_the_tests_import(name):
    want = cube_import.read_blob(fnet_pad.import_sources(*fnet_pad.cube_sources((31, 13, 1), fnet_pad.zoo_specs(name))))
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
    ref, w = fdata_ref.Adadelta(0.95, 1e-7), [w0.copy()]
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
    ref, k32 = fdata_ref.Adadelta(0.95, 1e-7), fdata_ref.Adadelta32(0.95, 1e-7)
    w32 = [w0.astype(np.float32)]
    for i, g in enumerate(gs):
        g32 = g.astype(np.float32)
        # as the GPU test: the float64 restatement steps from the float32 weights with the float32 gradient, its state runs on in float64
        want = [w32[0].astype(np.float64)]
        ref.step(want, [g32.astype(np.float64)], 1.0)
        k32.step(w32, [g32], 1.0)
        err = fdata_ref.tensor_error(w32[0], want[0])
        print("step %d: %.3g (bound %.3g)" % (i + 1, err, 4 * fdata_ref.EPS32))
        assert err <= 4 * fdata_ref.EPS32


# ---- from scratch, in float64 ----------------------------------------------------------------------------------------------------------
def test_the_host_trainer_learns_the_synthetic_set_from_a_get_model_network():
    """test_fit_learns_the_synthetic_set's set and conditions on a freshly initialised network: the GPU test's architecture and steps."""
    x, y = fgrad_ref.fit_set()
    model = scratch_model()
    host = fgrad_ref.HostTrainer(model)
    hist = train.fit(host, x, y, epochs=100, batch_size=fgrad_ref.FIT_BATCH, seed=0, lr=fgrad_ref.FIT_LR, max_steps=SCRATCH_STEPS)
    acc = (host.grad(x, y)["argmax"] == y).mean()
    print("%s, %d steps: loss %.5f -> %.5f, accuracy %.3f" % (SCRATCH_ARCH, hist["steps"], hist["loss"][0], hist["loss"][-1], acc))
    assert hist["steps"] == SCRATCH_STEPS
    assert hist["loss"][-1] < 0.5 * hist["loss"][0] and acc >= 0.9


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

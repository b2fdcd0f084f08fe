"""CPU tests of tests/ftrain_ref.py with BatchNorm, the restatement the GPU tests of BatchNorm in the float32 trainer are held to (DESIGN.md section
19c): against torch's float64 autograd and central differences; that leaving the truncated positions out of the statistics would be
seen; the fold against BatchNorm in inference mode; the precondition of the GPU test's bound on the very inputs it draws; the new
kws train options and the refusals that need no GPU; and the resources of the new kernels from the compiler's remarks."""
import io
import os
import re
import subprocess

import numpy as np
import pytest

import fnet_host
import ftrain_ref
import ftrain_rows
from edison_amd import build as B
from edison_amd import train
from edison_amd.kws import kws_train

torch = pytest.importorskip("torch")


def close(got, want, tol=1e-10):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", ftrain_rows.BN_ROWS)
def test_the_restatement_is_torchs_float64_autograd(name):
    c = ftrain_rows.bn_case(name)
    for call in (0, 1):
        ref, after = ftrain_rows.bn_reference(name, call)
        state = ftrain_rows.bn_state(name, call)
        t = ftrain_ref.torch_grads(c["model"], c["x"], c["y"], torch.float64, dropout=(c["sp"], c["seed"], call), bn=dict(state=state))
        assert close(ref["loss"], t["loss"]) and close(ref["logits"], t["logits"])
        unb = ftrain_ref.moved(state, ref["bn"], unbiased=True)
        for i, (g, tg, b, tb) in enumerate(zip(ref["grads"], t["grads"], ref["bn"], t["bn"])):
            assert close(g["w"], tg["w"]), (name, call, i)
            assert close(g["b_sum"], tg["b"]), (name, call, i)
            if b is None:
                assert tb is None and np.array_equal(g["b"], g["b_sum"])
                continue
            assert not g["b"].any() and np.abs(g["b_sum"]).max() < 1e-12            # sum dz = 0: reported as exactly 0
            assert close(b["gamma"], tb["gamma"]) and close(b["beta"], tb["beta"]), (name, call, i)
            # torch's running statistics: the mean, and the variance with Bessel's correction (the unbiased flag's rule)
            assert close(unb[i]["mean"], tb["mean"]) and close(unb[i]["var"], tb["var"]), (name, call, i)
            # without the flag: the population variance, which is torch's with the correction taken out
            m = ftrain_ref.MOMENTUM
            pop = (tb["var"] - m * np.asarray(state[i]["var"], np.float64)) / (1.0 - m) * (b["N"] - 1.0) / b["N"]
            assert close(after[i]["var"], m * np.asarray(state[i]["var"], np.float64) + (1.0 - m) * pop), (name, call, i)
            assert close(after[i]["mean"], tb["mean"])


@pytest.mark.parametrize("name", ["bn_trunc", "bn_mixed"])
def test_the_restatement_is_the_central_difference_of_its_loss(name):
    c = ftrain_rows.bn_case(name)
    ref, _ = ftrain_rows.bn_reference(name, 0)
    base = [dict(w=np.asarray(L["w"], np.float64), b=np.asarray(L["b"], np.float64)) for L in fnet_host.conv_records(c["model"])]
    state = [None if st is None else {k: np.asarray(v, np.float64).copy() for k, v in st.items()} for st in c["state0"]]

    def mean_loss(weights, st):
        return ftrain_ref.loss_grad(c["model"], c["x"], c["y"], weights=weights, dropout=(c["sp"], c["seed"], 0), bn=dict(state=st))["loss"].mean()

    rng = np.random.default_rng(5)
    h = 1e-6
    for i in range(len(base)):
        picks = [("w", tuple(rng.integers(0, s) for s in base[i]["w"].shape)) for _ in range(3)]
        if state[i] is None:
            picks.append(("b", (int(rng.integers(0, len(base[i]["b"]))),)))
        for k, idx in picks:
            vals = []
            for sgn in (1, -1):
                w = [dict(w=t["w"].copy(), b=t["b"].copy()) for t in base]
                w[i][k][idx] += sgn * h
                vals.append(mean_loss(w, state))
            cd = (vals[0] - vals[1]) / (2 * h)
            assert abs(cd - ref["grads"][i][k][idx]) <= 1e-6 * max(1.0, abs(cd)), (name, i, k, idx, cd, ref["grads"][i][k][idx])
        if state[i] is None:
            continue
        for k in ("gamma", "beta"):
            ch = int(rng.integers(0, len(state[i][k])))
            vals = []
            for sgn in (1, -1):
                st = [None if s is None else {kk: v.copy() for kk, v in s.items()} for s in state]
                st[i][k][ch] += sgn * h
                vals.append(mean_loss(base, st))
            cd = (vals[0] - vals[1]) / (2 * h)
            assert abs(cd - ref["bn"][i][k][ch]) <= 1e-6 * max(1.0, abs(cd)), (name, i, k, ch, cd, ref["bn"][i][k][ch])


@pytest.mark.parametrize("name", ["bn_trunc", "shipped"])
def test_leaving_the_truncated_positions_out_would_be_seen(name):
    """The restatement with the truncated positions left out of the statistics and of dz differs from the right one by more than
    100 x the GPU test's bound on some tensor: the GPU test can see that mistake."""
    c = ftrain_rows.bn_case(name)
    ref, _ = ftrain_rows.bn_reference(name, 0)
    wrong = ftrain_ref.loss_grad(c["model"], c["x"], c["y"], dropout=(c["sp"], c["seed"], 0), bn=dict(state=c["state0"], trunc_in_stats=False))
    per, _, _ = ftrain_rows.bn_bounds(name, 0)
    ratios = []
    for g, gw, b, bw, bound in zip(ref["grads"], wrong["grads"], ref["bn"], wrong["bn"], per):
        ratios.append(ftrain_ref.tensor_error(gw["w"], g["w"]) / bound["w"][0])
        if b is not None:
            ratios += [ftrain_ref.tensor_error(bw[k], b[k]) / bound[k][0] for k in ("gamma", "beta")]
    print(name, "wrong / bound:", np.round(ratios, 1))
    assert max(ratios) > 100, ratios


@pytest.mark.parametrize("name", ["bn_pool21_neg", "bn_mixed", "shipped"])
def test_the_folded_network_is_batchnorm_in_inference_mode(name):
    c = ftrain_rows.bn_case(name)
    rng = np.random.default_rng(31)
    weights = [dict(w=np.asarray(L["w"], np.float64), b=np.asarray(L["b"], np.float64)) for L in fnet_host.conv_records(c["model"])]
    state = [None if st is None else dict(gamma=rng.normal(0, 1, len(st["gamma"])), beta=rng.normal(0, 1, len(st["gamma"])),
                                          mean=rng.normal(0, 1, len(st["gamma"])), var=rng.uniform(0.2, 3, len(st["gamma"]))) for st in c["state0"]]
    want = ftrain_ref.inference(c["model"], c["x"], weights, state)
    got = ftrain_ref.loss_grad(c["model"], c["x"], c["y"], weights=ftrain_ref.fold(weights, state))["logits"]
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", ftrain_rows.BN_ROWS)
def test_the_bounds_precondition_on_the_inputs_the_gpu_test_draws(name):
    """On both training calls: the float32 host model and float64 pick the same pool winner and agree on the sign under every ReLU, and
    the smallest softmax probability is above 1e-4."""
    c = ftrain_rows.bn_case(name)
    for call in (0, 1):
        ref, _ = ftrain_rows.bn_reference(name, call)
        state = ftrain_rows.bn_state(name, call)
        r32 = ftrain_ref.loss_grad(c["model"], c["x"], c["y"], dropout=(c["sp"], c["seed"], call), bn=dict(state=state), dtype=np.float32, detail=True)
        assert r32["logits"].dtype == np.float32
        for L, d32, d64 in zip(fnet_host.conv_records(c["model"]), r32["detail"], ref["detail"]):
            assert np.array_equal(d32["first"], d64["first"]), (name, call)
            if L["relu"]:
                assert np.array_equal(d32["y"] > 0, d64["y"] > 0), (name, call)
        assert ref["probs"].min() > 1e-4, (name, call, ref["probs"].min())


def test_keras_batchnorm_lists_the_eight_architectures():
    assert set(train.KERAS_BATCHNORM) == set(train.KERAS_DROPOUT)
    for k, v in train.KERAS_BATCHNORM.items():
        assert len(v) == len(train.KERAS_DROPOUT[k]) and v[-1] == 0
        assert (sum(v) > 0) == (k == "kws_conv")
    assert train.KERAS_BATCHNORM["kws_conv"] == [1, 1, 1, 1, 0]


def test_kws_train_parses_the_batchnorm_options_and_refuses_without_a_gpu(tmp_path, monkeypatch):
    seen = {}

    def fake_run(*args, **kw):
        seen.update(kw)

    monkeypatch.setattr(kws_train, "run", fake_run)
    base = ["train", "n.ednf", "x.npy", "y.npy", "o.ednf"]
    assert kws_train.main(base + ["--batchnorm", "1,1,0", "--bn-momentum", "0.9", "--bn-eps", "1e-5", "--bn-unbiased", "--dropout-arch", "kws_conv"]) == 0
    assert seen["batchnorm"] == [1, 1, 0] and seen["bn_momentum"] == 0.9 and seen["bn_eps"] == 1e-5 and seen["bn_unbiased"] is True
    assert seen["dropout_arch"] == "kws_conv"
    seen.clear()
    assert kws_train.main(base + ["--batchnorm-arch", "kws_conv"]) == 0
    assert seen["batchnorm_arch"] == "kws_conv" and seen["batchnorm"] is None and seen["bn_unbiased"] is False and seen["bn_momentum"] is None
    assert kws_train.main(base + ["--batchnorm", "1,x"]) == 1
    assert kws_train.main(base + ["--bn-momentum"]) == 1
    monkeypatch.undo()
    # refusals that are decided before anything touches the GPU
    out = io.StringIO()
    for bad in (dict(batchnorm_arch="no_such"), dict(batchnorm_arch="kws_conv", batchnorm=[1, 0]), dict(bn_momentum=0.9), dict(bn_unbiased=True),
                dict(batchnorm=[1, 0], bn_momentum=1.0), dict(batchnorm=[1, 0], bn_eps=0.0), dict(batchnorm=[1, 1])):
        with pytest.raises(ValueError):
            kws_train.run("n.ednf", "x.npy", "y.npy", "o.ednf", out=out, **bad)


def test_the_new_kernels_use_no_scratch_and_at_most_128_vgprs():
    hipcc = B._hipcc()                                         # a missing compiler is an error, as in the build
    csrc = B.CSRC
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize", "-O3", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "fnet_bn_kernels.hip"), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    vgprs = [int(v) for v in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(vgprs) == len(scratch) >= 10, r.stderr[-2000:]
    for n, v, s in zip(names, vgprs, scratch):
        assert s == 0 and v <= 128, (n, v, s)
    assert any("edb_conv_kernel" in n for n in names) and any("edb_back_kernel" in n for n in names)

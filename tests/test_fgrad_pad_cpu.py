"""The float64 restatement of training (tests/ftrain_ref.py) on padded networks held to torch's float64 autograd and to central
differences, to ftrain_ref.loss_grad where every pad is zero, and to the first-present-maximum rule; what tests/test_gpu_ftrain_pad.py
rests on: that float32 and float64 choose the same pool winners and ReLU signs on the very inputs it uses, the trainer's batch with two
ints per padded row, that the float64 replay of its fit meets its thresholds with room; and the compiler's resource remarks of both
instantiations of ed_ftrain_grad_kernel. No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from edison_amd import cube_import, train

import fnet_host
import fnet_plan
import fnet_rows
import ftrain_ref
import ftrain_rows


@pytest.mark.parametrize("name", ftrain_rows.PAD_ROWS)
def test_agrees_with_torch_float64_autograd(name):
    import torch
    m = ftrain_rows.pad_model(name)
    x, y = ftrain_rows.pad_data(name, 5)
    ref = ftrain_ref.loss_grad(m, x, y)
    tor = ftrain_ref.torch_grads(m, x, y, torch.float64)
    assert np.allclose(ref["logits"], tor["logits"], rtol=1e-10, atol=1e-12)
    assert np.allclose(ref["loss"], tor["loss"], rtol=1e-10, atol=1e-12)
    for i, (a, b) in enumerate(zip(ref["grads"], tor["grads"])):
        for k in ("w", "b"):
            scale = max(np.abs(b[k]).max(), 1e-300)
            assert np.abs(a[k] - b[k]).max() <= 1e-10 * scale, (name, i, k, np.abs(a[k] - b[k]).max() / scale)
    # and the forward half is fnet_host's float64 restatement
    for got, want in zip([ref["logits"]], fnet_host.run64(m, x)["acts"][-1:]):
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ["asym_even", "pool41_lead"])
def test_agrees_with_central_differences(name):
    m = ftrain_rows.pad_model(name)
    x, y = ftrain_rows.pad_data(name, 4)
    ref = ftrain_ref.loss_grad(m, x, y)
    base = [dict(w=np.asarray(L["w"], np.float64), b=np.asarray(L["b"], np.float64)) for L in fnet_host.conv_records(m)]
    h = 1e-6
    for i, t in enumerate(base):
        for k in ("w", "b"):
            num = np.zeros(t[k].size)
            for j in range(t[k].size):
                vals = []
                for sgn in (1.0, -1.0):
                    w = [dict(w=u["w"].copy(), b=u["b"].copy()) for u in base]
                    w[i][k].reshape(-1)[j] += sgn * h
                    vals.append(ftrain_ref.loss_grad(m, x, y, weights=w)["loss"].mean())
                num[j] = (vals[0] - vals[1]) / (2 * h)
            g = ref["grads"][i][k].reshape(-1)
            # as tests/test_fgrad_cpu.py: O(h^2) |f'''| + rounding / h between the kinks of ReLU and max
            assert np.abs(num - g).max() <= 1e-7 * max(np.abs(g).max(), 1.0), (name, i, k, np.abs(num - g).max())


@pytest.mark.parametrize("name", ["pool22_trunc_hw", "inc3_oc64_oc65_s21"])
def test_without_pads_it_is_the_unpadded_restatement(name):
    """One restatement serves padded and unpadded networks: a record without cpad / ppad borders nothing. The same bits with the keys
    absent and with explicit zero pads, the forward half fnet_host's float64 one, the live rows the truncated map Ph ph x Pw pw,
    and a plan without a padded record one int a row."""
    m = fnet_rows.model(name)
    recs = fnet_host.conv_records(m)
    assert not any("cpad" in L or "ppad" in L for L in recs)
    zeros = dict(m, layers=[dict(L, cpad=fnet_host.Z4, ppad=fnet_host.Z4) if L in recs else L for L in m["layers"]])
    x = ftrain_ref.inputs(name, 5, int(np.prod(m["in_shape"])))
    y = (np.arange(5) % int(np.prod(recs[-1]["out"]))).astype(np.int32)
    a, b = ftrain_ref.loss_grad(zeros, x, y), ftrain_ref.loss_grad(m, x, y)
    assert np.array_equal(a["loss"], b["loss"]) and np.array_equal(a["logits"], b["logits"])
    for s, t in zip(a["grads"], b["grads"]):
        assert np.array_equal(s["w"], t["w"]) and np.array_equal(s["b"], t["b"])
    assert np.allclose(b["logits"], fnet_host.run64(m, x)["logits"], rtol=1e-12, atol=1e-12)
    assert ftrain_ref.terms(zeros, 5) == ftrain_ref.terms(m, 5) == [5 * L["out"][0] * L["p"][0] * L["out"][1] * L["p"][1] for L in recs]
    q = fnet_plan.plan(fnet_rows.blob(name))
    assert not any(L["pad"] for L in q["layers"])
    p = dict(q, layers=[{k: v for k, v in L.items() if k != "pad"} for L in q["layers"]])       # a plan that never heard of pads
    assert ftrain_ref.train_batch(q) == ftrain_ref.train_batch(p) and ftrain_ref.train_lds_bytes(q, p["batch"]) == ftrain_ref.train_lds_bytes(p, p["batch"])
    mp = [(p["batch"] * L["rows"] + 15) // 16 * 16 for L in p["layers"]]
    backward = dict(p, buf_n=[0] * len(p["buf_n"]), w_lds=0, k_lds=0)
    assert ftrain_ref.train_lds_bytes(backward, p["batch"]) == 4 * max(r * L["n_pad"] for r, L in zip(mp, p["layers"])) + 4 * max(mp)


@pytest.mark.parametrize("pool", ftrain_ref.TIE_PADS, ids=lambda p: "pool%d%d" % p)
def test_tied_windows_send_the_gradient_to_their_first_present_element(pool):
    """The rows tests/test_gpu_ftrain_pad.py holds the trainer's choice to: window 0 has an absent element leading, window 1 two
    trailing; channel 2's present elements all tie. The restatement sends such a window's gradient to its first present element
    only; the last maximum instead moves dW far beyond any rounding bound; an absent element never gets any."""
    import torch
    m, x, y = ftrain_ref.tie_case(pool, ppad=ftrain_ref.TIE_PADS[pool])
    conv = fnet_host.conv_records(m)[0]
    assert conv["relu"] == 0 and fnet_host.conv_map(conv) == (5, 5) and ftrain_ref.live(conv) == 25
    ref = ftrain_ref.loss_grad(m, x, y, detail=True)
    d = ref["detail"][0]
    axis = 0 if pool[0] == 4 else 1
    first = np.moveaxis(d["first"], 1 + axis, 1)                            # [n][window along the pooled axis][other][oc]
    assert first.shape[1] == 2
    assert (first[:, 0, :, 2] == 1).all() and (first[:, 1, :, 2] == 0).all()      # the all-tied channel: the first present element
    assert (first[:, 0] >= 1).all() and (first[:, 1] <= 1).all()            # no absent element anywhere
    for c in (0, 1):                                                        # the other channels tie too, at more than one position
        pre = np.moveaxis(d["pre"], 1 + axis, 1)[..., c]                    # [n][5 along the pooled axis][5]
        w0, w1 = pre[:, 0:3], pre[:, 3:5]
        assert ((w0 == w0.max(axis=1, keepdims=True)).sum(axis=1) > 1).any() and ((w1 == w1.max(axis=1, keepdims=True)).sum(axis=1) > 1).any()
    dy = np.moveaxis(d["dy"], 1 + axis, 1)[..., 2]                          # channel 2: conv rows 0 and 3 take everything
    assert (dy[:, [1, 2, 4]] == 0).all() and (dy[:, [0, 3]] != 0).all()
    last = ftrain_ref.loss_grad(m, x, y, pick="last")
    assert ftrain_ref.tensor_error(last["grads"][0]["w"], ref["grads"][0]["w"]) > 1e-2
    tor = ftrain_ref.torch_grads(m, x, y, torch.float64)
    for a, b in zip(ref["grads"], tor["grads"]):
        assert ftrain_ref.tensor_error(a["w"], b["w"]) <= 1e-10 and ftrain_ref.tensor_error(a["b"], b["b"]) <= 1e-10
    # the blob of such a network is version 2 and the plan counts the absent rows
    p = fnet_plan.plan(cube_import.build_blob(m))
    assert p["layers"][0]["pad"] and p["layers"][0]["rows"] == 40 and p["layers"][0]["live"] == 25


def _float32_choices(m, x):
    """Per record (first [n][Ph][Pw][oc], positive [n][rows][oc], live [rows]) of the bit-exact float32 host model of the kernel
    (fnet_host.pre_activation), each record fed the float32 output of the one before, rows in the kernel's order r = q P + e."""
    out, a = [], np.asarray(x, np.float32)
    for L in fnet_host.conv_records(m):
        Ph, Pw, oc = L["out"]
        P = L["p"][0] * L["p"][1]
        v, live = fnet_host.pre_activation(L, a)
        act = np.maximum(v, np.float32(0)) if L["relu"] else v
        act = np.where(live[:, None], act, np.float32(-np.inf)).reshape(-1, Ph, Pw, P, oc)
        out.append((act.argmax(axis=3), (v > 0).reshape(len(a), -1, oc), live[:Ph * Pw * P]))
        a = act.max(axis=3).reshape(len(a), -1)
    return out


@pytest.mark.parametrize("name", ftrain_rows.PAD_ROWS)
def test_float32_and_float64_make_the_same_choices_on_the_gpu_tests_inputs(name):
    """The precondition of holding the GPU's gradient to float64 by a rounding bound: on the 17 rows tests/test_gpu_ftrain_pad.py uses
    (50 on the rows it also runs at 3 x batch + 2),
    the bit-exact float32 model of the kernel and float64 choose the same element of every pool window and the same sign under every
    ReLU, and no softmax saturates. If a change of seeds breaks this, move the seed offset of ftrain_rows.pad_data; never drop a row."""
    m = ftrain_rows.pad_model(name)
    x, y = ftrain_rows.pad_data(name, ftrain_rows.n_max(name))
    ref = ftrain_ref.loss_grad(m, x, y, detail=True)
    for L, d, (first32, pos32, live) in zip(fnet_host.conv_records(m), ref["detail"], _float32_choices(m, x)):
        ph, pw = L["p"]
        Ph, Pw, oc = L["out"]
        assert np.array_equal(d["first"], first32), name
        bordered = ftrain_ref._border(d["pre"], fnet_host.pads(L)[1], np.nan)[:, :Ph * ph, :Pw * pw]
        pre64 = bordered.reshape(-1, Ph, ph, Pw, pw, oc).transpose(0, 1, 3, 2, 4, 5).reshape(len(x), -1, oc)
        assert np.array_equal(np.isnan(pre64[0, :, 0]), ~live)
        if L["relu"]:
            assert np.array_equal((pre64 > 0)[:, live], pos32[:, live]), name
        if name == ftrain_rows.NEG_T and L is fnet_host.conv_records(m)[0]:
            assert (pre64[:, live] < 0).all()                               # an absent element that became 0 would win its window
    print("%s: smallest softmax probability %.3g" % (name, ref["probs"].min()))
    assert ref["probs"].min() > 1e-4, (name, ref["probs"].min())


def test_neg_no_relu_t_is_negative_everywhere():
    m = ftrain_rows.pad_model(ftrain_rows.NEG_T)
    x, y = ftrain_rows.pad_data(ftrain_rows.NEG_T)
    assert (x < 0).all() and not fnet_host.conv_records(m)[0]["relu"]
    ref = ftrain_ref.loss_grad(m, x, y, detail=True)
    assert all((d["pre"] < 0).all() for d in ref["detail"])                 # every present pre-activation, the logits included
    assert ref["probs"].min() > 1e-4
    zero = fnet_host.layer(fnet_host.conv_records(m)[0], x, absent=0.0)             # what an absent 0 would do: win the windows it is in
    assert (zero == 0).any() and (fnet_host.layer(fnet_host.conv_records(m)[0], x) < 0).all()


LOWERED = {"mid_pads_batch": 5, "simple_conv": 6}      # row -> the batch it trains at, where that is below its forward batch (7, 16)


def test_train_batch_with_two_ints_per_padded_row():
    """ftrain_ref.train_batch on every padded row: all train at their forward batch but mid_pads_batch (5 of 7) and simple_conv (6 of 16:
    its stride-1 'same' conv keeps the whole 31 x 13 map, 16 padded channels of dY and two ints a row); the rule itself on
    pool41_lead's plan and on a limit between two batches."""
    for name in ftrain_rows.PAD_ROWS:
        p = fnet_plan.plan(ftrain_rows.pad_blob(name))
        tb = ftrain_ref.train_batch(p)
        print("%s: forward batch %d, trains at %d, %d bytes" % (name, p["batch"], tb, ftrain_ref.train_lds_bytes(p, tb)))
        assert 1 <= tb <= p["batch"] and ftrain_ref.train_lds_bytes(p, tb) <= fnet_plan.LDS_BYTES
        assert tb == LOWERED.get(name, p["batch"]), (name, tb, p["batch"])
    p = fnet_plan.plan(fnet_rows.blob("pool41_lead"))
    L = p["layers"][0]
    assert L["pad"] and L["rows"] == 24 and L["n_pad"] == 16 and p["batch"] == 16
    mp = 16 * 24
    # one int more per row than the unpadded rule counts, visible where the backward half is the larger one
    lim = 4 * mp * L["n_pad"] + 8 * mp
    fwd = 4 * (16 * sum(p["buf_n"]) + p["w_lds"]) + 4 * p["k_lds"]
    assert ftrain_ref.train_lds_bytes(p, 16) == max(fwd, lim)
    small = dict(p, buf_n=[0, 0], w_lds=0, k_lds=0)                         # the backward half alone
    unpadded = dict(small, layers=[dict(R, pad=False) for R in small["layers"]])
    assert ftrain_ref.train_lds_bytes(small, 16) == lim and ftrain_ref.train_lds_bytes(unpadded, 16) == lim - 4 * mp
    assert ftrain_ref.train_batch(small, limit=lim) == 16 and ftrain_ref.train_batch(small, limit=lim - 1) == 15
    assert ftrain_ref.train_batch(small, limit=ftrain_ref.train_lds_bytes(small, 1) - 1) == 0


def test_fit_replay_in_float64_meets_the_gpu_tests_thresholds():
    """The condition tests/test_gpu_ftrain_pad.py puts on the GPU's fit (loss below half its first value, accuracy 0.9), met with room
    by the float64 replay on the padded restatement: 40 Adam steps at batch 32, lr 0.01, seed 0."""
    x, y = ftrain_rows.pad_fit_set()
    host = ftrain_ref.HostTrainer(ftrain_rows.pad_model(ftrain_rows.PAD_FIT_ROW))
    hist = train.fit(host, x, y, epochs=100, batch_size=ftrain_rows.FIT_BATCH, seed=0, lr=ftrain_rows.FIT_LR, max_steps=ftrain_rows.FIT_STEPS)
    assert hist["steps"] == 40
    r = host.grad(x, y)
    print("first epoch loss %.4f, last %.4f; final loss on the set %.4f, accuracy %.3f" % (hist["loss"][0], hist["loss"][-1], r["loss"].mean(),
                                                                                           (r["argmax"] == y).mean()))
    assert hist["loss"][-1] < 0.25 * hist["loss"][0] and (r["argmax"] == y).mean() >= 0.97


def test_model_dicts_keep_their_pads_through_a_blob():
    """What Trainer.model() / export() rest on: a model dict read from a version-2 blob carries cpad / ppad, and build_blob of it
    (with other weights) is version 2 with the same pads."""
    import struct
    blob = fnet_rows.blob("medium_embedding_conv")
    m = cube_import.read_blob(blob)
    again = dict(m, layers=[dict(L) for L in m["layers"]])
    for L in train.conv_records(again):
        L["w"] = L["w"] * np.float32(1.5)
    out = cube_import.build_blob(again, again.get("keywords"))
    assert struct.unpack_from("<i", out, 4)[0] == 2 and len(out) == len(blob)
    back = cube_import.read_blob(out)
    assert [fnet_host.pads(L) for L in train.conv_records(back)] == [fnet_host.pads(L) for L in train.conv_records(m)]
    assert any(any(c) or any(q) for c, q in map(fnet_host.pads, train.conv_records(back)))


def test_both_gradient_kernels_use_no_scratch_and_fit_four_waves_a_simd(tmp_path):
    """The compiler's resource remarks of fnet_grad_kernels.hip (the method of tests/test_host_cpu.py::test_hot_kernels_use_no_scratch):
    both instantiations of ed_ftrain_grad_kernel spill nothing and hold at most 128 VGPRs, the four waves per SIMD of DESIGN.md
    section 19."""
    from edison_amd import build as B
    name = "fnet_grad_kernels.hip"
    cmd = [B._hipcc(), "--offload-arch=" + B.ARCH, "--cuda-device-only", "-c", "-std=c++17", "-fno-slp-vectorize", "-O3", "-I" + B.CSRC,
           "-Rpass-analysis=kernel-resource-usage"] + B.PER_FILE_FLAGS.get(name, []) + ["-x", "hip", os.path.join(B.CSRC, name), "-o", str(tmp_path / (name + ".o"))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = {}
    for b in blocks:
        fn = b.split()[0]
        if "ed_ftrain_grad_kernel" not in fn:
            continue
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgprs = int(re.search(r"VGPRs: (\d+)", b).group(1))
        print("%s: %d VGPRs, %d bytes of scratch per lane" % (fn, vgprs, scratch))
        seen["ILb1E" in fn] = (vgprs, scratch)
    assert set(seen) == {False, True}, seen                                 # <false> and <true>
    for pads, (vgprs, scratch) in seen.items():
        assert scratch == 0 and vgprs <= 128, (pads, vgprs, scratch)

"""The dropout mask (csrc/fnet_dropout.h), its restatement (tests/fdrop_ref.py) and training with it (tests/ftrain_ref.py) without a GPU: Philox's known answers, a stand-alone host
program on the header, the mask's statistics, the restatement against torch's float64 autograd, central differences and the
dropout-free restatement, the precondition of tests/test_gpu_ftrain_dropout.py's rounding bound on the very inputs it draws, fit's
calls on a scripted trainer, and the compiler's resource remarks of all four instantiations of ed_ftrain_grad_kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

from edison_amd import train

import fdrop_ref as fd
import fnet_host
import ftrain_ref
import ftrain_rows

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "edison_amd", "csrc")


def words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("ctr, key, out", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, out):
    assert [int(w) for w in fd.philox4x32_10(words(ctr), words(key))] == words(out)


def test_keys_are_philox_words_0_and_1_at_the_stated_counter():
    seed, call, u, l = (5 << 32) | 9, (3 << 32) | 77, 123456, 4
    w = fd.philox4x32_10([u, 77, 3, l], [9, 5])
    kA, kB = fd.keys(seed, call, [u], l)
    assert (int(kA[0]), int(kB[0])) == (int(w[0]), int(w[1]))
    assert int(fd.fmix32([1])[0]) == 0x514e28b7                             # MurmurHash3's finaliser of 1
    assert fd.threshold(0.25) == 1 << 30 and fd.threshold(0.5) == 1 << 31 and fd.threshold(0.0) == 0
    assert fd.scale(0.25) == np.float32(4.0 / 3.0) and fd.scale(0.5) == np.float32(2.0)


PROGRAM = r"""
#include <stdio.h>
#include <inttypes.h>
#include "fnet_dropout.h"
int main(void)
{
	unsigned long long seed, call;
	unsigned u, l, e;
	double rate;
	while (scanf("%llu %llu %u %u %u %lf", &seed, &call, &u, &l, &e, &rate) == 6)
		printf("%d %" PRIu32 " %.9g\n", edd_keep(seed, call, u, l, e, rate), edd_threshold(rate), (double)edd_scale(rate));
	return 0;
}
"""


def test_a_stand_alone_host_program_on_the_header_gives_the_restatements_bits(tmp_path):
    """fnet_dropout.h is plain C: a host program with its own main, compiled by the C compiler, prints keep bits that equal
    fdrop_ref.keep, for calls and seeds at and above 2^32 too."""
    import shutil
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        from edison_amd import build as B
        cc = os.path.join(os.path.dirname(B._hipcc()), "amdclang")
    (tmp_path / "keep.c").write_text(PROGRAM)
    r = subprocess.run([cc, "-std=c99", "-O1", "-I" + CSRC, str(tmp_path / "keep.c"), "-o", str(tmp_path / "keep")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(41)
    cases = []
    for seed in (0, 7, 2 ** 32, 2 ** 32 + 5, 2 ** 64 - 1):
        for call in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 3, 2 ** 60 - 1):
            for rate in (0.0, 0.2, 0.25, 0.3, 0.5, 0.999):
                for _ in range(6):
                    cases.append((seed, call, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 16)), int(rng.integers(0, 2 ** 20)), rate))
    cases += [(7, 0, u, l, e, 0.5) for u in (0, 1, 2 ** 32 - 1) for l in (0, 15) for e in (0, 1, 2 ** 32 - 1)]
    text = "".join("%d %d %d %d %d %r\n" % c for c in cases)
    r = subprocess.run([str(tmp_path / "keep")], input=text, capture_output=True, text=True)
    assert r.returncode == 0
    got = [ln.split() for ln in r.stdout.splitlines()]
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert int(g[0]) == int(fd.keep(*c)), c
        assert int(g[1]) == fd.threshold(c[5]) and np.float32(float(g[2])) == fd.scale(c[5]), c
    bits = [int(g[0]) for g in got]
    assert 0 < sum(bits) < len(bits)


N = 1 << 20


def _mask(seed=7, call=0, u=0, l=0, rate=0.5, n=N):
    return fd.kept(seed, call, 1, l, n, rate, u0=u)[0]


@pytest.mark.parametrize("rate", [0.2, 0.25, 0.3, 0.5])
def test_the_kept_fraction_is_one_minus_rate(rate):
    k = _mask(rate=rate)
    sd = np.sqrt(rate * (1 - rate) / N)
    dev = abs(k.mean() - (1 - rate)) / sd
    print("rate %.2f: kept %.6f, %.2f standard deviations" % (rate, k.mean(), dev))
    assert dev <= 4.0


def _corr(a, b):
    a, b = a.astype(np.float64) - a.mean(), b.astype(np.float64) - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_masks_are_uncorrelated_across_samples_records_calls_seeds_and_lags():
    base = _mask()
    others = dict(sample=_mask(u=1), record=_mask(l=1), call=_mask(call=1), seed=_mask(seed=8))
    worst = 0.0
    for name, m in others.items():
        c = _corr(base, m)
        worst = max(worst, abs(c))
        assert abs(c) < 4 / np.sqrt(N), (name, c)
    for lag in (1, 16, 64):
        c = _corr(base[:-lag], base[lag:])
        worst = max(worst, abs(c))
        assert abs(c) < 4 / np.sqrt(N - lag), (lag, c)
    print("largest correlation %.2f / sqrt(N)" % (worst * np.sqrt(N)))


def test_every_element_of_a_small_tensor_is_kept_at_its_rate_over_samples():
    rate, n, m = 0.25, 4096, 64
    k = fd.kept(7, 0, n, 0, m, rate)
    dev = np.abs(k.mean(axis=0) - (1 - rate)) / np.sqrt(rate * (1 - rate) / n)
    print("largest deviation of an element: %.2f standard deviations" % dev.max())
    assert dev.max() <= 4.5


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ftrain_rows.DROP_ROWS)
def test_restatement_agrees_with_torch_float64_autograd(name):
    import torch
    c = ftrain_rows.drop_case(name)
    x, y = c["x"][:5], c["y"][:5]
    ref = ftrain_ref.loss_grad(c["model"], x, y, dropout=(c["sp"], c["seed"], 3))
    tor = ftrain_ref.torch_grads(c["model"], x, y, torch.float64, dropout=(c["sp"], c["seed"], 3))
    assert np.allclose(ref["logits"], tor["logits"], rtol=1e-10, atol=1e-12) and np.allclose(ref["loss"], tor["loss"], rtol=1e-10, atol=1e-12)
    for i, (a, b) in enumerate(zip(ref["grads"], tor["grads"])):
        for k in ("w", "b"):
            assert ftrain_ref.tensor_error(a[k], b[k]) <= 1e-10, (name, i, k)
    plain = ftrain_ref.loss_grad(c["model"], x, y)
    assert not np.array_equal(plain["logits"], ref["logits"])               # the mask does something


@pytest.mark.parametrize("name", ["pool21_before", "pool21_after"])
def test_restatement_agrees_with_central_differences(name):
    c = ftrain_rows.drop_case(name)
    m, x, y = c["model"], c["x"][:4], c["y"][:4]
    ref = ftrain_ref.loss_grad(m, x, y, dropout=(c["sp"], c["seed"], 0))
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
                    vals.append(ftrain_ref.loss_grad(m, x, y, weights=w, dropout=(c["sp"], c["seed"], 0))["loss"].mean())
                num[j] = (vals[0] - vals[1]) / (2 * h)
            g = ref["grads"][i][k].reshape(-1)
            # as tests/test_fgrad_pad_cpu.py: O(h^2) |f'''| + rounding / h between the kinks of ReLU and max
            assert np.abs(num - g).max() <= 1e-7 * max(np.abs(g).max(), 1.0), (name, i, k, np.abs(num - g).max())


@pytest.mark.parametrize("name", ["pool21_before", "mid_pads_batch", "shipped_kws_conv"])
def test_at_rate_zero_it_is_the_dropout_free_restatement_exactly(name):
    c = ftrain_rows.drop_case(name)
    none = fd.spec(c["model"], [0] * len(c["sp"]))
    a, b = ftrain_ref.loss_grad(c["model"], c["x"][:5], c["y"][:5], dropout=(none, 3, 9)), ftrain_ref.loss_grad(c["model"], c["x"][:5], c["y"][:5])
    assert np.array_equal(a["loss"], b["loss"]) and np.array_equal(a["logits"], b["logits"])
    for s, t in zip(a["grads"], b["grads"]):
        assert np.array_equal(s["w"], t["w"]) and np.array_equal(s["b"], t["b"])
    f32 = fd.forward32(c["model"], c["x"][:5], none, 3, 9)
    assert all(np.array_equal(p, q) for p, q in zip(f32, fnet_host.run(c["model"], c["x"][:5])))


@pytest.mark.parametrize("name", ftrain_rows.DROP_ROWS)
def test_float32_and_float64_make_the_same_choices_on_the_gpu_tests_inputs(name):
    """The precondition of holding the GPU's gradient to float64 by a rounding bound, on the 17 rows and the counters (0 and 1)
    tests/test_gpu_ftrain_dropout.py uses: forward32 and float64 choose the same element of every window, the same sign under every
    ReLU and the same dropped-winner bit, and the smallest softmax probability is above 1e-4. If a row fails, give it another mask
    seed in ftrain_rows.DROP_ROWS; never drop a row."""
    c = ftrain_rows.drop_case(name)
    m, x = c["model"], c["x"]
    for call in (0, 1):
        ref = ftrain_rows.drop_reference(name, call)
        _, det = fd.forward32(m, x, c["sp"], c["seed"], call, detail=True)
        for L, d, (first32, pos32, dropped32) in zip(fnet_host.conv_records(m), ref["detail"], det):
            ph, pw = L["p"]
            Ph, Pw, oc = L["out"]
            assert np.array_equal(d["first"].reshape(len(x), -1, oc), first32), name
            assert np.array_equal(d["dropped"].reshape(len(x), -1, oc), dropped32), name
            if L["relu"]:
                bordered = ftrain_ref._border(d["pre"], fnet_host.pads(L)[1], np.nan)[:, :Ph * ph, :Pw * pw]
                pre64 = bordered.reshape(-1, Ph, ph, Pw, pw, oc).transpose(0, 1, 3, 2, 4, 5).reshape(len(x), -1, oc)
                live = ~np.isnan(pre64[0, :, 0])
                assert np.array_equal((pre64 > 0)[:, live], pos32[:, live]), name
        print("%s call %d: smallest softmax probability %.3g" % (name, call, ref["probs"].min()))
        assert ref["probs"].min() > 1e-4, (name, call, ref["probs"].min())
    assert not np.array_equal(ftrain_rows.drop_reference(name, 0)["logits"], ftrain_rows.drop_reference(name, 1)["logits"])


def test_the_rows_cover_what_the_gpu_test_says_they_cover():
    P = lambda name: [L["p"][0] * L["p"][1] for L in fnet_host.conv_records(ftrain_rows.drop_case(name)["model"])]
    assert set(P("p1_inc3")) == {1} and 2 in P("p2_pool12_no_relu_before") and 4 in P("p4_pool22_before") and 4 in P("p4_pool22_after")
    c = ftrain_rows.drop_case("p2_pool12_no_relu_before")
    assert not fnet_host.conv_records(c["model"])[0]["relu"] and c["sp"][0] == (0.25, True)
    c = ftrain_rows.drop_case("neg_no_relu_before")
    assert not fnet_host.conv_records(c["model"])[0]["relu"] and c["sp"][0][1]
    d = ftrain_rows.drop_reference("neg_no_relu_before")["detail"][0]
    assert d["dropped"].any() and not d["dropped"].all()                    # with every value negative a dropped +0 wins its window
    assert ftrain_rows.drop_case("pool21_before")["sp"][0][1] and not ftrain_rows.drop_case("pool21_after")["sp"][0][1]
    rates = {r for name in ftrain_rows.DROP_ROWS for r, _ in ftrain_rows.drop_case(name)["sp"]}
    assert {0.25, 0.5, 0.2, 0.3} <= rates
    assert len(ftrain_rows.drop_case("shipped_kws_conv")["sp"]) == 5
    for name, spec in train.KERAS_DROPOUT.items():
        r, b = train.dropout_spec(spec)
        assert r[-1] == 0.0 and all(0 <= v < 1 for v in r) and len(r) == len(b), name
    assert train.KERAS_DROPOUT["simple_conv"] == [(0.25, 0), 0] and train.KERAS_DROPOUT["kws_conv"] == [0, 0, 0.2, 0.3, 0]


# ---- fit ------------------------------------------------------------------------------------------------------------------------------
class Scripted:
    """A trainer that records how fit calls it."""

    def __init__(self, on=None, keyword=True):
        self.calls, self.on = [], on
        if on is not None:
            self.dropout = lambda: dict(on=on)
        self.grad = self._grad_kw if keyword else self._grad_plain

    def _grad_kw(self, x, y, **kw):
        self.calls.append((len(y), dict(kw)))
        return dict(loss=np.ones(len(y)), argmax=np.asarray(y))

    def _grad_plain(self, x, y):
        self.calls.append((len(y), {}))
        return dict(loss=np.ones(len(y)), argmax=np.asarray(y))

    def step(self, lr):
        pass


def test_fit_evaluates_validation_with_dropout_off_and_leaves_other_trainers_alone():
    x, y = np.zeros((10, 3), np.float32), np.arange(10) % 2
    vx, vy = np.zeros((7, 3), np.float32), np.arange(7) % 2
    t = Scripted(on=True)
    train.fit(t, x, y, epochs=2, batch_size=4, val=(vx, vy))
    train_calls = [c for c in t.calls if c[0] != 7]
    val_calls = [c for c in t.calls if c[0] == 7]
    assert len(train_calls) == 6 and len(val_calls) == 2
    assert all(kw in ({}, dict(training=True)) for _, kw in train_calls)
    assert all(kw == dict(training=False) for _, kw in val_calls)
    for t in (Scripted(on=False), Scripted(on=None), Scripted(on=None, keyword=False)):   # dropout off, or no such notion: today's calls
        train.fit(t, x, y, epochs=2, batch_size=4, val=(vx, vy))
        assert len(t.calls) == 8 and all(kw == {} for _, kw in t.calls)
    c = ftrain_rows.drop_case("pool21_after")

    class Minimal:                                                          # no keyword, no dropout(), no batchnorm(): keeps working
        def __init__(self):
            self.inner = ftrain_ref.HostTrainer(c["model"])

        def grad(self, x, y):
            return self.inner.grad(x, y)

        def step(self, lr):
            self.inner.step(lr)

    host = Minimal()
    h = train.fit(host, c["x"], c["y"], epochs=1, batch_size=8, val=(c["x"], c["y"]))
    assert len(h["val_loss"]) == 1


def test_host_trainer_counts_training_calls_only():
    c = ftrain_rows.drop_case("pool21_before")
    t = ftrain_ref.HostTrainer(c["model"], c["dropout"], seed=c["seed"])
    a = t.grad(c["x"], c["y"])
    assert t.call == 1 and np.array_equal(a["loss"], ftrain_rows.drop_reference("pool21_before", 0)["loss"])
    e = t.grad(c["x"], c["y"], training=False)
    assert t.call == 1 and np.array_equal(e["loss"], ftrain_ref.loss_grad(c["model"], c["x"], c["y"])["loss"])
    b = t.grad(c["x"], c["y"])
    assert t.call == 2 and np.array_equal(b["loss"], ftrain_rows.drop_reference("pool21_before", 1)["loss"])


def test_all_four_gradient_kernels_use_no_scratch_and_fit_four_waves_a_simd(tmp_path):
    """tests/test_fgrad_pad_cpu.py's resource check, on every instantiation by name: <PADS, DROP> for both values of each."""
    from edison_amd import build as B
    name = "fnet_grad_kernels.hip"
    cmd = [B._hipcc(), "--offload-arch=" + B.ARCH, "--cuda-device-only", "-c", "-std=c++17", "-fno-slp-vectorize", "-O3", "-I" + B.CSRC,
           "-Rpass-analysis=kernel-resource-usage"] + B.PER_FILE_FLAGS.get(name, []) + ["-x", "hip", os.path.join(B.CSRC, name), "-o", str(tmp_path / (name + ".o"))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        fn = b.split()[0]
        m = re.search(r"ed_ftrain_grad_kernelILb([01])ELb([01])E", fn)
        if not m:
            continue
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgprs = int(re.search(r"VGPRs: (\d+)", b).group(1))
        print("%s: %d VGPRs, %d bytes of scratch per lane" % (fn, vgprs, scratch))
        seen[m.group(1), m.group(2)] = (vgprs, scratch)
    assert set(seen) == {(a, b) for a in "01" for b in "01"}, seen
    for key, (vgprs, scratch) in seen.items():
        assert scratch == 0 and vgprs <= 128, (key, vgprs, scratch)

"""GPU tests of the evaluator (edison_eval_*, csrc/eval_kernels.hip, edison_amd/evaluate.py). All counting is in integers, so every
comparison is equality; prob is compared bit for bit.

  * the kernel equals the host functions (edison_nnom_prediction_run / edison_eval_f32_host, which tests/test_eval_cpu.py pins on the
    reference) over n in {1, 63, 64, 65, 257, 5 000} x n_out in {1, 2, 10, 64, 65, 256} -- the LDS matrix, the global matrix and the
    boundary between them; rows of at most 16 bytes (registers) and longer ones --, max_blocks in {1, 2, default} (at n = 5 000 a single
    workgroup makes 20 grid-stride passes), all three rules, the adversarial rows of the CPU pin, per-utterance outputs given and NULL;
  * adds accumulate, reset zeroes, result between adds disturbs nothing, counters do not wrap at 65 536, two evaluators agree byte
    for byte, an add queued behind edison_cnn_batch_dev without a synchronisation counts that call's outputs;
  * Context.evaluate on each audio-to-class flow, in chunks with a short last one and unlabelled utterances, equals the numpy restatement
    (tests/nnom_eval_ref.py) applied to what the flow's own call returns;
  * refusals.
"""
import ctypes
import os

import numpy as np
import pytest

import nnom_eval_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
NS = (1, 63, 64, 65, 257, 5000)
N_OUTS = (1, 2, 10, 64, 65, 256)
RULES = ("nnom", "keras", "argmax")
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def ev(built_lib):
    from edison_amd import evaluate
    return evaluate


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pools():
    """(rule, n_out) -> (outputs [5 000, n_out], labels): made once, read only. int8: the adversarial rows of the CPU pin where it has
    that width, then random rows; float32: random and softmax-like rows with exact 0.5, ties and NaN among them. One label in eight is
    out of range (-1, n_out, INT32_MAX)."""
    golden = np.load(os.path.join(GOLDEN, "eval_golden.npz"))
    made = {}
    for n_out in N_OUTS:
        rng = np.random.default_rng(1000 + n_out)
        labels = rng.integers(0, n_out, NS[-1]).astype(np.int32)
        i8 = rng.integers(-128, 128, (NS[-1], n_out)).astype(np.int8)
        i8[1::7] = (rng.integers(-1, 2, i8[1::7].shape) * 50).astype(np.int8)            # ties
        if "out_%d" % n_out in golden:
            g, gl = golden["out_%d" % n_out], golden["labels_%d" % n_out]
            order = np.random.default_rng(7).permutation(g.shape[0])                     # every kind of row among the first 63
            i8[:g.shape[0]], labels[:g.shape[0]] = g[order], gl[order]
        f = rng.random((NS[-1], n_out)).astype(np.float32)
        f[::3] = rng.dirichlet(np.ones(n_out) * 0.3, f[::3].shape[0]).astype(np.float32)
        f[4::11] = np.float32(0.5)
        f[5::13, n_out // 2] = np.float32(0.5)
        f[6::17] = np.round(f[6::17] * 4) / 4                                            # ties between classes
        f[7::97, 0] = np.nan
        f[8::101, n_out - 1] = np.nan
        for k, bad in ((0, -1), (8, n_out), (16, INT32_MAX)):
            labels[k + 3::24] = bad
        for rule in RULES:
            made[rule, n_out] = (i8 if rule == "nnom" else f, labels)
    return made


def check(got, want, what, per_row):
    assert (got.count, got.skipped, got.correct) == (want.count, want.skipped, want.correct), what
    assert np.array_equal(got.confusion, want.confusion), what + ": confusion matrix"
    assert np.array_equal(got.top_k, want.top_k), what + ": top-k histogram"
    if per_row is not None:
        assert np.array_equal(per_row["pred"], want.pred), what + ": pred"
        assert np.array_equal(per_row["rank"], want.rank), what + ": rank"
        assert np.array_equal(_bits(per_row["prob"]), _bits(want.prob)), what + ": prob, bit for bit"


@pytest.mark.parametrize("n_out", N_OUTS)
@pytest.mark.parametrize("rule", RULES)
def test_kernel_equals_the_host_function(ctx, ev, pools, rule, n_out):
    out, labels = pools[rule, n_out]
    top_k = min(n_out, 5) + 1
    seen_skipped = 0
    evs = {mb: ev.Evaluator(ctx, rule, n_out, top_k=top_k, max_blocks=mb) for mb in (1, 2, 0)}
    try:
        for n in NS:
            want = ev.host_eval(rule, out[:n], labels[:n], top_k=top_k)
            seen_skipped += want.skipped
            for mb, e in evs.items():
                for outputs in (True, False):
                    e.reset()
                    per_row = e.add(out[:n], labels[:n], return_pred=outputs)
                    check(e.result(), want, "%s, n_out %d, n %d, max_blocks %d, outputs %s" % (rule, n_out, n, mb, outputs), per_row)
    finally:
        for e in evs.values():
            e.close()
    assert seen_skipped > 500                                                            # labels out of range were among them


def test_restatement_on_the_device_results(ctx, ev, pools):
    """The same against the numpy restatement directly (not through the host function), on the shipped width"""
    out, labels = pools["nnom", 10]
    with ev.Evaluator(ctx, "nnom", 10, top_k=3) as e:
        per_row = e.add(out[:2000], labels[:2000], return_pred=True)
        got = e.result()
    want = ref.nnom(out[:2000], labels[:2000], 3)
    assert (got.count, got.skipped, got.correct) == (want["count"], want["skipped"], want["correct"])
    assert np.array_equal(got.confusion, want["confusion"]) and np.array_equal(got.top_k, want["top_k"])
    assert np.array_equal(per_row["pred"], want["pred"]) and np.array_equal(per_row["rank"], want["rank"])
    assert np.array_equal(_bits(per_row["prob"]), _bits(want["prob"]))


@pytest.mark.parametrize("rule,n_out", [("nnom", 10), ("argmax", 65)])
def test_adds_accumulate_reset_and_result_between(ctx, ev, pools, rule, n_out):
    out, labels = pools[rule, n_out]
    whole = ev.host_eval(rule, out[:500], labels[:500], top_k=4)
    with ev.Evaluator(ctx, rule, n_out, top_k=4) as e:
        parts = []
        for a, b in ((0, 100), (100, 101), (101, 500)):
            e.add(out[a:b], labels[a:b])
            parts.append(e.result())                                                     # a result between adds: the counters go on
        check(parts[0], ev.host_eval(rule, out[:100], labels[:100], top_k=4), "after the first add", None)
        check(parts[1], ev.host_eval(rule, out[:101], labels[:101], top_k=4), "after the second add", None)
        check(parts[2], whole, "three adds of 100 / 1 / 399", None)
        check(e.result(), whole, "a second result", None)
        e.reset()
        z = e.result()
        assert (z.count, z.skipped, z.correct) == (0, 0, 0) and not z.confusion.any() and not z.top_k.any()
        e.add(out[:500], labels[:500])
        check(e.result(), whole, "one add of the 500 after a reset", None)
        e.add(np.zeros((0, n_out), out.dtype), np.zeros(0, np.int32))                    # n == 0: nothing
        check(e.result(), whole, "after an empty add", None)


@pytest.mark.parametrize("n_out,max_blocks", [(10, 1), (10, 0), (65, 0)])
def test_cells_do_not_wrap_at_65536(ctx, ev, n_out, max_blocks):
    """70 000 rows into one cell: NNoM's uint16 cell would read 4 464"""
    out = np.zeros((70000, n_out), np.int8)
    out[:, 2] = 100
    labels = np.zeros(70000, np.int32)
    with ev.Evaluator(ctx, "nnom", n_out, top_k=2, max_blocks=max_blocks) as e:
        e.add(out, labels)
        r = e.result()
    assert r.confusion[0, 2] == 70000 and int(r.confusion.sum()) == 70000 and r.count == 70000 and r.correct == 0
    assert list(r.top_k) == [0, 70000]                                                   # only class 2 is above class 0


def test_two_evaluators_give_identical_bytes(ctx, ev, pools):
    out, labels = pools["keras", 64]
    got = []
    for mb in (0, 3):
        with ev.Evaluator(ctx, "keras", 64, top_k=64, max_blocks=mb) as e:
            e.add(out, labels)
            e.add(out[:777], labels[:777])
            r = e.result()
            got.append((r.confusion.tobytes(), r.top_k.tobytes(), r.count, r.skipped, r.correct))
    assert got[0] == got[1]


def test_add_queued_behind_the_network(ctx, ev, built_lib):
    """edison_cnn_batch_dev, then edison_eval_add_i8_dev on the same stream with no synchronisation in between, on torch tensors"""
    import torch
    n = 3000
    rng = np.random.default_rng(11)
    feat = rng.integers(-128, 128, (n, 403)).astype(np.int8)
    labels = rng.integers(-1, 10, n).astype(np.int32)
    want = ev.host_eval("nnom", ctx.cnn(feat)["softmax"], labels, top_k=3)
    dev = torch.device("cuda", ctx.device)
    f, y = torch.from_numpy(feat).to(dev), torch.from_numpy(labels).to(dev)
    sm = torch.zeros((n, 10), dtype=torch.int8, device=dev)
    pred, rank = torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev)
    prob = torch.zeros(n, dtype=torch.float32, device=dev)
    ctx.use_torch_stream()
    try:
        with ctx.evaluator(top_k=3) as e:                                                # defaults from the loaded graph: "nnom", 10 classes
            assert (e.rule, e.n_classes) == (0, 10)
            ctx.cnn_t(f, n, softmax=sm)
            e.add_t(sm, y, pred=pred, prob=prob, rank=rank)
            got = e.result()
    finally:
        ctx.use_own_stream()
    check(got, want, "add behind cnn_t", dict(pred=pred.cpu().numpy().view(np.uint32), prob=prob.cpu().numpy(), rank=rank.cpu().numpy()))
    assert want.skipped > 100 and want.count > 2000


# ------------------------------------------------------------------------------------------------------------------------ end to end
E2E_LABELS = np.array([3, -1, 0, 9, -1, 5, 2, 1], np.int32)


def _e2e(c, ev, audio, flow, last, rule, n_out, **flow_args):
    labels = E2E_LABELS % n_out
    labels[E2E_LABELS < 0] = -1
    want = (ref.nnom if rule == "nnom" else ref.keras if rule == "keras" else ref.argmax)(last, labels, 3)
    got = c.evaluate(audio, labels, flow=flow, chunk=3, top_k=3, return_pred=True, rule=None if rule in ("nnom", "keras") else rule, **flow_args)
    assert (got.count, got.skipped, got.correct) == (want["count"], want["skipped"], want["correct"]) and got.count == 6 and got.skipped == 2
    assert np.array_equal(got.confusion, want["confusion"]) and np.array_equal(got.top_k, want["top_k"])
    assert np.array_equal(got.pred, want["pred"]) and np.array_equal(got.rank, want["rank"]) and np.array_equal(_bits(got.prob), _bits(want["prob"]))
    return got


def _noise(n, samples, seed):
    rng = np.random.default_rng(seed)
    return np.clip(rng.normal(0, 3000, (n, samples)), -32768, 32767).astype(np.int16)


def test_evaluate_kws(ctx, ev):
    import torch
    audio = _noise(8, 32000, 21)
    for q15 in (False, True):
        got = _e2e(ctx, ev, audio, "kws", ctx.kws(audio.reshape(-1), n_utt=8, q15=q15)["softmax"], "nnom", 10, q15=q15)
        assert "Test frames: 6\n" in got.summary()
    # device-resident audio read in place, one-hot labels, no per-utterance array asked for
    labels = np.abs(E2E_LABELS)
    a = torch.from_numpy(audio.reshape(-1)).to(torch.device("cuda", ctx.device))
    whole = ctx.evaluate(a, np.eye(10)[labels], flow="kws", chunk=5, top_k=3)
    want = ref.nnom(ctx.kws(audio.reshape(-1), n_utt=8)["softmax"], labels, 3)
    assert whole.pred is None and whole.prob is None and whole.rank is None and (whole.count, whole.skipped) == (8, 0)
    assert np.array_equal(whole.confusion, want["confusion"]) and np.array_equal(whole.top_k, want["top_k"]) and whole.correct == want["correct"]


def test_evaluate_kws_geom(built_lib, ev):
    import geom_sweep as gs
    from edison_amd.context import Context
    g = gs.geometry("fs8k", net_input_scale=0.25)
    audio = _noise(8, g.n_samples, 22)
    c = Context(0, model_path=None)
    try:
        c.load_model_bytes(gs.dense_graph(g, seed=3, n_out=4))
        r = c.kws_geom(audio, g)
        assert r["softmax"] is None and len(np.unique(r["logits"])) > 2
        _e2e(c, ev, audio, "kws_geom", r["logits"], "nnom", 4, geometry=g)
    finally:
        c.close()


def test_evaluate_kws_f32(built_lib, ev):
    import test_gpu_nnom_kws as nk
    c, m = nk._open(nk.blob_kws())
    try:
        audio = nk._audio(8 * nk.UTT, 5).reshape(8, nk.UTT)
        r = c.kws_f32(m, audio, n_utt=8, utt_stride=nk.UTT, hop=nk.HOP)
        last = r["softmax"] if r["softmax"] is not None else r["logits"]
        _e2e(c, ev, audio, "kws_f32", last, "nnom", nk.N_OUT, mfcc=m, hop=nk.HOP)
    finally:
        m.close()
        c.close()


def test_evaluate_kws_float(built_lib, ev):
    from edison_amd.context import Context
    cube = np.load(os.path.join(GOLDEN, "cube_golden.npz"))
    audio = np.concatenate([np.stack([cube["audio_" + s] for s in ("edison", "hey", "noise0", "noise1", "noise2")]), _noise(3, 32000, 23)])
    c = Context(0)
    try:
        c.fnet_load(os.path.join(GOLDEN, "cube_kws.ednf"))
        probs = c.kws_float(audio)["probs"]
        _e2e(c, ev, audio, "kws_float", probs, "keras", 10)
        _e2e(c, ev, audio, "kws_float", probs, "argmax", 10)
        firmware = c.kws_float(audio, q15=True)["probs"]
        _e2e(c, ev, audio, "kws_float", firmware, "keras", 10, q15=True)
        with c.evaluator(rule="keras") as e:                                             # defaults from the float network
            assert e.n_classes == 10 and e.is_float
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx, ev, built_lib):
    from edison_amd import _lib
    for kw in (dict(n_classes=0), dict(n_classes=257), dict(n_classes=10, top_k=-1), dict(n_classes=10, max_blocks=-1), dict(n_classes=10, rule=3)):
        args = dict(rule="nnom", top_k=2)
        args.update(kw)
        with pytest.raises(_lib.EdisonError) as err:
            ev.Evaluator(ctx, args.pop("rule"), args.pop("n_classes"), **args)
        assert err.value.code == _lib.E_ARGUMENT and "edison_eval_create" in str(err.value)
    ev.Evaluator(ctx, "nnom", 256, top_k=0).close()
    with ev.Evaluator(ctx, "nnom", 1, top_k=300) as e:                                   # top_k above n_classes is allowed
        assert e.result().top_k.shape == (300,)
    i8, f32, lab = np.zeros((4, 10), np.int8), np.zeros((4, 10), np.float32), np.zeros(4, np.int32)
    L = built_lib
    with ev.Evaluator(ctx, "keras", 10) as fe, ev.Evaluator(ctx, "nnom", 10) as ie:
        for fn, h, x in ((L.edison_eval_add_i8, fe._h, i8), (L.edison_eval_add_f32, ie._h, f32)):
            assert fn(h, x.ctypes.data, lab.ctypes.data, 4, None, None, None) == _lib.E_ARGUMENT
            assert b"rule takes" in L.edison_last_error(ctx._h)
        assert L.edison_eval_add_i8_dev(fe._h, None, None, 4, None, None, None) == _lib.E_ARGUMENT
        assert L.edison_eval_add_i8(ie._h, None, lab.ctypes.data, 4, None, None, None) == _lib.E_ARGUMENT
        assert L.edison_eval_add_i8(ie._h, i8.ctypes.data, lab.ctypes.data, -1, None, None, None) == _lib.E_ARGUMENT
        assert L.edison_eval_add_i8(ie._h, None, None, 0, None, None, None) == 0
        for e in (fe, ie):
            r = e.result()
            assert r.count == 0 and r.skipped == 0 and not r.confusion.any()
    assert L.edison_eval_add_i8_dev(None, None, None, 0, None, None, None) == _lib.E_ARGUMENT and L.edison_eval_reset(None) == _lib.E_ARGUMENT
    assert L.edison_eval_result(None, None, None, None) == _lib.E_ARGUMENT
    with pytest.raises(ValueError):
        ctx.evaluate(np.zeros(100, np.int16), [0], flow="kws")                           # audio too short
    with pytest.raises(ValueError):
        ctx.evaluate(np.zeros(32000, np.int16), [0], flow="nosuch")

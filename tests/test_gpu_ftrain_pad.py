"""GPU tests (-m gpu) of training padded float32 networks (edison_ftrain_create_ex with EDISON_FTRAIN_PADDED, Context.trainer(padded=True),
kws train; DESIGN.md sections 14b and 19) against tests/ftrain_ref.py, the float64 restatement, with pads.

The bounds are tests/test_gpu_ftrain.py's, measured the same way: per tensor max |g - g64| / max |g64|, allowed 4 x the same error of
torch's CPU float32 autograd, floored at 8 x 2^-24 x sqrt(terms), terms = n x the record's live rows. tests/test_fgrad_pad_cpu.py shows
the precondition on the very inputs used here: float32 and float64 choose the same pool winners and ReLU signs.

Every network is loaded with 1e6 in all its weight padding (test_gpu_ftrain.poisoned)."""
import hashlib
import io
import struct

import numpy as np
import pytest

import fnet_host
import fnet_plan
import fnet_rows
import ftrain_ref
import ftrain_rows
import test_gpu_ftrain as gt
from edison_amd import _lib, cube_import, train

pytestmark = pytest.mark.gpu

EPS = gt.EPS
ALL_N = ftrain_rows.ALL_N                                         # rows that run n over {1, b - 1, b, b + 1, 3 b + 2}
LOWERED = {"mid_pads_batch": 5, "simple_conv": 6}        # tests/test_fgrad_pad_cpu.py: rows that train below their forward batch


@pytest.fixture(scope="module")
def ctx(built_lib):
    from edison_amd.context import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh(built_lib):
    from edison_amd.context import Context
    c = Context(0)
    yield c
    c.close()


_CASES = {}


def case(name):
    """(model, blob with poisoned padding, mask of the packed array's real entries) of a row of ftrain_rows.PAD_ROWS, built once."""
    if name not in _CASES:
        bad, real = gt.poisoned(ftrain_rows.pad_blob(name))
        _CASES[name] = (ftrain_rows.pad_model(name), bad, real)
    return _CASES[name]


def check_plan(blob, info):
    p = fnet_plan.plan(blob)
    assert info["batch"] == ftrain_ref.train_batch(p) and info["lds_bytes"] == ftrain_ref.train_lds_bytes(p, info["batch"]), (info, p["batch"])
    return p


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_call(ctx, tr, name, model, real, x, y, w0):
    """One host-form gradient call held in every way: logits and argmax edison_fnet_batch's bits, loss and every tensor by the float64
    bounds, padding +0.0f, a repeat the same bits, nothing else moved. Returns the packed gradient."""
    n = len(y)
    ref = ftrain_ref.loss_grad(model, x, y)
    before = ctx.fnet(x)
    r = tr.grad(x, y)
    assert same_bits(tr.logits(n), before["logits"]), (name, n)
    assert np.array_equal(r["argmax"], before["argmax"])
    lb, le = ftrain_ref.bounds(model, x, y, ref)[1]
    lerr = ftrain_ref.tensor_error(r["loss"], ref["loss"])
    print("%s n=%d loss: gpu %.3g  e32 %.3g  bound %.3g" % (name, n, lerr, le, lb))
    assert lerr <= lb, (name, n, lerr, lb)
    gt.check_gradient(name, tr, model, real, x, y, ref)
    g = tr.gradient()
    r2 = tr.grad(x, y)
    assert same_bits(tr.gradient(), g), (name, n)
    assert same_bits(r2["loss"], r["loss"]) and same_bits(tr.logits(n), before["logits"])
    assert same_bits(tr.packed_weights(), w0)
    after = ctx.fnet(x)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    return g


@pytest.mark.parametrize("name", ftrain_rows.PAD_ROWS)
def test_logits_loss_gradient_padding_repeat_and_no_side_effect(ctx, name):
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    with ctx.trainer(padded=True) as tr:
        info = tr.info()
        b = info["batch"]
        assert info["w_floats"] == len(real) and info["lds_bytes"] <= 160 * 1024 and info["grid"] >= 1 and info["steps"] == 0
        p = check_plan(blob, info)
        assert b == LOWERED.get(name, p["batch"]), (name, b, p["batch"])
        assert any(L["pad"] for L in p["layers"])
        if name == "mid_pads_batch":                                        # a mixed network: the kernel runs both instantiations of the tile
            assert [L["pad"] for L in p["layers"]] == [False, True, True, False] and ("pad_layer", 1) in fnet_rows.pad_facts(name)
        ns = sorted({ftrain_rows.N_ROWS} | ({1, max(b - 1, 1), b, b + 1, 3 * b + 2} if name in ALL_N else set()))
        assert max(ns) <= ftrain_rows.n_max(name)                                    # the rows the CPU test holds the precondition on
        xs, ys = ftrain_rows.pad_data(name, max(ns))
        if name == ftrain_rows.NEG_T:
            assert (xs < 0).all()
        w0 = tr.packed_weights()
        for n in ns:
            check_call(ctx, tr, name, model, real, xs[:n], ys[:n], w0)


@pytest.mark.parametrize("pool", ftrain_ref.TIE_PADS, ids=lambda p: "pool%d%d" % p)
def test_tied_pool_windows_send_the_gradient_to_their_first_present_element(ctx, pool):
    """ftrain_ref.tie_case with pool pads: windows with absent elements leading and trailing whose present elements tie exactly
    (tests/test_fgrad_pad_cpu.py shows that another choice moves dW by more than 1e-2 of its largest entry)."""
    model, x, y = ftrain_ref.tie_case(pool, ppad=ftrain_ref.TIE_PADS[pool])
    name = "tie_pad_pool%d%d" % tuple(pool)
    blob, real = gt.poisoned(cube_import.build_blob(model))
    ctx.fnet_load(blob)
    with ctx.trainer(padded=True) as tr:
        assert tr.info()["batch"] < len(y)                                  # more than one tile
        check_plan(blob, tr.info())
        check_call(ctx, tr, name, model, real, x, y, tr.packed_weights())


def pow2_at_least(v):
    return 1 << max(int(v) - 1, 0).bit_length()


def test_a_multi_tile_gradient_is_the_fold_of_its_tiles_exactly(ctx):
    """The method of tests/test_gpu_ftrain_tiles.py on sym3x3: N = 2 x grid x batch rounded up to a power of two, N(0, 1) inputs; every
    tile alone among fillers labelled -1 gives its term of the big call times N / n', exactly; the big call's gradient is
    ftrain_ref.fold_tiles of those terms, element for element."""
    import torch
    name = "sym3x3"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    with ctx.trainer(padded=True) as tr:
        info = tr.info()
        b, G, w = info["batch"], info["grid"], info["w_floats"]
        N = pow2_at_least(2 * G * b)
        n1 = pow2_at_least(b)
        n_tiles = (N + b - 1) // b
        assert n_tiles >= 2 * G and n1 <= G * b and N >= 2 * n1
        rng = np.random.default_rng(586 + sum(map(ord, name)))
        x = rng.normal(0, 1, (N + n1, int(np.prod(model["in_shape"])))).astype(np.float32)
        y = (np.arange(N + n1) % tr.n_out).astype(np.int32)
        w0 = tr.packed_weights()
        big = check_call(ctx, tr, name, model, real, x[:N], y[:N], w0)
        labels = np.full((n_tiles, n1), -1, np.int32)
        for j in range(n_tiles):
            own = y[j * b:min((j + 1) * b, N)]
            labels[j, :len(own)] = own
        fillers = int((labels < 0).sum())
        dev = torch.device("cuda", 0)
        xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev)
        torch.cuda.synchronize()
        ignored0 = tr.info()["ignored"]
        T = np.empty((n_tiles, w), np.float32)
        smallest, digests = np.inf, set()
        for j in range(n_tiles):
            tr.grad_t(xt[j * b:j * b + n1], yt[j], n1)
            T[j] = tr.gradient()
            nz = np.abs(T[j][T[j] != 0])
            smallest = min(smallest, float(nz.min()) if nz.size else np.inf)
            digests.add(hashlib.blake2b(T[j].tobytes(), digest_size=16).digest())
        assert tr.info()["ignored"] - ignored0 == fillers == n_tiles * n1 - N
        scale = n1 / N
        print("%s: batch %d, grid %d, N %d, %d tiles, small calls of %d rows, smallest term %.3g x %g" % (name, b, G, N, n_tiles, n1, smallest, scale))
        assert len(digests) == n_tiles, "two tiles give the same gradient: a swapped order would not show"
        assert np.isfinite(T).all() and smallest * scale > 2.0 ** -100
        assert not T[:, ~real].view(np.uint32).any()
        want = ftrain_ref.fold_tiles(T, G, scale)
        diff = np.flatnonzero(~(want == big))
        assert diff.size == 0, "%s: %d of %d gradient entries are not the fold of the tiles' (first at %d: call %r, fold %r)" % (
            name, diff.size, w, diff[0], big[diff[0]], want[diff[0]])
        assert not big[~real].view(np.uint32).any()
        assert same_bits(tr.packed_weights(), w0)


def test_adam_steps_in_place_and_the_exported_network(ctx, fresh):
    name = "medium_embedding_conv"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    x, y = ftrain_rows.pad_data(name)
    lr = 0.01
    with ctx.trainer(padded=True) as tr:
        adam = ftrain_ref.Adam()
        for step in range(3):
            w_before = tr.packed_weights().astype(np.float64)
            tr.grad(x, y)
            g = tr.gradient().astype(np.float64)
            tr.step(lr)
            want = [w_before.copy()]
            adam.step(want, [g], lr)
            got = tr.packed_weights()
            err = gt.step_errors(tr, real, got, want[0])
            print("step %d: %.3g (bound %.3g)" % (step + 1, err.max(), 4 * EPS))
            assert err.max() <= 4 * EPS, (step, int(err.argmax()), err.max())
            assert (got[~real] == np.float32(1.0e6)).all()
            assert np.abs(got[real] - w_before[real]).max() > 0.5 * lr * 0.9
        assert tr.info()["steps"] == 3
        new = ctx.fnet(x)
        exported = cube_import.build_blob(tr.model())
        assert struct.unpack_from("<i", exported, 4)[0] == 2                # a version-2 blob ...
        back = cube_import.read_blob(exported)
        assert [fnet_host.pads(L) for L in train.conv_records(back)] == [fnet_host.pads(L) for L in train.conv_records(model)]   # ... with the pads
        assert any(any(c) or any(q) for c, q in map(fnet_host.pads, train.conv_records(back)))
        fresh.fnet_load(exported)
        again = fresh.fnet(x)
        assert same_bits(new["logits"], again["logits"])
        assert not np.array_equal(new["logits"], gt.fnet_logits_of(fresh, blob, x))
        assert tr.export() == cube_import.build_blob(tr.model(), tr.model().get("keywords"))


def test_fit_learns_the_synthetic_set(ctx):
    """40 Adam steps at batch 32, lr 0.01, seed 0 on three noisy class patterns at stride2_same's input shape: the train loss falls
    below half its first value and the accuracy reaches 0.9 (the float64 replay meets both with room: tests/test_fgrad_pad_cpu.py), and
    the last loss is the replay's."""
    x, y = ftrain_rows.pad_fit_set()
    model = ftrain_rows.pad_model(ftrain_rows.PAD_FIT_ROW)
    blob, _ = gt.poisoned(fnet_rows.blob(ftrain_rows.PAD_FIT_ROW))
    ctx.fnet_load(blob)
    kw = dict(epochs=100, batch_size=ftrain_rows.FIT_BATCH, seed=0, lr=ftrain_rows.FIT_LR, max_steps=ftrain_rows.FIT_STEPS)
    with ctx.trainer(padded=True) as tr:
        hist = tr.fit(x, y, **kw)
        assert hist["steps"] == 40 and tr.info()["steps"] == 40
        acc = (ctx.fnet(x)["argmax"] == y).mean()
    replay = train.fit(ftrain_ref.HostTrainer(model), x, y, **kw)
    print("loss %.5f -> %.5f (float64 replay %.5f), accuracy %.3f" % (hist["loss"][0], hist["loss"][-1], replay["loss"][-1], acc))
    assert hist["loss"][-1] < 0.5 * hist["loss"][0] and acc >= 0.9
    assert abs(hist["loss"][-1] - replay["loss"][-1]) <= 1e-3 * replay["loss"][-1]
    assert len(hist["loss"]) == len(replay["loss"]) == 14


def test_kws_train_then_kws_quantize(ctx, tmp_path):
    """kws train on tiny_conv at 31 x 13 x 1 (a 'same' strided conv), 5 epochs, then kws quantize of what it wrote."""
    from edison_amd import config as cfg
    from edison_amd.kws import kws_quantize, kws_train
    from edison_amd.kws.geometry import KwsGeometry
    model = ftrain_rows.pad_model("tiny_conv")
    x, y = ftrain_rows.kws_set()
    keywords = ["k%d" % i for i in range(10)]
    with open(tmp_path / "net.ednf", "wb") as f:
        f.write(cube_import.build_blob(model, keywords))
    np.save(tmp_path / "x.npy", x)
    np.save(tmp_path / "y.npy", y)
    out = io.StringIO()
    blob, hist = kws_train.run(str(tmp_path / "net.ednf"), str(tmp_path / "x.npy"), str(tmp_path / "y.npy"), str(tmp_path / "out.ednf"), epochs=5,
                               batch=32, lr=0.01, val=(str(tmp_path / "x.npy"), str(tmp_path / "y.npy")), ctx=ctx, out=out)
    assert (tmp_path / "out.ednf").read_bytes() == blob and hist["steps"] == 15 and len(hist["val_loss"]) == 5
    assert "epoch   5" in out.getvalue() and "after 15 steps" in out.getvalue()
    assert hist["loss"][-1] < hist["loss"][0]
    trained = cube_import.read_blob(blob)
    assert trained["keywords"] == keywords and struct.unpack_from("<i", blob, 4)[0] == 2
    assert [fnet_host.pads(L) for L in train.conv_records(trained)] == [fnet_host.pads(L) for L in train.conv_records(model)]
    assert not np.array_equal(train.conv_records(trained)[0]["w"], train.conv_records(model)[0]["w"])
    assert np.array_equal(ctx.fnet(x)["logits"], gt.fnet_logits_of(ctx, blob, x))      # the context ran the trained weights already
    g = KwsGeometry.from_config(net_input_scale=cfg.net_input_scale)
    assert g.n_features == 403
    rng = np.random.default_rng(8)
    np.save(tmp_path / "audio.npy", np.clip(rng.normal(0, 3000, (6, g.n_samples)), -32768, 32767).astype(np.int16))
    qblob, rep = kws_quantize.run(str(tmp_path / "out.ednf"), str(tmp_path / "audio.npy"), str(tmp_path / "q.ednn"), ctx=ctx, out=io.StringIO())
    assert (tmp_path / "q.ednn").read_bytes() == qblob and len(rep["float_argmax"]) == 6


def test_refusals_and_the_flag_on_an_unpadded_network(ctx):
    import ctypes
    ctx.fnet_load(fnet_rows.blob("sym3x3"))
    h = ctypes.c_void_p()
    for flags in (2, 3, 0x80000000):
        assert ctx._L.edison_ftrain_create_ex(ctx._h, flags, ctypes.byref(h)) == _lib.E_ARGUMENT and not h.value
    with pytest.raises(_lib.EdisonError) as e:                              # the plain call keeps its refusal, word for word
        ctx.trainer()
    assert e.value.code == _lib.E_NO_IMPL and "record 0" in str(e.value) and "pad" in str(e.value)
    assert "edison_ftrain_create: record 0 has a conv or pool pad; training runs networks without pads" in str(e.value)
    with pytest.raises(_lib.EdisonError) as e:
        ctx.trainer(padded=False)
    assert e.value.code == _lib.E_NO_IMPL
    # on a network without pads the flag changes nothing: one gradient call, the same bits and the same plan
    name = "pool21_trunc_h"
    model, blob, real = gt.case(name)
    ctx.fnet_load(blob)
    x, y = gt.data(name, model, 19)
    with ctx.trainer() as plain:
        r0 = plain.grad(x, y)
        g0, z0, i0 = plain.gradient(), plain.logits(19), plain.info()
    with ctx.trainer(padded=True) as flagged:
        r1 = flagged.grad(x, y)
        assert same_bits(flagged.gradient(), g0) and same_bits(flagged.logits(19), z0) and same_bits(r1["loss"], r0["loss"])
        assert np.array_equal(r1["argmax"], r0["argmax"]) and flagged.info() == i0
        assert g0[real].any()

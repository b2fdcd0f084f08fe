"""GPU tests (-m gpu) of training padded float32 networks (edison_ftrain_create_ex with EDISON_FTRAIN_PADDED, Context.trainer(padded=True),
kws train; DESIGN.md sections 14b and 19) against tests/ftrain_ref.py, the float64 restatement, with pads.

The bounds are tests/test_gpu_ftrain.py's, measured the same way: per tensor max |g - g64| / max |g64|, allowed 4 x the same error of
torch's CPU float32 autograd, floored at 8 x 2^-24 x sqrt(terms), terms = n x the record's live rows. tests/test_fgrad_pad_cpu.py shows
the precondition on the very inputs used here: float32 and float64 choose the same pool winners and ReLU signs.

Every network is loaded with 1e6 in all its weight padding (ftrain_drive.poisoned); the machinery is tests/ftrain_drive.py's."""
import struct

import numpy as np
import pytest

import fnet_host
import fnet_rows
import ftrain_ref
import ftrain_rows
from edison_amd import _lib, cube_import, train
from ftrain_drive import (EPS, case, check_call, check_fit_learns, check_fold, check_plan, data, fnet_logits_of, kws_files, kws_quantized, kws_trained, own_context,
                          poisoned, same_bits, step_checked)

pytestmark = pytest.mark.gpu

ALL_N = ftrain_rows.ALL_N                                         # rows that run n over {1, b - 1, b, b + 1, 3 b + 2}
LOWERED = {"mid_pads_batch": 5, "simple_conv": 6}        # tests/test_fgrad_pad_cpu.py: rows that train below their forward batch


@pytest.fixture(scope="module")
def ctx(built_lib):
    yield from own_context()


@pytest.fixture(scope="module")
def fresh(built_lib):
    yield from own_context()


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
    blob, real = poisoned(cube_import.build_blob(model))
    ctx.fnet_load(blob)
    with ctx.trainer(padded=True) as tr:
        assert tr.info()["batch"] < len(y)                                  # more than one tile
        check_plan(blob, tr.info())
        check_call(ctx, tr, name, model, real, x, y, tr.packed_weights())


def test_a_multi_tile_gradient_is_the_fold_of_its_tiles_exactly(ctx):
    """The method of tests/test_gpu_ftrain_tiles.py on sym3x3: N = 2 x grid x batch rounded up to a power of two, N(0, 1) inputs; every
    tile alone among fillers labelled -1 gives its term of the big call times N / n', exactly; the big call's gradient is
    ftrain_ref.fold_tiles of those terms, element for element."""
    name = "sym3x3"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    with ctx.trainer(padded=True) as tr:
        check_fold(ctx, tr, name, model, real, 2)


def test_adam_steps_in_place_and_the_exported_network(ctx, fresh):
    name = "medium_embedding_conv"
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    x, y = ftrain_rows.pad_data(name)
    lr = 0.01
    with ctx.trainer(padded=True) as tr:
        adam = ftrain_ref.Adam()
        for step in range(3):
            s = step_checked(tr, real, x, y, [adam], lr, "step %d" % (step + 1))
            print("step %d: %.3g (bound %.3g)" % (step + 1, s.errs[0].max(), 4 * EPS))
            assert np.abs(s.got[real] - s.before.astype(np.float64)[real]).max() > 0.5 * lr * 0.9
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
        assert not np.array_equal(new["logits"], fnet_logits_of(fresh, blob, x))
        assert tr.export() == cube_import.build_blob(tr.model(), tr.model().get("keywords"))


def test_fit_learns_the_synthetic_set(ctx):
    """40 Adam steps at batch 32, lr 0.01, seed 0 on three noisy class patterns at stride2_same's input shape: the train loss falls
    below half its first value and the accuracy reaches 0.9 (the float64 replay meets both with room: tests/test_fgrad_pad_cpu.py), and
    the last loss is the replay's."""
    x, y = ftrain_rows.pad_fit_set()
    model = ftrain_rows.pad_model(ftrain_rows.PAD_FIT_ROW)
    check_fit_learns(ctx, dict(padded=True), model, poisoned(fnet_rows.blob(ftrain_rows.PAD_FIT_ROW))[0], x, y)


def test_kws_train_then_kws_quantize(ctx, tmp_path):
    """kws train on tiny_conv at 31 x 13 x 1 (a 'same' strided conv), 5 epochs, then kws quantize of what it wrote."""
    from edison_amd import config as cfg
    from edison_amd.kws.geometry import KwsGeometry
    model = ftrain_rows.pad_model("tiny_conv")
    x, y = ftrain_rows.kws_set()
    keywords = ["k%d" % i for i in range(10)]
    args, val = kws_files(tmp_path, model, x, y, keywords)
    blob, hist, text, trained = kws_trained(ctx, tmp_path, args, val)
    assert "epoch   5" in text
    assert hist["loss"][-1] < hist["loss"][0]
    assert trained["keywords"] == keywords and struct.unpack_from("<i", blob, 4)[0] == 2
    assert [fnet_host.pads(L) for L in train.conv_records(trained)] == [fnet_host.pads(L) for L in train.conv_records(model)]
    assert not np.array_equal(train.conv_records(trained)[0]["w"], train.conv_records(model)[0]["w"])
    assert np.array_equal(ctx.fnet(x)["logits"], fnet_logits_of(ctx, blob, x))      # the context ran the trained weights already
    assert KwsGeometry.from_config(net_input_scale=cfg.net_input_scale).n_features == 403
    kws_quantized(ctx, tmp_path)


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
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    x, y = data(name, model, 19)
    with ctx.trainer() as plain:
        r0 = plain.grad(x, y)
        g0, z0, i0 = plain.gradient(), plain.logits(19), plain.info()
    with ctx.trainer(padded=True) as flagged:
        r1 = flagged.grad(x, y)
        assert same_bits(flagged.gradient(), g0) and same_bits(flagged.logits(19), z0) and same_bits(r1["loss"], r0["loss"])
        assert np.array_equal(r1["argmax"], r0["argmax"]) and flagged.info() == i0
        assert g0[real].any()

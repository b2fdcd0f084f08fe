"""GPU tests (-m gpu) of float32 networks whose layers exceed the LDS (edison_fnet_load_ex, the layer road). The
rows, their inputs and the restated tiling are tests/fnet_rows.py's; the reference is tests/fnet_host.py's bit-exact host model of the
k-ordered fmaf chain, which the layer road must give bit for bit, as the one-launch kernel does.

  every row at every utterance count, and in three chunks under a capped workspace: logits and every layer bit-equal to the host model;
    probs within 1e-6 of the float64 softmax of the kernel's logits; argmax the first maximum of the kernel's probs, and the float64
    chain's wherever its top-2 margin exceeds MARGIN (test_gpu_fnet.py's rules); the same call twice gives the same bits
  the full-size conv_model and low_latency_conv: logits bit-equal to the host model
  layered=True on networks that fit: every output bit-identical to the one-launch kernel's
  large=True on a network that fits: the plain load's plan and outputs; flags 0 on an over-LDS row: today's refusal
  kws_float and evaluate(flow="kws_float") on a layered network
  the consumers that cannot run a layered network refuse it by name; bad flags; a workspace cap below one utterance"""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from geom_sweep import geom
from stream_drive import recordings

import fnet_host as fh
import fnet_plan as fpl
import fnet_rows as fr
from edison_amd import cube_import, train

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "cube_kws.ednf")
MARGIN = 1e-3
# 8 frames of 6 coefficients: the input of fnet_rows.LARGE's conv_model row
SMALL = dict(variant="B", frame_len=512, frame_step=256, n_samples=512 + 7 * 256, mel_nbins=16, first_mfcc=0, num_mfcc=6)


@pytest.fixture(scope="module")
def ctx(built_lib):
    from edison_amd.context import Context
    c = Context(0)
    yield c
    c.close()


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    v = (lambda a: a.view(np.uint32)) if got.dtype == np.float32 else (lambda a: a)
    diff = v(got) != v(want)
    assert not diff.any(), "%s: %d of %d differ (first at %s: got %r, want %r)" % (what, int(diff.sum()), got.size, np.argwhere(diff)[0], got[diff][0],
                                                                                  want[diff][0])


_REF = {}


def _ref(name):
    """(inputs, the host model's layers, the float64 chain's logits) of row `name` at the largest utterance count; computed once."""
    if name not in _REF:
        x = fr.inputs(name, max(fr.NS))
        _REF[name] = (x, fh.run(fr.model(name), x), fh.run64(fr.model(name), x)["logits"])
    return _REF[name]


def _check_row(ctx, name, n, what):
    m = fr.model(name)
    x, want, z64 = (a[:n] if isinstance(a, np.ndarray) else [w[:n] for w in a] for a in _ref(name))
    r = ctx.fnet(x)
    _same(r["logits"], want[-1], "%s %s logits" % (name, what))
    acts = ctx.fnet_layers(x)
    model_layers, got = fh.layers_from(m, x, acts)
    for i, (w, g) in enumerate(zip(model_layers, got)):
        _same(g, w, "%s %s layer %d" % (name, what, i))
    assert np.abs(r["probs"] - fh.softmax(r["logits"].astype(np.float64))).max() <= 1e-6
    assert np.array_equal(r["argmax"], np.argmax(r["probs"], axis=1))
    top = np.sort(z64, axis=1)
    clear = top[:, -1] - top[:, -2] > MARGIN
    assert np.array_equal(r["argmax"][clear], np.argmax(fh.softmax(z64), axis=1)[clear])
    again = ctx.fnet(x)
    for k in r:
        _same(again[k], r[k], "%s %s the same call again: %s" % (name, what, k))
    _same(ctx.fnet_layers(x), acts, "%s %s the same call again: acts" % (name, what))


@pytest.mark.parametrize("name", list(fr.LARGE))
def test_row_bit_exact(ctx, name):
    p = fr.plan_of(name, large=True)
    layers = p["layers"]
    ctx.fnet_load(fr.blob(name), large=True)
    info = ctx.fnet_info()
    assert (info["layered"], info["batch"], info["lds_bytes"], info["n_layers"], info["acts_floats"], info["n_out"]) == \
        (True, 0, fpl.LAYER_LDS_BYTES, len(layers), sum(L["out_n"] for L in layers), layers[-1]["out_n"])
    for n in fr.NS:
        _check_row(ctx, name, n, "n = %d" % n)
    ctx.fnet_workspace(fpl.cap_for(p, fr.CHUNK))
    try:
        assert fpl.launches(p, fr.N_CHUNKED, fpl.cap_for(p, fr.CHUNK)) == 3 * (len(layers) + 1)
        _check_row(ctx, name, fr.N_CHUNKED, "in chunks of %d" % fr.CHUNK)
    finally:
        ctx.fnet_workspace(0)


@pytest.mark.parametrize("arch", ["conv_model", "low_latency_conv"])
def test_full_size_architectures(ctx, arch):
    """train.get_model's two architectures the one-launch kernel cannot hold, at the shipped 31x13x1 input and 10 classes."""
    m = train.get_model(arch, (31, 13, 1), 10, seed=3)
    blob = cube_import.build_blob(m)
    assert fpl.plan(blob) == dict(error=fpl.E_NO_IMPL)      # both meet a record over the LDS first: 2560 x 64, and 248 x 192
    ctx.fnet_load(blob, large=True)
    assert ctx.fnet_info()["layered"]
    x = fr.inputs("sym3x3", 3, 403)
    _same(ctx.fnet(x)["logits"], fh.run(m, x)[-1], arch + " logits")


def _fitting():
    """(name, blob, inputs) of networks that fit: the fixture, and sweep rows of both instantiations at P = 1, 2 and 4."""
    rng = np.random.default_rng(11)
    yield "fixture", open(FIXTURE, "rb").read(), (60 * rng.normal(0, 1, (37, 403))).astype(np.float32)
    for name in ("pool21_trunc_h", "pool22_trunc_hw", "inc3_oc64_oc65_s21", "n_out_210", "subnormal"):
        p = fpl.plan(fr.blob(name))
        yield name, fr.blob(name), fr.inputs(name, 2 * p["batch"] + 1, p["in_n"])
    for name in ("sym3x3", "pool21_tail", "pool22_odd", "oc65_pad", "mid_pads_batch"):
        p = fpl.plan(fr.blob(name))
        yield name, fr.blob(name), fr.inputs(name, 2 * p["batch"] + 1, p["in_n"])


def test_fitting_rows_cover_both_instantiations():
    seen = set()
    for name in ("pool21_trunc_h", "pool22_trunc_hw", "inc3_oc64_oc65_s21"):
        seen |= {(False, L["P"]) for L in fpl.plan(fr.blob(name))["layers"]}
    for name in ("sym3x3", "pool21_tail", "pool22_odd"):
        seen |= {(True, L["P"]) for L in fpl.plan(fr.blob(name))["layers"] if L["pad"]}
    assert seen >= {(pad, P) for pad in (False, True) for P in (1, 2, 4)}


def test_layered_equals_the_one_launch_kernel(ctx):
    for name, blob, x in _fitting():
        ctx.fnet_load(blob)
        plain, plain_acts = ctx.fnet(x), ctx.fnet_layers(x)
        assert not ctx.fnet_info()["layered"]
        ctx.fnet_load(blob, layered=True)
        assert ctx.fnet_info()["layered"] and ctx.fnet_info()["batch"] == 0
        got = ctx.fnet(x)
        for k in plain:
            _same(got[k], plain[k], "%s layered against plain: %s" % (name, k))
        _same(ctx.fnet_layers(x), plain_acts, name + " layered against plain: acts")


def test_large_on_a_fitting_network_changes_nothing(ctx):
    from edison_amd import _lib
    for name, blob, x in list(_fitting())[:3]:
        ctx.fnet_load(blob)
        info, plain, plain_acts = ctx.fnet_info(), ctx.fnet(x), ctx.fnet_layers(x)
        ctx.fnet_load(blob, large=True)
        assert ctx.fnet_info() == info and not info["layered"] and info["batch"] >= 1
        got = ctx.fnet(x)
        for k in plain:
            _same(got[k], plain[k], "%s large against plain: %s" % (name, k))
        _same(ctx.fnet_layers(x), plain_acts, name + " large against plain: acts")
        # flags 0 on a network that does not fit: today's refusals, the loaded network answering as before
        for row, text in (("dense_over", "a layer's weights exceed the LDS"),
                          ("acts_over", "one utterance's activations and the largest layer do not fit the LDS")):
            with pytest.raises(_lib.EdisonError, match=text) as e:
                ctx.fnet_load(fr.blob(row))
            assert e.value.code == _lib.E_NO_IMPL
        _same(ctx.fnet(x)["logits"], plain["logits"], name + " after the refusals")


def test_kws_float_and_evaluate(ctx):
    g = geom(**SMALL)
    name = "conv_model"
    assert (g.frame_count, g.num_mfcc, 1) == fr.LARGE[name][0]["in_shape"]
    ctx.fnet_load(fr.blob(name), large=True)
    n = 11
    audio = recordings(g, n, g.frame_count + 1, 7)[:, :g.n_samples]
    r = ctx.kws_float(audio.ravel(), g, n_utt=n)
    f = ctx.fnet(r["feat"])
    for k in ("logits", "probs", "argmax"):
        _same(r[k], f[k], "kws_float against fnet on its features: " + k)
    _same(r["logits"], fh.run(fr.model(name), r["feat"])[-1], "kws_float logits against the host model")
    labels = (np.arange(n) * 3) % 4
    ctx.fnet_workspace(fpl.cap_for(fr.plan_of(name, large=True), 2))           # evaluate's chunks of 4 utterances run in two chunks of the road each
    try:
        keras = ctx.evaluate(audio, labels, flow="kws_float", chunk=4, top_k=2, return_pred=True, geometry=g)
        first = ctx.evaluate(audio, labels, flow="kws_float", chunk=4, top_k=2, return_pred=True, geometry=g, rule="argmax")
    finally:
        ctx.fnet_workspace(0)
    # the host count: the float flow's default rule is the reference's (the first class above 0.5, else class 0), "argmax" the first maximum
    over = r["probs"] > np.float32(0.5)
    for got, pred in ((keras, np.where(over.any(axis=1), over.argmax(axis=1), 0)), (first, r["argmax"])):
        want = np.zeros((4, 4), np.uint64)
        np.add.at(want, (labels, pred), 1)
        assert np.array_equal(got.confusion, want) and got.count == n and got.skipped == 0
        assert np.array_equal(got.pred, pred)
        _same(got.prob, r["probs"][np.arange(n), pred], "evaluate's probabilities")


def test_consumers_refuse_a_layered_network_by_name(ctx):
    from edison_amd import _lib
    from edison_amd.stream import FloatBank, FloatStream
    g = geom(**SMALL)
    name = "conv_model"
    ctx.fnet_load(fr.blob(name), large=True)
    x = fr.inputs(name, 5)
    before, acts = ctx.fnet(x), ctx.fnet_layers(x)
    for what, create in (("calibrator", ctx.calibrator), ("trainer", ctx.trainer), ("padded trainer", lambda: ctx.trainer(padded=True)),
                         ("float stream", lambda: FloatStream(ctx, g)), ("float bank", lambda: FloatBank(ctx, 3, g))):
        with pytest.raises(_lib.EdisonError, match="layer road") as e:
            create()
        assert e.value.code == _lib.E_NO_IMPL, what
        after = ctx.fnet(x)
        for k in before:
            _same(after[k], before[k], "after the %s's refusal: %s" % (what, k))
        _same(ctx.fnet_layers(x), acts, "after the %s's refusal: acts" % what)


def test_bad_flags_and_workspace(ctx):
    from edison_amd import _lib
    name = "mixed"
    p, blob = fr.plan_of(name, large=True), fr.blob(name)
    ctx.fnet_load(blob, large=True)
    x = fr.inputs(name, 5)
    before = ctx.fnet(x)
    buf = ctypes.create_string_buffer(blob, len(blob))
    for flags in (4, 8 | _lib.FNET_LARGE, 0x80000000):
        assert ctx._L.edison_fnet_load_mem_ex(ctx._h, buf, len(blob), flags) == _lib.E_ARGUMENT
    # a cap below one utterance of the loaded layered network: refused, the cap stays
    with pytest.raises(_lib.EdisonError, match="workspace cap of %d bytes" % (fpl.cap_for(p, 1) - 8)) as e:
        ctx.fnet_workspace(fpl.cap_for(p, 1) - 8)
    assert e.value.code == _lib.E_NO_MEMORY
    for k in before:
        _same(ctx.fnet(x)[k], before[k], "after the refused cap: " + k)
    # a load under a cap that one utterance of the new network exceeds: refused, the previous network stays
    small, big = "dense_over", "low_latency_conv"
    cap = fpl.cap_for(fr.plan_of(small, large=True), 1)
    assert fpl.chunk_of(fr.plan_of(small, large=True), cap) == 1 and fpl.chunk_of(fr.plan_of(big, large=True), cap) == 0
    ctx.fnet_workspace(cap)
    try:
        ctx.fnet_load(fr.blob(small), large=True)
        one = ctx.fnet(fr.inputs(small, 3))
        _same(one["logits"], fh.run(fr.model(small), fr.inputs(small, 3))[-1], "one utterance per chunk")
        with pytest.raises(_lib.EdisonError, match="workspace cap of %d bytes" % cap) as e:
            ctx.fnet_load(fr.blob(big), large=True)
        assert e.value.code == _lib.E_NO_MEMORY
        _same(ctx.fnet(fr.inputs(small, 3))["logits"], one["logits"], "after the refused load")
    finally:
        ctx.fnet_load(open(FIXTURE, "rb").read())
        ctx.fnet_workspace(0)

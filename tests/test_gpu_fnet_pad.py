"""GPU tests (-m gpu) of padded float32 networks ('same' convolutions and pools, .ednf version 2). The rows,
the bit-exact host model and the float64 restatement are tests/fnet_host.py's.

Per row, at 2 batch + 1 utterances (a full tile, a second one, a tile of one):
  fnet_info = the restated version-2 plan
  every layer of fnet_layers, layer i fed the kernel's own layer i - 1: bit-equal to the host model (the k-ordered fmaf chain with +0.0f
    at the padded taps, -inf for the absent elements of a pool window) and within K_BOUND 1e-7 S of the float64 restatement
  logits = the last layer; probs within 1e-6 of the float64 softmax of the kernel's logits; argmax the first maximum of the kernel's
    probs, and the float64 chain's wherever its top-2 margin exceeds MARGIN (test_gpu_fnet.py's rules)
Then the loader's refusals, streams and the bank, the calibrator's counters, quantising to NNoM's PADDING_SAME, and the shipped
network's answers around a padded load."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from geom_sweep import geom
from stream_drive import recordings, tail

import cube_synth
import fnet_host as fh
import fnet_plan as fpl
import fnet_rows as fr
from edison_amd import cube_import
from edison_amd import quantize as qz
from oracle import net_ref

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "cube_kws.ednf")
MARGIN = 1e-3
# 10 frames of 6 coefficients: medium_embedding_conv's 8x8 stride-2 'same' conv gives a 5 x 3 map, whose 'same' pool pads both far ends
SMALL = dict(variant="B", frame_len=512, frame_step=256, n_samples=512 + 9 * 256, mel_nbins=16, first_mfcc=0, num_mfcc=6)
SMALL_IN = (10, 6, 1)


@pytest.fixture(scope="module")
def ctx(built_lib):
    from edison_amd.context import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    """(blob, model, geometry) of medium_embedding_conv at the small geometry, through the X-CUBE-AI source format and the importer."""
    g = geom(**SMALL)
    assert (g.frame_count, g.num_mfcc, 1) == SMALL_IN
    blob = cube_synth.import_sources(*cube_synth.cube_sources(SMALL_IN, fr.zoo_specs("medium_embedding_conv", SMALL_IN), seed=5))
    m = cube_import.read_blob(blob)
    assert [pads for L in fh.conv_records(m) for pads in (L["cpad"], L["ppad"])][:4] == [(3, 3, 3, 3), (0, 0, 1, 1), (1, 1, 2, 2), (0, 0, 0, 0)]
    return blob, m, g


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    v = (lambda a: a.view(np.uint32)) if got.dtype == np.float32 else (lambda a: a)
    assert np.array_equal(v(got), v(want)), "%s: %d of %d differ" % (what, int((v(got) != v(want)).sum()), got.size)


@pytest.mark.parametrize("name", list(fr.PAD))
def test_row_bit_exact(ctx, name):
    blob = fr.blob(name)
    p, m = fpl.plan(blob), fr.model(name)
    ctx.fnet_load(blob)
    info = ctx.fnet_info()
    assert (info["batch"], info["lds_bytes"], info["acts_floats"], info["n_layers"], info["n_out"]) == \
        (p["batch"], p["lds_bytes"], p["acts_floats"], p["n_layers"], p["n_out"])
    n = 2 * p["batch"] + 1
    x = fr.inputs(name, n, p["in_n"])
    acts = ctx.fnet_layers(x)
    want, got = fh.layers_from(m, x, acts)
    prev = x
    for i, (L, w, g) in enumerate(zip(fh.conv_records(m), want, got)):
        diff = w.view(np.uint32) != g.view(np.uint32)
        assert not diff.any(), "%s layer %d: %d of %d outputs differ from the model (first at %s: gpu %r, model %r)" % (
            name, i, diff.sum(), diff.size, np.argwhere(diff)[0], g[diff][0], w[diff][0])
        w64, S = fh.layer_from(m, i, prev)
        assert (np.abs(g - w64) <= fh.bound(L, S)).all(), (name, i)
        prev = g
    r = ctx.fnet(x)
    _same(r["logits"], want[-1], name + " logits")
    assert np.abs(r["probs"] - fh.softmax(r["logits"].astype(np.float64))).max() <= 1e-6
    assert np.array_equal(r["argmax"], np.argmax(r["probs"], axis=1))
    z64 = fh.run64(m, x)["logits"]
    top = np.sort(z64, axis=1)
    clear = top[:, -1] - top[:, -2] > MARGIN if z64.shape[1] > 1 else np.ones(n, bool)
    assert np.array_equal(r["argmax"][clear], np.argmax(fh.softmax(z64), axis=1)[clear])
    # an utterance's answer does not depend on its neighbours in the tile
    one = ctx.fnet(x[n - 1:])
    _same(one["logits"], r["logits"][n - 1:], name + " last utterance alone")


def test_refusals_keep_the_loaded_network(ctx):
    """Every refusal returns its code and leaves the network loaded before it answering bit-identically."""
    from edison_amd import _lib
    name = "pool22_odd"
    ctx.fnet_load(fr.blob(name))
    p = fpl.plan(fr.blob(name))
    x = fr.inputs(name, p["batch"] + 1, p["in_n"])
    before, acts = ctx.fnet(x), ctx.fnet_layers(x)
    for ref, (build, code, note) in fr.PAD_REFUSALS.items():
        with pytest.raises(_lib.EdisonError) as e:
            ctx.fnet_load(build())
        assert e.value.code == code, (ref, note)
        after = ctx.fnet(x)
        assert all(np.array_equal(before[k], after[k]) for k in before), ref
        assert np.array_equal(ctx.fnet_layers(x), acts), ref


def _batch_call(c, g, x):
    """Context.kws_float on the zero-led recording, one utterance per full window (utt_stride = frame_step)."""
    z = np.concatenate([np.zeros(tail(g), np.int16), x])
    return c.kws_float(z, g, n_utt=x.shape[0] // g.frame_step - g.frame_count + 1, utt_stride=g.frame_step)


def _pushes(s, x):
    """Chunk-1 host pushes of a recording [K * hop] (a bank: [n_mics][K * hop]); the outputs stacked over the frames."""
    K = x.shape[-1] // s.hop
    parts = [s.push(x[..., k * s.hop:(k + 1) * s.hop]) for k in range(K)]
    return {k: np.concatenate([p[k] for p in parts]) for k in ("logits", "probs", "argmax")}


def test_stream_and_bank_on_a_padded_network(ctx, small):
    """FloatStream's outputs of full windows equal kws_float bit for bit; a FloatBank of 3 microphones equals three streams."""
    from edison_amd.stream import FloatBank, FloatStream
    blob, m, g = small
    ctx.fnet_load(blob)
    K, F = 30, g.frame_count
    xs = recordings(g, 3, K, 91)
    streams = []
    for mic in range(3):
        s = FloatStream(ctx, g)
        streams.append(_pushes(s, xs[mic]))
        assert s.frames_seen == K
        s.close()
        want = _batch_call(ctx, g, xs[mic])
        for k in ("logits", "probs", "argmax"):
            _same(streams[mic][k][F - 1:], want[k], "microphone %d stream against kws_float: %s" % (mic, k))
    # the batch call's features through the host model: the stream's logits are the padded chain's
    feat = _batch_call(ctx, g, xs[0])["feat"]
    _same(streams[0]["logits"][F - 1:], fh.run(m, feat)[-1], "stream logits against the host model")
    b = FloatBank(ctx, 3, g)
    got = _pushes(b, xs)
    b.close()
    for mic in range(3):
        for k in ("logits", "probs", "argmax"):
            _same(got[k][:, mic], streams[mic][k], "bank microphone %d %s" % (mic, k))


@pytest.mark.parametrize("name", ["pool22_odd", "pool41_lead", "neg_no_relu", "mid_pads_batch"])
def test_calibrator_counters(ctx, name):
    """absmax, hist and count equal the host restatement exactly: absent elements are counted nowhere, count = present rows x out_c."""
    m, blob = fr.model(name), fr.blob(name)
    p = fpl.plan(blob)
    ctx.fnet_load(blob)
    with ctx.calibrator() as cal:
        batch = cal.batch
        x = fr.inputs(name, 2 * batch + 1, p["in_n"])
        for k in sorted({1, batch + 1, 2 * batch + 1}):
            cal.reset()
            cal.add(x[:k])
            got, want = cal.result(), fh.stats(m, x[:k])
            for key in ("count", "absmax", "hist"):
                assert np.array_equal(got[key], want[key]), "%s, n = %d: %s differs at %s" % (name, k, key, np.argwhere(got[key] != want[key])[:4].tolist())
            assert (got["hist"].sum(axis=1) == got["count"]).all()
            assert got["count"].tolist() == [k * p["in_n"]] + [k * L["live"] * L["out_c"] for L in p["layers"]]
    if name == "neg_no_relu":
        assert (fh.run(m, x)[0] < -30).all()          # every pooled value is a real one: none came from an absent 0


def test_quantize_medium_embedding_conv(ctx, small):
    """Context.quantize on the padded network: the .ednn carries PADDING_SAME on both convs and the pool, equals the blob of the host
    statistic, and the int8 kernel runs it equal to the int8 checker (oracle/net_ref.py), as test_gpu_quantize.py checks unpadded ones."""
    from edison_amd import nnom_import
    blob, m, g = small
    ctx.fnet_load(blob)
    audio = recordings(g, 6, g.frame_count + 1, 7)[:, :g.n_samples]
    q, rep = ctx.quantize(audio.ravel(), geometry=g, chunk=4, return_features=True)
    want_q, _ = qz.quantize(m, fh.stats(m, rep["features"]))
    assert q == want_q
    assert [(L["type"], L["same"]) for L in rep["graph"] if "same" in L] == [(nnom_import.T_CONV, 1), (nnom_import.T_POOL, 1), (nnom_import.T_CONV, 1)]
    (_, recs, _) = net_ref.parse_blob(q)
    assert [(v[8] >> 1) & 1 for v in recs if v[0] in (net_ref.T_CONV, net_ref.T_POOL)] == [1, 1, 1]
    xi = qz.quantize_input(rep["features"], rep["input"]["dec"])
    ctx.load_model_bytes(q)
    got, ref = ctx.net(xi), net_ref.run(q, xi)
    assert np.array_equal(got["logits"], ref["logits"]) and np.array_equal(got["softmax"], ref["softmax"])
    assert np.array_equal(got["argmax"], ref["argmax"])
    # a padded record NNoM cannot express is refused by name, with the context still usable
    ctx.fnet_load(fr.blob("tiny_embedding_conv"))
    with ctx.calibrator() as cal:
        cal.add(fr.inputs("tiny_embedding_conv", 3, 403))
        with pytest.raises(qz.QuantizeError, match="^conv2d_2: its conv pads"):
            qz.quantize(fr.model("tiny_embedding_conv"), cal.result())


def test_shipped_network_unchanged_around_a_padded_load(ctx):
    """edison_fnet_batch on the shipped network answers the same before and after a padded network was loaded and run on the context."""
    rng = np.random.default_rng(6)
    x = rng.normal(0, 60, (40, 403)).astype(np.float32)
    ctx.fnet_load(FIXTURE)
    before, acts = ctx.fnet(x), ctx.fnet_layers(x[:9])
    want, got = fh.layers_from(fh.load(FIXTURE), x[:9], acts)
    assert all(np.array_equal(w, g) for w, g in zip(want, got))
    ctx.fnet_load(fr.blob("medium_embedding_conv"))
    ctx.fnet(x)
    ctx.fnet_load(FIXTURE)
    after = ctx.fnet(x)
    for k in before:
        _same(after[k], before[k], "shipped network " + k)
    _same(ctx.fnet_layers(x[:9]), acts, "shipped network layers")

"""GPU tests (-m gpu) of float32 X-CUBE-AI networks (edison_fnet_*, edison_kws_float_batch*). The reference answer is
tests/fnet_host.py, the float64 restatement of the Cube layers, on the .ednf fixture of the reference's own network
(tests/golden/cube_kws.ednf) and on networks generated in the importer's input format (tests/cube_synth.py).

Bounds (DESIGN.md section 14 has what was measured):
  every layer, fed the kernel's own previous layer: |gpu - f64| <= K_BOUND 1e-7 S, S = sum |a| |w| + |bias| (f32 MFMA: a k-ordered fmaf chain)
    and, on up to 266 inputs per call, bit-equal to the host model of that chain (tests/fnet_host.py)
  probabilities: within 1e-6 of the float64 softmax of the kernel's logits
  argmax: equal to the float64 chain's wherever its top-2 logit margin exceeds MARGIN
  host-flow features: at most FEAT_FLIPS elements per utterance differ from the reference's float32 net input, by 1 ulp"""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

import cube_synth
import fnet_host

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "cube_kws.ednf")
K_BOUND = 8.0
MARGIN = 1e-3
FEAT_FLIPS = 2
SOURCES = ("edison", "hey", "noise0", "noise1", "noise2")


@pytest.fixture(scope="module")
def fctx(built_lib):
    from edison_amd.context import Context
    c = Context(0)
    c.fnet_load(FIXTURE)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model():
    return fnet_host.load(FIXTURE)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "cube_golden.npz"))


def _inputs(golden, n=4096):
    rng = np.random.default_rng(2024)
    x = rng.normal(0, 60, (n, 403)).astype(np.float32)
    x[: n // 4] *= 20                                    # int16-range features, as the host flow's clip allows
    fx = [golden["net_in_" + s] for s in SOURCES] + [golden["q15_" + s].astype(np.float32).reshape(-1) for s in SOURCES]
    return np.concatenate([x, np.stack(fx)])


EXACT_N = 256       # inputs of a call checked bit for bit against fnet_host (the first 256 and the last 10: the fixture inputs)


def check_layers(ctx, model, x):
    """Every layer of the kernel against the restatement fed the kernel's own previous layer, and bit for bit against the host model
    of the kernel (tests/fnet_host.py: k-ordered fmaf chain, bias, ReLU, pool) on at most EXACT_N + 10 of the inputs; returns the
    largest err / (1e-7 S)."""
    acts32 = ctx.fnet_layers(x)
    pick = np.arange(len(x)) if len(x) <= EXACT_N + 10 else np.r_[:EXACT_N, len(x) - 10:len(x)]
    want, got = fnet_host.layers_from(model, np.asarray(x, np.float32)[pick], acts32[pick])
    for i, (w, g) in enumerate(zip(want, got)):
        assert np.array_equal(w, g), "layer %d: %d of %d outputs differ from the fmaf chain" % (i, (w != g).sum(), w.size)
    acts = acts32.astype(np.float64)
    prev, off, worst = np.asarray(x, np.float64), 0, 0.0
    for i, L in enumerate(fnet_host.conv_records(model)):
        n_out = int(np.prod(L["out"]))
        got = acts[:, off:off + n_out]
        want, S = fnet_host.layer_from(model, i, prev)
        err = np.abs(got - want)
        bad = err > K_BOUND * 1e-7 * S
        assert not bad.any(), "layer %d: %d outputs outside %g 1e-7 S (worst ratio %.3g)" % (i, bad.sum(), K_BOUND, (err / (1e-7 * S + 1e-300)).max())
        worst = max(worst, float((err / (1e-7 * S + 1e-300)).max()))
        prev, off = got, off + n_out
    assert off == acts.shape[1]
    return acts, worst


def test_info(fctx):
    i = fctx.fnet_info()
    assert (i["in_h"], i["in_w"], i["in_c"], i["n_out"], i["n_layers"]) == (31, 13, 1, 10, 5)
    assert i["acts_floats"] == 13 * 9 * 16 + 5 * 7 * 32 + 3 * 5 * 64 + 3 * 32 + 10
    assert i["batch"] >= 1 and i["lds_bytes"] <= 160 * 1024


def test_net_alone(fctx, model, golden):
    x = _inputs(golden)
    acts, _ = check_layers(fctx, model, x)
    r = fctx.fnet(x)
    # logits = the last layer of the dump (same kernel, same arithmetic)
    assert np.array_equal(r["logits"], acts[:, -10:].astype(np.float32))
    p64 = fnet_host.softmax(r["logits"].astype(np.float64))
    assert np.abs(r["probs"] - p64).max() <= 1e-6
    assert np.array_equal(r["argmax"], np.argmax(r["probs"], axis=1))
    ref = fnet_host.run64(model, x)
    top = np.sort(ref["logits"], axis=1)
    clear = top[:, -1] - top[:, -2] > MARGIN
    assert clear.mean() > 0.99
    assert np.array_equal(r["argmax"][clear], ref["argmax"][clear])
    # the fixture inputs' probabilities against the generator's float64 ones
    for j, s in enumerate(SOURCES):
        np.testing.assert_allclose(r["probs"][4096 + j], golden["probs_" + s], rtol=0, atol=1e-5)
        np.testing.assert_allclose(r["probs"][4096 + 5 + j], golden["q15_probs_" + s], rtol=0, atol=1e-5)


@pytest.mark.parametrize("n", [1, 6, 7, 8, 50])
def test_batch_edges(fctx, model, golden, n):
    """Utterance counts around the workgroup's tile: each utterance's result does not depend on its neighbours."""
    x = _inputs(golden, 64)[:n]
    r = fctx.fnet(x)
    one = np.concatenate([fctx.fnet(x[i:i + 1])["logits"] for i in range(n)])
    assert np.array_equal(r["logits"], one)


def _audio(golden):
    return np.stack([golden["audio_" + s] for s in SOURCES])


def test_host_flow(fctx, golden):
    a = _audio(golden)
    r = fctx.kws_float(a)
    for j, s in enumerate(SOURCES):
        want = golden["net_in_" + s]
        d = r["feat"][j] != want
        assert d.sum() <= FEAT_FLIPS, (s, int(d.sum()))
        if d.any():
            ulp = np.abs(r["feat"][j][d].view(np.int32).astype(np.int64) - want[d].view(np.int32).astype(np.int64))
            assert ulp.max() <= 1
    assert r["argmax"][0] == 0
    assert abs(r["probs"][0, 0] - golden["probs_edison"][0]) <= 1e-5
    # the features go through the same kernel as the net alone
    assert np.array_equal(fctx.fnet(r["feat"])["logits"], r["logits"])


def test_firmware_flow(fctx, model, golden):
    a = _audio(golden)
    r = fctx.kws_float(a, q15=True)
    for j, s in enumerate(SOURCES):
        q = fctx.mfcc_q15(a[j][:31 * 1024], n_coef=13)
        assert np.array_equal(r["feat"][j], q.astype(np.float32).reshape(-1))
        assert np.array_equal(q, golden["q15_" + s])
    check_layers(fctx, model, r["feat"])
    ref = fnet_host.run64(model, r["feat"])
    assert np.abs(r["logits"] - ref["logits"]).max() <= 1e-4 * (1.0 + np.abs(ref["logits"]).max())
    for j, s in enumerate(SOURCES):
        np.testing.assert_allclose(r["logits"][j], golden["q15_logits_" + s], rtol=0, atol=1e-4 * (1.0 + np.abs(ref["logits"]).max()))
    top = np.sort(ref["logits"], axis=1)
    clear = top[:, -1] - top[:, -2] > MARGIN
    assert np.array_equal(r["argmax"][clear], ref["argmax"][clear])


def test_device_form(fctx, golden):
    torch = pytest.importorskip("torch")
    from edison_amd.kws.geometry import KwsGeometry
    a = _audio(golden)
    want = fctx.kws_float(a)
    dev = torch.device("cuda", 0)
    au = torch.from_numpy(a.reshape(-1).copy()).to(dev)
    n = a.shape[0]
    feat = torch.zeros((n, 403), dtype=torch.float32, device=dev)
    lg = torch.zeros((n, 10), dtype=torch.float32, device=dev)
    pr = torch.zeros((n, 10), dtype=torch.float32, device=dev)
    am = torch.zeros(n, dtype=torch.int32, device=dev)
    fctx.use_torch_stream()
    try:
        fctx.kws_float_t(au, KwsGeometry.from_config(), n, 32000, feat, lg, pr, am)
        torch.cuda.current_stream().synchronize()
    finally:
        fctx.use_own_stream()
    assert np.array_equal(feat.cpu().numpy(), want["feat"]) and np.array_equal(pr.cpu().numpy(), want["probs"])
    assert np.array_equal(am.cpu().numpy(), want["argmax"])


SECOND_GEOM = dict(frame_len=512, frame_step=256, n_samples=16000, mel_nbins=20, num_mfcc=10, lower_edge_hertz=125.0, upper_edge_hertz=3800.0,
                   net_input_scale=0.5)
SECOND_NET = [("conv", 12, (5, 3), (1, 1), (2, 2), 1), ("conv", 70, (3, 2), (2, 1), (1, 1), 1), ("conv", 24, (3, 2), (1, 1), (2, 1), 0),
              ("dense", 40), ("relu",), ("dense", 6), ("softmax",)]


def test_second_geometry(built_lib, tmp_path):
    """A float network at another geometry (61 frames x 10 coefficients), generated in X-CUBE-AI's format from seeded weights and
    imported: net alone per layer, then audio -> class through the host flow with its own scale and clip."""
    from edison_amd import cube_import
    from edison_amd.context import Context
    from edison_amd.kws.geometry import KwsGeometry
    g = KwsGeometry.from_config(**SECOND_GEOM)
    assert g.frame_count == 61
    net_c, data_c = cube_synth.cube_sources((61, 10, 1), SECOND_NET, seed=11)
    (tmp_path / "n.c").write_text(net_c)
    (tmp_path / "n_data.c").write_text(data_c)
    blob = cube_import.import_files(str(tmp_path / "n.c"), str(tmp_path / "n_data.c"))
    m = fnet_host.load(blob)
    ctx = Context(0)
    try:
        ctx.fnet_load(blob)
        assert ctx.fnet_info()["n_layers"] == 5
        x = np.random.default_rng(3).normal(0, 30, (1000, 610)).astype(np.float32)
        check_layers(ctx, m, x)
        rng = np.random.default_rng(4)
        a = np.clip(rng.normal(0, 2000, 9 * 16000), -32768, 32767).astype(np.int16)
        r = ctx.kws_float(a, g, clip_min=-40.0, clip_max=40.0)
        y = ctx.mfcc_geom(a, g).reshape(9, -1)
        want = np.clip(y.astype(np.float32) * np.float32(0.5), np.float32(-40.0), np.float32(40.0))
        assert np.array_equal(r["feat"], want)
        check_layers(ctx, m, r["feat"])
        np.testing.assert_allclose(r["probs"], fnet_host.softmax(r["logits"].astype(np.float64)), rtol=0, atol=1e-6)
    finally:
        ctx.close()


def test_errors(built_lib, golden, tmp_path):
    from edison_amd import _lib
    from edison_amd.context import Context
    from edison_amd.kws.geometry import KwsGeometry
    ctx = Context(0)
    try:
        a = golden["audio_edison"]
        # no float network loaded: every entry point says so; the int8 path is unaffected
        for call in (lambda: ctx.fnet_info(), lambda: ctx.fnet(np.zeros((1, 403), np.float32)), lambda: ctx.kws_float(a)):
            with pytest.raises(_lib.EdisonError) as e:
                call()
            assert e.value.code == _lib.E_NO_MODEL
        before = ctx.kws(a, n_utt=1)
        # unsupported / malformed files
        good = open(FIXTURE, "rb").read()
        for blob, code in ((b"NOPE" + good[4:], _lib.E_SIZE), (good[:-4], _lib.E_SIZE), (good[:4] + b"\x02" + good[5:], _lib.E_NO_IMPL)):
            with pytest.raises(_lib.EdisonError) as e:
                ctx.fnet_load(blob)
            assert e.value.code == code
        bad = tmp_path / "x.ednf"
        bad.write_bytes(good[:100])
        with pytest.raises(_lib.EdisonError):
            ctx.fnet_load(str(bad))
        with pytest.raises(_lib.EdisonError):
            ctx.fnet_info()
        # softmax not last: the record order is checked
        import struct
        nl = struct.unpack_from("<i", good, 8)[0]
        recs = bytearray(good)
        first = 32
        last = 32 + 64 * (nl - 1)
        recs[first:first + 64], recs[last:last + 64] = good[last:last + 64], good[first:first + 64]
        with pytest.raises(_lib.EdisonError) as e:
            ctx.fnet_load(bytes(recs))
        assert e.value.code in (_lib.E_NO_IMPL, _lib.E_SIZE)
        # wrong size: 12 coefficients x 31 frames for a 403-input network
        ctx.fnet_load(FIXTURE)
        with pytest.raises(_lib.EdisonError) as e:
            ctx.kws_float(a, KwsGeometry.from_config(num_mfcc=12))
        assert e.value.code == _lib.E_SIZE
        with pytest.raises(_lib.EdisonError) as e:
            ctx.kws_float(a, KwsGeometry.from_config(frame_len=512, frame_step=512, num_mfcc=13, n_samples=16384), q15=True)
        assert e.value.code == _lib.E_NO_IMPL
        # both kinds of network in one context: the int8 answer is unchanged
        after = ctx.kws(a, n_utt=1)
        assert all(np.array_equal(before[k], after[k]) for k in before)
        assert ctx.kws_float(a)["argmax"][0] == 0
    finally:
        ctx.close()


def test_kws_host_net_option(built_lib, golden, tmp_path, capsys):
    """`kws mcu fileinf|frame|file <wav> --net <file.ednf>`: the float flow, printed as kws_on_mcu.report prints it."""
    import scipy.io.wavfile as wavfile
    from edison_amd.kws import kws_host
    wav = tmp_path / "edison.wav"
    wavfile.write(str(wav), 16000, golden["audio_edison"])
    for mode in ("fileinf", "frame", "file"):
        assert kws_host.main(["mcu", mode, str(wav), "--net", FIXTURE]) == 0
        out = capsys.readouterr().out
        assert "host prediction:" in out and "edison" in out.split("host prediction:")[1].splitlines()[0]
        assert ("mcu prediction:" in out) == (mode == "file")

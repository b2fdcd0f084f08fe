"""GPU tests (-m gpu) of keyword spotting at any MFCC geometry (edison_kws_geom_batch*, Context.kws_geom): audio -> float64 MFCC ->
int8 features -> the loaded graph in one call. The reference answer is the reference's host flow restated: oracle.mfcc_numpy (float64
numpy, pinned on the reference's own outputs in test_oracle.py), the coefficients first_mfcc .. first_mfcc + num_mfcc - 1, float32 *
net_input_scale, clip, round half to even (oracle.net_input), then the graph on those features through ctx.net (pinned bit-exact on
NNoM elsewhere). Everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest

from geom_sweep import GEOMS, geom, header, signals

pytestmark = pytest.mark.gpu


def _oracle_feat(oracle, rows, g, starts=None):
    """The reference's int8 features of each utterance: rows [n][>= span] int16 (or a flat stream with `starts`)."""
    import geom_sweep
    return geom_sweep.oracle_feat(oracle, geom_sweep.oracle_mfcc(oracle, rows, g, starts), g)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d differences, first at %s" % (what, bad.shape[0], bad[:5].tolist())


def _check_against_oracle(c, r, feat_ref):
    _same(r["feat"], feat_ref, "features")
    o = c.net(feat_ref)
    _same(r["logits"], o["logits"], "logits")
    _same(r["argmax"], o["argmax"], "argmax")
    if o["softmax"] is None:
        assert r["softmax"] is None
    else:
        _same(r["softmax"], o["softmax"], "softmax")


def test_shipped_geometry_equals_exact_kws_and_oracle(oracle_mod):
    """audio/config.py's geometry and the shipped graph, 16 384 utterances: host and device forms equal kws(exact=True) and the oracle."""
    import torch
    from edison_amd.context import Context
    c = Context(0)
    try:
        g = geom()
        assert (g.frame_count, g.num_mfcc, g.n_features) == (31, 13, 403)
        audio = signals(16384, 32000, 11)
        r = c.kws_geom(audio, g)
        ex = c.kws(audio, n_utt=audio.shape[0], utt_stride=32000, exact=True)
        for k in ("feat", "logits", "softmax", "argmax"):
            _same(r[k], ex[k], "kws(exact=True) " + k)
        _check_against_oracle(c, r, _oracle_feat(oracle_mod, audio, g))
        # the device form on a torch stream
        dev = torch.device("cuda", c.device)
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            a = torch.from_numpy(audio).to(dev)
            n = audio.shape[0]
            feat = torch.zeros((n, 403), dtype=torch.int8, device=dev)
            logits = torch.zeros((n, 10), dtype=torch.int8, device=dev)
            soft = torch.zeros((n, 10), dtype=torch.int8, device=dev)
            am = torch.zeros(n, dtype=torch.int32, device=dev)
            c.use_torch_stream(s)
            c.kws_geom_t(a, g, n, 32000, feat, logits, soft, am)
        s.synchronize()
        c.use_own_stream()
        for k, t in (("feat", feat), ("logits", logits), ("softmax", soft), ("argmax", am)):
            _same(t.cpu().numpy(), r[k], "device form " + k)
    finally:
        c.close()


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_retrained_graphs_at_their_geometry(oracle_mod, name):
    """Each committed alt_models graph, run at the geometry its input shape implies: 2 048 utterances, bit-exact features, logits,
    softmax (not written for odd_no_softmax) and argmax."""
    from edison_amd import _lib
    from edison_amd.context import Context, _np_ptr
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(header(name))
        info = c.net_info()
        g = geom(**GEOMS[name])
        assert g.n_features == info["in_h"] * info["in_w"] * info["in_c"]
        audio = signals(2048, g.n_samples, 100 + len(name))
        r = c.kws_geom(audio, g)
        _check_against_oracle(c, r, _oracle_feat(oracle_mod, audio, g))
        assert (r["softmax"] is None) == (name == "odd_no_softmax")
        # a softmax buffer handed to a graph without Softmax is left as it was
        n = 64
        soft = np.full((n, info["n_out"]), 0x55, np.int8)
        logits = np.zeros((n, info["n_out"]), np.int8)
        am = np.zeros(n, np.int32)
        gc = g.to_ctypes()
        assert c._L.edison_kws_geom_batch(c._h, ctypes.byref(gc), _np_ptr(audio), n, g.n_samples, None, _np_ptr(logits), _np_ptr(soft),
                                          _np_ptr(am)) == _lib.OK
        _same(logits, r["logits"][:n], "logits, feat NULL")
        _same(am, r["argmax"][:n], "argmax, feat NULL")
        if info["has_softmax"]:
            _same(soft, r["softmax"][:n], "softmax")
        else:
            assert (soft == 0x55).all()
    finally:
        c.close()


@pytest.mark.parametrize("name", ["kws_small", "square", "odd_no_softmax"])
def test_features_equal_the_generic_kernel(name):
    """The new kernel's int8 features equal edison_mfcc_generic's `feat` (direct DFT, dense mel product) on the same frames."""
    from edison_amd import _lib
    from edison_amd.context import Context
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(header(name))
        g = geom(**GEOMS[name])
        audio = signals(160, g.n_samples, 7)
        r = c.kws_geom(audio, g)
        gc = g.to_ctypes()
        F = g.frame_count
        for u in range(audio.shape[0]):
            x = np.ascontiguousarray(audio[u])
            feat = np.zeros((F, g.num_mfcc), np.int8)
            assert g.first_mfcc == 0
            assert c._L.edison_mfcc_generic(c._h, x.ctypes.data, F, g.frame_len, g.frame_step, gc.variant, g.mel_nbins, g.sample_rate,
                                            g.lower_edge_hertz, g.upper_edge_hertz, g.mel_mtx_scale, None, None, None, None, None,
                                            g.num_mfcc, feat.ctypes.data, g.net_input_scale) == _lib.OK
            _same(r["feat"][u], feat.reshape(-1), "utterance %d" % u)
    finally:
        c.close()


def test_errors_and_recovery():
    """Every refusal of section 2 of the entry point's contract, and correct results after each."""
    from edison_amd import _lib
    from edison_amd.context import Context, _np_ptr
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(header("kws_small"))
        g = geom(**GEOMS["kws_small"])
        audio = signals(20, g.n_samples, 5)
        good = c.kws_geom(audio, g)

        def code(gg, n_utt=2, stride=None, a=audio):
            gc = gg.to_ctypes()
            r = c._L.edison_kws_geom_batch(c._h, ctypes.byref(gc), _np_ptr(a), n_utt, gg.n_samples if stride is None else stride, None, None, None, None)
            msg = (c._L.edison_last_error(c._h) or b"").decode()
            again = c.kws_geom(audio, g)
            for k in ("feat", "logits", "softmax", "argmax"):
                _same(again[k], good[k], "after an error: " + k)
            return r, msg

        from dataclasses import replace
        r, msg = code(replace(g, num_mfcc=12))
        assert r == _lib.E_SIZE and "372" in msg and "403" in msg, msg
        assert code(replace(g, frame_count_=30))[0] == _lib.E_SIZE
        for bad in (dict(variant=_lib.MFCC_TF, use_log=False), dict(variant=_lib.MFCC_C, use_log=False), dict(frame_len=8192, n_samples=70000),
                    dict(frame_len=2), dict(mel_nbins=257), dict(mel_nbins=0)):
            assert code(replace(g, **bad))[0] == _lib.E_NO_IMPL, bad
        for bad in (dict(first_mfcc=8), dict(lower_edge_hertz=8000.0), dict(upper_edge_hertz=-1.0), dict(mel_mtx_scale=0.0),
                    dict(n_samples=500), dict(frame_step=0), dict(variant=_lib.MFCC_A, use_log=True)):
            assert code(replace(g, **bad))[0] == _lib.E_ARGUMENT, bad
        assert code(g, n_utt=0)[0] == _lib.OK
        # a span beyond what the staging buffer can hold: refused before anything is read
        assert code(g, n_utt=3, stride=1 << 60)[0] == _lib.E_SIZE
        # the device form refuses the same geometries
        gc = replace(g, num_mfcc=12).to_ctypes()
        assert c._L.edison_kws_geom_batch_dev(c._h, ctypes.byref(gc), None, 0, 0, None, None, None, None) == _lib.E_SIZE
        c2 = Context(0, model_path=None)
        try:
            gc = g.to_ctypes()
            assert c2._L.edison_kws_geom_batch(c2._h, ctypes.byref(gc), _np_ptr(audio), 2, g.n_samples, None, None, None, None) == _lib.E_NO_MODEL
        finally:
            c2.close()
    finally:
        c.close()


def test_state_isolation():
    """Two geometries in turn on one context, with kws() and edison_mfcc_configure calls in between: every result equals a fresh
    context's, and kws() is byte-identical before and after."""
    from edison_amd.context import Context
    g1 = geom()
    g2 = geom(**GEOMS["kws_small"])   # 31 x 13 as well: the shipped graph takes it
    audio = signals(300, 32000, 21)

    def fresh(fn):
        f = Context(0)
        try:
            return fn(f)
        finally:
            f.close()

    want1 = fresh(lambda f: f.kws_geom(audio, g1))
    want2 = fresh(lambda f: f.kws_geom(audio, g2))
    want_conf = fresh(lambda f: (f.configure_mfcc(16000, 300.0, 3400.0, 128), f.kws(audio, n_utt=300))[1])
    c = Context(0)
    try:
        base = c.kws(audio, n_utt=300)
        for step in range(3):
            r1 = c.kws_geom(audio, g1)
            k = c.kws(audio, n_utt=300)
            r2 = c.kws_geom(audio, g2)
            c.configure_mfcc(16000, 300.0, 3400.0, 128)
            kc = c.kws(audio, n_utt=300)
            r2b = c.kws_geom(audio, g2)
            r1b = c.kws_geom(audio, g1)
            c.configure_mfcc()
            for key in ("feat", "logits", "softmax", "argmax"):
                for got, want, what in ((r1, want1, "g1"), (r1b, want1, "g1 after configure"), (r2, want2, "g2"), (r2b, want2, "g2 after configure"),
                                        (k, base, "kws"), (kc, want_conf, "kws, configured")):
                    _same(got[key], want[key], "step %d %s %s" % (step, what, key))
        after = c.kws(audio, n_utt=300)
        for key in ("feat", "logits", "softmax", "argmax"):
            assert after[key].tobytes() == base[key].tobytes()
    finally:
        c.close()


def test_ragged_and_odd_shapes(oracle_mod):
    """utt_stride > n_samples (gaps), utt_stride < n_samples (overlapping utterances), and one utterance."""
    from edison_amd.context import Context
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(header("same_stride"))
        g = geom(**GEOMS["same_stride"])
        stream = signals(1, 300 * 16000, 3).reshape(-1)
        for stride, n in ((16000 + 37, 200), (16000 * 3 + 1, 90), (5003, 700), (800, 1000), (1, 500), (0, 3)):
            r = c.kws_geom(stream, g, n_utt=n, utt_stride=stride)
            _check_against_oracle(c, r, _oracle_feat(oracle_mod, stream, g, starts=[u * stride for u in range(n)]))
        one = signals(5, g.n_samples, 8)[4]
        r = c.kws_geom(one, g, n_utt=1)
        _check_against_oracle(c, r, _oracle_feat(oracle_mod, one[None, :], g))
    finally:
        c.close()


def test_host_flow_with_a_geometry(tmp_path):
    """kws_host.file_inference / infer_utterances with a geometry pad or cut to geometry.n_samples and run kws_geom; without one they
    are unchanged."""
    import scipy.io.wavfile as wavfile
    from edison_amd.context import Context
    from edison_amd.kws import kws_host
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(header("square"))
        g = geom(**GEOMS["square"])
        x = signals(5, 20000, 4)[4]
        path = str(tmp_path / "u.wav")
        wavfile.write(path, 16000, x)
        r = kws_host.file_inference(path, ctx=c, verbose=False, geometry=g)
        want = c.kws_geom(x[:g.n_samples], g, n_utt=1)
        for k in ("feat", "logits", "softmax", "argmax"):
            _same(r[k], want[k], k)
        short = x[:9000]
        r = kws_host.infer_utterances(np.stack([short, short]), ctx=c, geometry=g)
        want = c.kws_geom(np.pad(short, (0, g.n_samples - 9000)), g, n_utt=1)
        _same(r["feat"][1], want["feat"][0], "padded")
    finally:
        c.close()
    d = Context(0)
    try:
        x = signals(5, 32000, 4)[4]
        path = str(tmp_path / "v.wav")
        wavfile.write(path, 16000, x)
        r = kws_host.file_inference(path, ctx=d, verbose=False)
        want = d.kws(x, n_utt=1)
        for k in ("feat", "logits", "softmax", "argmax"):
            _same(r[k], want[k], k)
    finally:
        d.close()

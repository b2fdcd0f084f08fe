"""GPU tests (-m gpu) of float64 MFCC at any geometry (edison_mfcc_geom_batch*, Context.mfcc_geom / mfcc_geom_t, and
kws.features.dataset_features(..., geometry=)): ed_mfcc_geom_f64_kernel, the float64 instance of the any-geometry kernel that stores the
DCT row value y instead of its int8 rounding.

The references: the reference's own outputs at six geometries (tests/golden/mfcc_geom_golden.npz), oracle.mfcc_numpy over every row of
tests/geom_sweep.py (test_gpu_generic's bar, 1e-9 of the largest value + 1e-9), and the int8 path itself -- the float32 rounding of the
new output must be edison_kws_geom_batch's features bit for bit, at each row's sensitive scale."""
import ctypes

import numpy as np
import pytest

import geom_sweep as gs
from geom_sweep import GEOMS, geom, signals
from test_gpu_generic import GOLDEN, _near

pytestmark = pytest.mark.gpu

NAMES = sorted(gs.ROWS)


def _int8(y, scale):
    """kws_nnom.py:359-361 on float64 coefficients: int8(rint(clip(float32(y) * float32(scale), -128, 127)))."""
    v = np.asarray(y).astype(np.float32) * np.float32(scale)
    return np.rint(np.clip(v, np.float32(-128), np.float32(127))).astype(np.int8)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d differences, first at %s" % (what, bad.shape[0], bad[:5].tolist())


@pytest.mark.parametrize("idx", range(6))
def test_whole_rows_equal_the_reference(idx):
    """At the six geometries of mfcc_geom_golden.npz (g33 takes the direct DFT), first_mfcc = 0, num_mfcc = mel_nbins, one utterance of
    len(x) samples: variants A, B and B with log equal the reference's own mfcc / mfcc_mcu outputs within the bar. No model is loaded."""
    from edison_amd import _lib
    from edison_amd.context import Context
    golden = np.load(GOLDEN)
    name = str(golden["names"][idx])
    N, step, nm, lo, hi, scale = golden["configs"][idx]
    N, step, nm = int(N), int(step), int(nm)
    c = Context(0, model_path=None)
    try:
        for sname in ("edison", "noise"):
            x = golden["in_" + sname]
            k = "%s_%s_" % (name, sname)
            for tag, variant, use_log in (("A", _lib.MFCC_A, False), ("B", _lib.MFCC_B, False), ("Blog", _lib.MFCC_B, True)):
                g = geom(variant=variant, use_log=use_log, frame_len=N, frame_step=step, n_samples=len(x), mel_nbins=nm, first_mfcc=0,
                         num_mfcc=nm, sample_rate=16000.0, lower_edge_hertz=float(lo), upper_edge_hertz=float(hi), mel_mtx_scale=float(scale))
                got = c.mfcc_geom(x, g)
                assert got.shape == (1, g.frame_count, nm) and got.dtype == np.float64
                _near(got[0], golden[k + tag + "_mfcc"], k + tag + "_mfcc")
    finally:
        c.close()


def _log_allowance(audio, g):
    """[n_utt][F][num_mfcc]: what a float64 rounding of the mel bands can become through ln(e + 1e-6) and the DCT. A band whose exact
    value is 0 or near it (a bin that meets no band, a frame with little energy at that frequency) keeps a rounding residue of the
    transform -- for any float64 transform, at most ~N eps sum|x| per bin, about eps of the frame's large terms -- and ln(e + 1e-6)
    turns that into up to 1e-5 (the same effect test_gpu_geom_sweep's generic test allows for with the kernel's own mel). Per band:
    delta = N eps fft_scale spec_scale sum|x| * (the band's filter weight sum); the allowance is ln(e + delta + 1e-6) -
    ln(max(e - delta, 0) + 1e-6) at the oracle's band value e, carried through |DCT| / dct_div. 0 for variant B without ln."""
    from edison_amd import _lib
    from oracle import oracle
    from test_gpu_geom_sweep import _numpy_chain
    a_variant = g.variant == _lib.MFCC_A
    if not (a_variant or g.use_log):
        return 0.0
    N, F, nm = g.frame_len, g.frame_count, g.mel_nbins
    nb = N // 2 if a_variant else N // 2 + 1
    W = oracle.mel_weight_matrix(nm, nb, g.sample_rate, g.lower_edge_hertz, g.upper_edge_hertz)
    rows = np.arange(g.first_mfcc, g.first_mfcc + g.num_mfcc)
    D = 2.0 * np.cos(np.pi * np.outer(np.arange(nm), 2 * np.arange(nm) + 1) / (2.0 * nm))
    dct_div = np.sqrt(2.0 * nm) if a_variant else 64.0
    scale = 1.0 if a_variant else 1.0 / 1024.0 / np.sqrt(2.0)
    out = np.zeros((audio.shape[0], F, g.num_mfcc))
    for u in range(audio.shape[0]):
        x = audio[u, :(F - 1) * g.frame_step + N]
        _, _, mel, _ = _numpy_chain(x, g, W, D, dct_div)
        l1 = np.array([np.abs(x[f * g.frame_step:f * g.frame_step + N].astype(np.float64)).sum() for f in range(F)])
        delta = N * np.finfo(np.float64).eps * scale * l1[:, None] * W.sum(axis=0)[None, :]
        d_l = np.log(mel + delta + 1e-6) - np.log(np.maximum(mel - delta, 0.0) + 1e-6)
        out[u] = d_l @ np.abs(D[rows]).T / dct_div
    return out


@pytest.mark.parametrize("name", NAMES)
def test_sweep_row_equals_the_oracle_and_rounds_to_the_int8_path(name):
    """Every path of the kernel (both teams x packed / odd / direct, radices 2-5, N 4-4096, mel 1-256): the float64 output is within the
    bar of oracle.mfcc_numpy (plus, where ln is taken, the rounding of near-zero mel bands carried through it: _log_allowance), and its
    float32 rounding at the row's sensitive scale is edison_kws_geom_batch's int8 features bit for bit (the row's dense graph loaded, as
    the sweep test runs it)."""
    from edison_amd.context import Context
    g, audio, y, want = gs.row_data(name)
    c = Context(0, model_path=None)
    try:
        got = c.mfcc_geom(audio, g)
        assert got.shape == y.shape == (audio.shape[0], g.frame_count, g.num_mfcc)
        extra = _log_allowance(audio, g)
        tol = 1e-9 * max(1.0, float(np.abs(y).max())) + 1e-9 + extra
        d = np.abs(got - y)
        assert (d <= tol).all(), "%s mfcc: max |d| - tol %.3e at %s" % (name, float((d - tol).max()), np.unravel_index(np.argmax(d - tol), d.shape))
        if np.ndim(extra):
            # the allowance only matters where a band is near 0: most coefficients stay within the plain bar
            plain = d <= 1e-9 * max(1.0, float(np.abs(y).max())) + 1e-9
            assert plain.mean() > 0.5, (name, float(plain.mean()))
        c.load_model_bytes(gs.dense_graph(g, seed=NAMES.index(name)))
        feat = c.kws_geom(audio, g)["feat"]
        _same(_int8(got, g.net_input_scale).reshape(feat.shape), feat, name + " int8 of the float64 output vs kws_geom")
        _same(feat, want, name + " kws_geom vs the oracle")
    finally:
        c.close()


def test_shipped_geometry_rounds_to_the_exact_kws_features():
    """audio/config.py's geometry and the shipped graph, 16 384 utterances: the int8 rounding of mfcc_geom is kws(exact=True)'s
    features and kws_geom's, bit for bit."""
    from edison_amd.context import Context
    c = Context(0)
    try:
        g = geom()
        audio = signals(16384, 32000, 11)
        y = c.mfcc_geom(audio, g)
        assert y.shape == (16384, 31, 13)
        mine = _int8(y, g.net_input_scale).reshape(16384, 403)
        _same(mine, c.kws(audio, n_utt=audio.shape[0], utt_stride=32000, exact=True)["feat"], "kws(exact=True) feat")
        _same(mine, c.kws_geom(audio, g)["feat"], "kws_geom feat")
    finally:
        c.close()


CASES = ["shipped"] + sorted(GEOMS)


def _case(name):
    return geom() if name == "shipped" else geom(**GEOMS[name])


@pytest.mark.parametrize("name", CASES)
def test_dataset_features_in_one_call(oracle_mod, name):
    """dataset_features(x, geometry=g): the per-utterance oracle, scaled by g.net_input_scale and clipped, within the bar; equal to the
    host form of the same one call; [n, F, num_mfcc, 1] float64; rows longer than n_samples use their first n_samples; no rows, no
    features."""
    from edison_amd import config as cfg
    from edison_amd.context import Context
    from edison_amd.kws.features import dataset_features
    g = _case(name)
    x = signals(40, g.n_samples + 37, 5 + CASES.index(name))
    c = Context(0, model_path=None)
    try:
        got = dataset_features(x, geometry=g, ctx=c)
        assert got.shape == (40, g.frame_count, g.num_mfcc, 1) and got.dtype == np.float64
        y = gs.oracle_mfcc(oracle_mod, x, g)
        want = np.clip(y * g.net_input_scale, cfg.nnom_net_input_clip_min, cfg.nnom_net_input_clip_max)
        _near(got[..., 0], want, name + " dataset_features vs the oracle")
        host = c.mfcc_geom(np.ascontiguousarray(x[:, :g.n_samples]), g)
        one = np.clip(host * g.net_input_scale, cfg.nnom_net_input_clip_min, cfg.nnom_net_input_clip_max)
        assert np.array_equal(got[..., 0], one), name + " dataset_features vs the host call"
        empty = dataset_features(np.zeros((0, g.n_samples), np.int16), geometry=g, ctx=c)
        assert empty.shape == (0, g.frame_count, g.num_mfcc, 1) and empty.dtype == np.float64
    finally:
        c.close()


@pytest.mark.parametrize("name", ["n1200_m40", "n1280"])
def test_device_form_on_a_side_stream(name):
    """mfcc_geom_t on a torch side stream (a wavefront-team row, a workgroup-team row), interleaved with kws_geom_t at the same geometry
    and a second mfcc_geom_t, without a synchronisation in between: every output equals the host forms."""
    import torch
    from edison_amd.context import Context
    g, audio, y, want = gs.row_data(name)
    c = Context(0, model_path=None)
    try:
        c.load_model_bytes(gs.dense_graph(g, seed=NAMES.index(name)))
        host = c.mfcc_geom(audio, g)
        feat_host = c.kws_geom(audio, g)["feat"]
        dev = torch.device("cuda", c.device)
        s = torch.cuda.Stream(dev)
        n = audio.shape[0]
        with torch.cuda.stream(s):
            a = torch.from_numpy(audio).to(dev)
            out = torch.full((n, g.frame_count, g.num_mfcc), float("nan"), dtype=torch.float64, device=dev)
            out2 = torch.full_like(out, float("nan"))
            feat = torch.zeros((n, g.n_features), dtype=torch.int8, device=dev)
            logits = torch.zeros((n, 4), dtype=torch.int8, device=dev)
            am = torch.zeros(n, dtype=torch.int32, device=dev)
            c.use_torch_stream(s)
            c.mfcc_geom_t(a, g, n, g.n_samples, out)
            c.kws_geom_t(a, g, n, g.n_samples, feat, logits, None, am)
            c.mfcc_geom_t(a, g, n, g.n_samples, out2)
        s.synchronize()
        c.use_own_stream()
        assert np.array_equal(out.cpu().numpy(), host), name + " device form"
        assert np.array_equal(out2.cpu().numpy(), host), name + " device form after kws_geom_t"
        _same(feat.cpu().numpy(), feat_host, name + " kws_geom_t between")
        _same(feat_host, want, name + " kws_geom vs the oracle")
    finally:
        c.close()


def _call(c, g, x, n_utt, stride, out):
    """edison_mfcc_geom_batch on an edison_kws_geom record g (host arrays or None)."""
    return c._L.edison_mfcc_geom_batch(c._h, ctypes.byref(g), None if x is None else x.ctypes.data_as(ctypes.c_void_p), int(n_utt), int(stride),
                                       None if out is None else out.ctypes.data_as(ctypes.c_void_p))


def test_errors_and_state():
    """Every code of the geometry checks is reachable; no model is not an error; a NULL output with utterances is EDISON_E_ARGUMENT in
    both forms, n_utt = 0 is a no-op (NULL pointers included); more than 2^31 frames is refused before any work; after an error the next
    call is right, and alternating two geometries (a table rebuild each time) leaves both right."""
    from edison_amd import _lib
    from edison_amd.context import Context
    ga, audio_a, y_a, _ = gs.row_data("n1200_m40")
    gb, audio_b, y_b, _ = gs.row_data("n4093")
    audio_a, audio_b = audio_a[:6], audio_b[:3]
    c = Context(0, model_path=None)
    try:
        want_a, want_b = c.mfcc_geom(audio_a, ga), c.mfcc_geom(audio_b, gb)
        _near(want_a, y_a[:6], "n1200_m40")
        _near(want_b, y_b[:3], "n4093")
        x = np.zeros(50000, np.int16)
        out = np.zeros(50000 * 8)
        base = geom(frame_len=400, frame_step=160, n_samples=16000, mel_nbins=40, num_mfcc=13)

        def code(**changes):
            g = base.to_ctypes()
            for k, v in changes.items():
                setattr(g, k, v)
            return _call(c, g, x, 1, 16000, out)

        assert code() == _lib.OK
        assert code(variant=_lib.MFCC_TF) == _lib.E_NO_IMPL
        assert code(variant=_lib.MFCC_C) == _lib.E_NO_IMPL
        assert code(variant=_lib.MFCC_B | 0x200) == _lib.E_ARGUMENT
        assert code(variant=_lib.MFCC_A | _lib.MFCC_USE_LOG) == _lib.E_ARGUMENT
        assert code(frame_len=3) == _lib.E_NO_IMPL and code(frame_len=4097) == _lib.E_NO_IMPL
        assert code(mel_nbins=0) == _lib.E_NO_IMPL and code(mel_nbins=257) == _lib.E_NO_IMPL
        assert code(frame_step=0) == _lib.E_ARGUMENT
        assert code(n_samples=399) == _lib.E_ARGUMENT
        assert code(frame_count=-1) == _lib.E_ARGUMENT
        assert code(frame_count=100) == _lib.E_ARGUMENT   # 98 fit
        assert code(first_mfcc=-1) == _lib.E_ARGUMENT and code(num_mfcc=0) == _lib.E_ARGUMENT
        assert code(first_mfcc=30, num_mfcc=11) == _lib.E_ARGUMENT
        for bad in (dict(sample_rate=0.0), dict(lower_edge_hertz=-1.0), dict(upper_edge_hertz=10.0), dict(mel_mtx_scale=0.0),
                    dict(sample_rate=float("inf")), dict(net_input_scale=float("nan"))):
            assert code(**bad) == _lib.E_ARGUMENT, bad
        gc = base.to_ctypes()
        assert _call(c, gc, x, 1, 16000, None) == _lib.E_ARGUMENT
        assert c._L.edison_mfcc_geom_batch_dev(c._h, ctypes.byref(gc), x.ctypes.data_as(ctypes.c_void_p), 1, 16000, None) == _lib.E_ARGUMENT
        assert _call(c, gc, None, 0, 16000, None) == _lib.OK
        assert c._L.edison_mfcc_geom_batch_dev(c._h, ctypes.byref(gc), None, 0, 16000, None) == _lib.OK
        assert _call(c, gc, x, 1, -1, out) == _lib.E_ARGUMENT
        # 98 frames per utterance: 2^31 / 98 + 1 utterances are refused before the device is touched (stride 0: one utterance's samples)
        assert c._L.edison_mfcc_geom_batch_dev(c._h, ctypes.byref(gc), x.ctypes.data_as(ctypes.c_void_p), (1 << 31) // 98 + 1, 0,
                                               out.ctypes.data_as(ctypes.c_void_p)) == _lib.E_ARGUMENT
        with pytest.raises(_lib.EdisonError):
            c.mfcc_geom(audio_a, geom(frame_len=5000, frame_step=5000, n_samples=16000))
        for _ in range(2):
            assert np.array_equal(c.mfcc_geom(audio_a, ga), want_a)
            assert np.array_equal(c.mfcc_geom(audio_b, gb), want_b)
    finally:
        c.close()

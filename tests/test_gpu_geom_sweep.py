"""GPU tests (-m gpu) of the any-geometry MFCC kernels over the whole range they accept, at the rows of tests/geom_sweep.py: every team
(wavefront / workgroup) x transform (packed Stockham, odd Stockham, direct DFT) of ed_mfcc_geom_kernel, radices 2 / 3 / 4 / 5 in both
teams, frame_len 4 .. 4096, mel_nbins 1 .. 256, fs 8 / 16 / 44.1 / 48 kHz, an upper edge above Nyquist, DCT rows from the end.

Each row runs at a net_input_scale (a power of two, exact in float32) that puts the 99th percentile of its oracle coefficients near
the int8 limit, so a relative error of 1e-5 anywhere in the float64 chain moves features by an int8 step; a guard checks that at least
half of the row's features are neither 0 nor clipped and that they follow the signal (tests/test_geom_sweep_cpu.py). The references are float64: oracle.mfcc_numpy + oracle.net_input for the int8
features (bit for bit), numpy's FFT and the oracle's mel matrix for edison_mfcc_generic's intermediate outputs (test_gpu_generic's
1e-9 bar)."""
import numpy as np
import pytest

import geom_sweep as gs

pytestmark = pytest.mark.gpu

NAMES = sorted(gs.ROWS)
WORKGROUP_ROWS = [n for n in NAMES if gs.row_plan(n)["team"] == 256]


def _findings(got, want, y, g, limit=8):
    """The differing features: utterance, frame, coefficient, the two int8 values and the oracle's float32 value's distance to x.5."""
    out = []
    for u, i in np.argwhere(got != want)[:limit]:
        f, k = divmod(int(i), g.num_mfcc)
        v = float(np.float32(y[u, f, k]) * np.float32(g.net_input_scale))
        out.append(dict(utt=int(u), frame=f, coef=g.first_mfcc + k, got=int(got[u, i]), oracle=int(want[u, i]), value=round(v, 6),
                        to_boundary=round(abs(abs(v - np.floor(v)) - 0.5), 6)))
    return out


def _same_feat(got, want, y, g, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    n = int((got != want).sum())
    assert n == 0, "%s: %d of %d features differ: %s" % (what, n, want.size, _findings(got, want, y, g))


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d differences, first at %s" % (what, bad.shape[0], bad[:5].tolist())


def _near_plus(got, ref, extra, what):
    """test_gpu_generic._near's bar, 1e-9 of the array's largest value + 1e-9, plus a per-element allowance `extra`."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tol = 1e-9 * max(1.0, float(np.abs(ref).max())) + 1e-9 + extra
    d = np.abs(got - ref)
    assert (d <= tol).all(), "%s: max |d| - tol %.3e at %s" % (what, float((d - tol).max()), np.unravel_index(np.argmax(d - tol), d.shape))


def _load(c, name, g):
    c.load_model_bytes(gs.dense_graph(g, seed=sorted(gs.ROWS).index(name)))


@pytest.mark.parametrize("name", NAMES)
def test_geometry_kernel_equals_the_oracle(name):
    """ed_mfcc_geom_kernel's int8 features equal the float64 oracle's bit for bit; the graph's logits and argmax equal ctx.net on the
    oracle's features. Workgroup-team rows also run the device form on a torch side stream."""
    from edison_amd.context import Context
    g, audio, y, want = gs.row_data(name)
    c = Context(0, model_path=None)
    try:
        _load(c, name, g)
        r = c.kws_geom(audio, g)
        _same_feat(r["feat"], want, y, g, name + " features")
        o = c.net(want)
        _same(r["logits"], o["logits"], name + " logits")
        _same(r["argmax"], o["argmax"], name + " argmax")
        assert r["softmax"] is None
        if name in WORKGROUP_ROWS:
            import torch
            dev = torch.device("cuda", c.device)
            s = torch.cuda.Stream(dev)
            n = audio.shape[0]
            with torch.cuda.stream(s):
                a = torch.from_numpy(audio).to(dev)
                feat = torch.zeros((n, g.n_features), dtype=torch.int8, device=dev)
                logits = torch.zeros((n, 4), dtype=torch.int8, device=dev)
                am = torch.zeros(n, dtype=torch.int32, device=dev)
                c.use_torch_stream(s)
                c.kws_geom_t(a, g, n, g.n_samples, feat, logits, None, am)
            s.synchronize()
            c.use_own_stream()
            _same_feat(feat.cpu().numpy(), want, y, g, name + " device form features")
            _same(logits.cpu().numpy(), o["logits"], name + " device form logits")
            _same(am.cpu().numpy(), o["argmax"], name + " device form argmax")
    finally:
        c.close()


def _generic(c, x, g, n_coef=None):
    """edison_mfcc_generic over one utterance's frames with all five float64 outputs and the int8 features of DCT rows 0 .. n_coef-1."""
    from edison_amd import _lib
    F, N, nm = g.frame_count, g.frame_len, g.mel_nbins
    fo = N // 2 if g.variant == _lib.MFCC_A else N
    n_coef = g.first_mfcc + g.num_mfcc if n_coef is None else n_coef
    x = np.ascontiguousarray(x)
    out = dict(fft=np.zeros((F, fo, 2)), spec=np.zeros((F, fo)), mel=np.zeros((F, nm)), logmel=np.zeros((F, nm)), mfcc=np.zeros((F, nm)),
               feat=np.zeros((F, n_coef), np.int8))
    variant = g.to_ctypes().variant
    r = c._L.edison_mfcc_generic(c._h, x.ctypes.data, F, N, g.frame_step, variant, nm, g.sample_rate, g.lower_edge_hertz, g.upper_edge_hertz,
                                 g.mel_mtx_scale, *[out[k].ctypes.data for k in ("fft", "spec", "mel", "logmel", "mfcc")], n_coef,
                                 out["feat"].ctypes.data, g.net_input_scale)
    assert r == _lib.OK, (c._L.edison_last_error(c._h) or b"").decode()
    return out


def _numpy_chain(x, g, W, D, dct_div):
    """numpy float64, frame by frame with oracle.mfcc_numpy's own expressions: fft and spectrogram as edison_mfcc_generic returns them
    (A: bins 0 .. N/2-1; B: all N, / 1024, |.| / sqrt 2), the mel bands and the MFCC (all mel_nbins rows)."""
    from edison_amd import _lib
    N, a_variant = g.frame_len, g.variant == _lib.MFCC_A
    nb = W.shape[0]
    Xs, specs, mels, ms = [], [], [], []
    for f in range(g.frame_count):
        X = np.fft.fft(x[f * g.frame_step:f * g.frame_step + N].astype(np.float64))
        if a_variant:
            X = X[:nb]
            spec = np.abs(X)
            e = spec @ W
            ms.append(D @ np.log(e + 1e-6) / dct_div)
        else:
            X = X / 1024.0
            spec = np.abs(X) / np.sqrt(2.0)
            e = (spec[:nb] @ (g.mel_mtx_scale * W)) / g.mel_mtx_scale
            ms.append(D @ (np.log(e + 1e-6) if g.use_log else e) / dct_div)
        Xs.append(X)
        specs.append(spec)
        mels.append(e)
    return np.array(Xs), np.array(specs), np.array(mels), np.array(ms)


@pytest.mark.parametrize("name", NAMES)
def test_generic_kernel_at_the_row(name):
    """edison_mfcc_generic at the row. fft, spectrogram and mel against numpy float64 (np.fft.fft, the oracle's mel matrix) within
    test_gpu_generic's bar, 1e-9 of each array's largest value + 1e-9. logmel and mfcc: within that bar of ln(its own mel + 1e-6) and
    of the DCT-II of its own logmel, and of oracle.mfcc_numpy's within that bar plus its measured mel difference carried through ln
    and the DCT (0 where the mels agree). Its int8 features equal the oracle's, and so the geometry kernel's."""
    from edison_amd import _lib
    from edison_amd.context import Context
    from oracle import oracle
    from test_gpu_generic import _near
    g, audio, y, want = gs.row_data(name)
    N, F, a_variant = g.frame_len, g.frame_count, g.variant == _lib.MFCC_A
    nb = N // 2 if a_variant else N // 2 + 1
    W = oracle.mel_weight_matrix(g.mel_nbins, nb, g.sample_rate, g.lower_edge_hertz, g.upper_edge_hertz)
    ov = oracle.VARIANT_A if a_variant else oracle.VARIANT_B
    nm = g.mel_nbins
    k = np.arange(nm)
    D = 2.0 * np.cos(np.pi * np.outer(k, 2 * np.arange(nm) + 1) / (2.0 * nm))   # oracle.mfcc_numpy's DCT-II matrix, expression for expression
    dct_div = np.sqrt(2.0 * nm) if a_variant else 64.0
    c = Context(0, model_path=None)
    try:
        for u in range(audio.shape[0]):
            x = audio[u, :(F - 1) * g.frame_step + N]
            o = _generic(c, x, g)
            X, spec, mel, m = _numpy_chain(x, g, W, D, dct_div)
            tag = "%s utt %d " % (name, u)
            _near(o["fft"], np.stack([X.real, X.imag], axis=-1), tag + "fft")
            _near(o["spec"], spec, tag + "spectrogram")
            _near(o["mel"], mel, tag + "mel")
            # `mel` is the very value oracle.mfcc_numpy takes the logarithm of
            assert np.array_equal(m, oracle.mfcc_numpy(x, ov, N, g.frame_step, n_frames=F, num_mel_bins=nm, sample_rate=g.sample_rate,
                                                       lower_edge_hertz=g.lower_edge_hertz, upper_edge_hertz=g.upper_edge_hertz,
                                                       mel_mtx_scale=g.mel_mtx_scale, use_log=g.use_log)), tag + "numpy chain"
            # the kernel's own chain, at the bar: logmel = ln(its mel + 1e-6) (variant B without log: its mel), mfcc = DCT-II of its logmel
            take_log = a_variant or g.use_log
            _near(o["logmel"], np.log(o["mel"] + 1e-6) if take_log else o["mel"], tag + "logmel of its mel")
            _near(o["mfcc"], o["logmel"] @ D.T / dct_div, tag + "mfcc of its logmel")
            # against the oracle, at the bar plus the kernel's measured mel difference carried through ln and the DCT: a band that is
            # exactly 0 in exact arithmetic (a constant frame's bins above DC) leaves each side 1e-12 of rounding residue, which
            # ln(e + 1e-6) turns into up to 5e-7; where the two mels agree the allowance is 0
            d_l = np.abs(np.log(o["mel"] + 1e-6) - np.log(mel + 1e-6)) if take_log else np.abs(o["mel"] - mel)
            _near_plus(o["logmel"], np.log(mel + 1e-6) if take_log else mel, d_l, tag + "logmel")
            _near_plus(o["mfcc"], m, d_l @ np.abs(D).T / dct_div, tag + "mfcc")
            _same_feat(o["feat"][:, g.first_mfcc:].reshape(1, -1), want[u:u + 1], y[u:u + 1], g, tag + "generic feat")
    finally:
        c.close()


# a wave-team FFT row, a workgroup FFT row, a workgroup direct row and a wave direct row
STATE_ROWS = ("n1200_m40", "n1280", "n4093", "n882_blog")


def test_state_across_kernel_instances():
    """One context cycles twice through STATE_ROWS, loading each row's graph, with fixed-shape ctx.mfcc and edison_mfcc_generic calls
    in between: every result is byte-equal to a fresh context's. Covers the table-cache rebuild and the switch between the wave and
    workgroup instances with their different LDS sizes."""
    from edison_amd.context import Context
    rows = {n: gs.row_data(n) for n in STATE_ROWS}
    cut = {n: rows[n][1][:10] for n in STATE_ROWS}
    fixed = gs.row_signals("n1280", gs.geometry("n1280"), 62)[2, :].copy()
    fixed = np.concatenate([fixed, fixed])[:32000]
    gen_g = gs.geometry("n375", net_input_scale=rows["n1280"][0].net_input_scale)

    def run(c, n):
        g = rows[n][0]
        _load(c, n, g)
        return c.kws_geom(cut[n], g)

    want = {}
    for n in STATE_ROWS:
        f = Context(0, model_path=None)
        try:
            want[n] = run(f, n)
        finally:
            f.close()
    f = Context(0)
    try:
        want_mfcc = f.mfcc(fixed)
        want_gen = _generic(f, cut["n1280"][3], gen_g)
    finally:
        f.close()
    c = Context(0)
    try:
        for step in range(2):
            for n in STATE_ROWS:
                r = run(c, n)
                for k in ("feat", "logits", "argmax"):
                    assert r[k].tobytes() == want[n][k].tobytes(), (step, n, k)
                assert c.mfcc(fixed).tobytes() == want_mfcc.tobytes(), (step, n, "mfcc")
                gen = _generic(c, cut["n1280"][3], gen_g)
                for k in want_gen:
                    assert gen[k].tobytes() == want_gen[k].tobytes(), (step, n, "generic " + k)
    finally:
        c.close()

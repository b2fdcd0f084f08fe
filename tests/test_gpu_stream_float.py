"""GPU tests (-m gpu) of continuous keyword spotting with float32 X-CUBE-AI networks (edison_stream_float_*, stream.FloatStream,
kws_live.run(..., net=)). Networks: the reference's own (tests/golden/cube_kws.ednf) in the host flow and in the firmware's q15 flow, and
three networks generated in X-CUBE-AI's format (tests/cube_synth.py) at geometries of test_gpu_kws_geom.GEOMS: kws_small (hop longer
than the frame), square (frame longer than the hop) and odd_no_softmax's (the direct-DFT path). The reference answers are the batch call
(Context.kws_float) on the zero-led recording, and tests/fnet_host.py on windows built on the host; everything is compared bit for bit."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_kws_geom import GEOMS, _geom, _same
from test_gpu_stream_geom import _filter_ref, _recording, _tail

import cube_synth
import fnet_host

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "cube_kws.ednf")
NETS = ["shipped", "shipped_q15", "kws_small", "square", "odd_no_softmax"]
SYNTH = [("conv", 8, (3, 3), (1, 1), (2, 2), 1), ("dense", 16), ("relu",), ("dense", 6), ("softmax",)]
OUTS = ("logits", "probs", "argmax")


@functools.lru_cache(maxsize=None)
def _blob(name):
    """The .ednf bytes of a network and its geometry."""
    from edison_amd import config as cfg
    from edison_amd.kws.geometry import KwsGeometry
    if name.startswith("shipped"):
        return open(FIXTURE, "rb").read(), KwsGeometry.from_config(net_input_scale=cfg.net_input_scale)
    g = _geom(**GEOMS[name])
    return _import(cube_synth.cube_sources((g.frame_count, g.num_mfcc, 1), SYNTH, seed=len(name))), g


def _import(sources):
    """(net_c, data_c) in X-CUBE-AI's format -> .ednf bytes."""
    import tempfile
    from edison_amd import cube_import
    with tempfile.TemporaryDirectory() as d:
        for fname, text in zip(("n.c", "n_data.c"), sources):
            with open(os.path.join(d, fname), "w") as f:
                f.write(text)
        return cube_import.import_files(os.path.join(d, "n.c"), os.path.join(d, "n_data.c"))


def _open(name):
    """(context with the float network loaded, geometry, q15, the model dict of fnet_host)."""
    from edison_amd import cube_import
    from edison_amd.context import Context
    blob, g = _blob(name)
    c = Context(0, model_path=None)
    c.fnet_load(blob)
    return c, g, name.endswith("_q15"), cube_import.read_blob(blob)


def _stream(c, g, q15, **kw):
    from edison_amd.stream import FloatStream
    return FloatStream(c, g, q15=q15, **kw)


def _dev_stream(c, g, q15, x, chunk, s=None, filt=False, alpha=0.5):
    """Device pushes of `chunk` frames, a ragged last push through push_n_dev; returns the outputs (and the filtered ones)."""
    import torch
    dev = torch.device("cuda", c.device)
    own = s is None
    s = s or _stream(c, g, q15, chunk_frames=chunk, output_filter=filt, alpha=alpha)
    no = s.n_out
    K = x.shape[0] // g.frame_step
    xt = torch.from_numpy(x).to(dev)
    lo = torch.zeros((K, no), dtype=torch.float32, device=dev)
    pr = torch.zeros((K, no), dtype=torch.float32, device=dev)
    am = torch.zeros(K, dtype=torch.int32, device=dev)
    fl = torch.zeros((K, no), dtype=torch.float32, device=dev) if filt else None
    li = torch.zeros(K, dtype=torch.int32, device=dev) if filt else None
    sp = torch.zeros(K, dtype=torch.int32, device=dev) if filt else None
    h = g.frame_step
    c.use_torch_stream(torch.cuda.current_stream(dev))
    try:
        for k0 in range(0, K, chunk):
            n = min(chunk, K - k0)
            sl = slice(k0, k0 + n)
            kw = dict(logits=lo[sl], probs=pr[sl], argmax=am[sl])
            if filt:
                kw.update(filtered=fl[sl], likely=li[sl], spotted=sp[sl])
            s.push_t(xt[k0 * h:(k0 + n) * h], n_frames=None if n == chunk else n, **kw)
        torch.cuda.synchronize(dev)
    finally:
        c.use_own_stream()
    if own:
        s.close()
    out = dict(logits=lo.cpu().numpy(), probs=pr.cpu().numpy(), argmax=am.cpu().numpy())
    if filt:
        out.update(filtered=fl.cpu().numpy(), likely=li.cpu().numpy(), spotted=sp.cpu().numpy())
    return out


def _host_pushes(s, x, n):
    parts = [s.push(x[i * s.chunk * s.hop:(i + 1) * s.chunk * s.hop]) for i in range(n)]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if isinstance(parts[0][k], np.ndarray)}


def _batch(c, g, q15, x, n_utt=None):
    """Context.kws_float on the zero-led recording, one utterance per full window (utt_stride = frame_step)."""
    z = np.concatenate([np.zeros(_tail(g), np.int16), x])
    K = x.shape[0] // g.frame_step
    return c.kws_float(z, g, q15=q15, n_utt=K - g.frame_count + 1 if n_utt is None else n_utt, utt_stride=g.frame_step)


def _same_outputs(got, want, what):
    for k in OUTS:
        _same(got[k], want[k], what + " " + k)


@pytest.mark.parametrize("name", NETS)
def test_full_windows_equal_the_batch_call(built_lib, name):
    """Outputs F - 1 .. of a long stream -- chunk 512, 20 device pushes (the buffers wrap several times), a ragged last one -- equal one
    kws_float batch call with utt_stride = frame_step on the same zero-led recording."""
    c, g, q15, _ = _open(name)
    try:
        K = 512 * 19 + 37
        x = _recording(g, K, 31 + len(name))
        got = _dev_stream(c, g, q15, x, 512)
        want = _batch(c, g, q15, x)
        F = g.frame_count
        _same_outputs({k: v[F - 1:] for k, v in got.items()}, want, name)
    finally:
        c.close()


@pytest.mark.parametrize("name", NETS)
def test_every_output_equals_the_exact_model(built_lib, name):
    """Every output, the F - 1 partial windows included, equals tests/fnet_host.py on windows built on the host from F - 1 zero rows and
    the batch call's feature rows (logits); probs and argmax equal the network alone (Context.fnet) on those windows."""
    c, g, q15, model = _open(name)
    try:
        F, nm = g.frame_count, g.num_mfcc
        K = F + 100
        x = _recording(g, K, 17 + len(name))
        got = _dev_stream(c, g, q15, x, 7)
        feat = _batch(c, g, q15, x)["feat"].reshape(-1, F, nm)
        rows = np.concatenate([feat[0], feat[1:, F - 1]])                       # frames 0 .. K - 1
        assert rows.shape == (K, nm)
        r = np.concatenate([np.zeros((F - 1, nm), np.float32), rows])
        win = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(r, (F, nm))[:, 0].reshape(K, -1))
        _same(got["logits"], fnet_host.run(model, win)[-1], name + " logits against the fmaf chain")
        alone = c.fnet(win)
        _same(got["probs"], alone["probs"], name + " probs")
        _same(got["argmax"], alone["argmax"], name + " argmax")
    finally:
        c.close()


@pytest.mark.parametrize("name", NETS)
def test_host_device_and_alternating_pushes_agree(built_lib, name):
    """Chunk-1 host pushes, chunk-7 device pushes, and chunk-7 pushes alternating between host and device (one history) agree."""
    c, g, q15, _ = _open(name)
    try:
        K = 7 * 12
        x = _recording(g, K, 55)
        want = _dev_stream(c, g, q15, x, 7)
        s = _stream(c, g, q15)
        _same_outputs(_host_pushes(s, x, K), want, name + " chunk-1 host pushes")
        assert s.frames_seen == K
        s.close()
        s = _stream(c, g, q15, chunk_frames=7)
        h = 7 * g.frame_step
        parts = []
        for i in range(K // 7):
            seg = x[i * h:(i + 1) * h]
            parts.append(s.push(seg) if i % 2 == 0 else _dev_stream(c, g, q15, seg, 7, s=s))
        _same_outputs({k: np.concatenate([p[k] for p in parts]) for k in OUTS}, want, name + " alternating pushes")
        assert s.frames_seen == K
        s.reset()
        assert s.frames_seen == 0
        _same_outputs(_host_pushes(s, x, K // 7), want, name + " host pushes after reset")
        s.close()
    finally:
        c.close()


@pytest.mark.parametrize("name", NETS)
def test_output_filter(built_lib, name):
    """filtered / likely / spotted equal the numpy recurrence (float32 state, double product and sum each rounded, first maximum) on the
    stream's probabilities, for host and device pushes, at alpha 0.5 (the Cube build's) and 0.9."""
    c, g, q15, _ = _open(name)
    try:
        K = 7 * 30
        x = _recording(g, K, 91)
        probs = _dev_stream(c, g, q15, x, 7)["probs"]
        for alpha in (0.5, 0.9):
            ref = _filter_ref(probs, alpha, 0.5)
            s = _stream(c, g, q15, chunk_frames=7, output_filter=True, alpha=alpha)
            host = _host_pushes(s, x, K // 7)
            s.close()
            d = _dev_stream(c, g, q15, x, 7, filt=True, alpha=alpha)
            for k, r in zip(("filtered", "likely", "spotted"), ref):
                _same(host[k], r, "%s alpha %g host %s" % (name, alpha, k))
                _same(d[k], r, "%s alpha %g device %s" % (name, alpha, k))
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "shipped_q15"])
def test_state_machine(built_lib, name):
    """fsm_states equal oracle/fsm_ref.walk on the filtered maxima, dt = floor(1024 * 1e6 / 16000) us; keyword names come from the .ednf;
    reset restarts the machine."""
    from oracle import fsm_ref
    c, g, q15, model = _open(name)
    try:
        K = 4 * 125
        x = _recording(g, K, 5)
        s = _stream(c, g, q15, chunk_frames=125, fsm=True)
        assert s.keywords == model["keywords"]
        for _ in range(2):
            outs = [s.push(x[i * 125 * 1024:(i + 1) * 125 * 1024]) for i in range(4)]
            filt = np.concatenate([o["filtered"] for o in outs])
            likely = np.concatenate([o["likely"] for o in outs])
            states, _ = fsm_ref.walk(filt[np.arange(K), likely], likely, 64000)
            _same(np.concatenate([o["fsm_states"] for o in outs]), np.array(states, np.int32), name + " fsm states")
            assert outs[0]["keywords"] == [model["keywords"][i] for i in outs[0]["argmax"]]
            s.reset()
        s.close()
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "shipped_q15"])
def test_edison_utterance_between_silences(built_lib, name):
    """The fixture's `edison` recording streamed between silences at a frame-aligned offset: at its full window p("edison") equals the
    reference's probability (probs_edison, q15_probs_edison) within 1e-5, and the class is edison."""
    golden = np.load(os.path.join(GOLDEN, "cube_golden.npz"))
    c, g, q15, _ = _open(name)
    try:
        a = 37
        x = np.concatenate([np.zeros(a * 1024, np.int16), golden["audio_edison"][:31 * 1024], np.zeros(40 * 1024, np.int16)])
        out = _dev_stream(c, g, q15, x, 16)
        k = a + g.frame_count - 1
        want = golden["q15_probs_edison" if q15 else "probs_edison"]
        assert abs(float(out["probs"][k, 0]) - want[0]) <= 1e-5
        assert out["argmax"][k] == 0
        np.testing.assert_allclose(out["probs"][k], want, rtol=0, atol=1e-5)
    finally:
        c.close()


def test_errors(built_lib):
    import ctypes
    from dataclasses import replace
    from edison_amd import _lib
    from edison_amd.context import Context
    from edison_amd.stream import FloatStream
    c = Context(0, model_path=None)
    try:
        blob, g = _blob("shipped")
        with pytest.raises(_lib.EdisonError) as e:
            FloatStream(c, g)
        assert e.value.code == _lib.E_NO_MODEL
        c.fnet_load(blob)
        for kw, code in ((dict(geometry=replace(g, num_mfcc=12)), _lib.E_SIZE),
                         (dict(geometry=replace(g, frame_len=512, frame_step=512, n_samples=16384), q15=True), _lib.E_NO_IMPL),
                         (dict(chunk_frames=0), _lib.E_ARGUMENT), (dict(chunk_frames=1 << 20), _lib.E_SIZE),
                         (dict(output_filter=True, alpha=1.5), _lib.E_ARGUMENT), (dict(output_filter=True, alpha=-0.1), _lib.E_ARGUMENT),
                         (dict(clip_min=1.0, clip_max=-1.0), _lib.E_ARGUMENT)):
            kw.setdefault("geometry", g)
            with pytest.raises(_lib.EdisonError) as e:
                FloatStream(c, **kw)
            assert e.value.code == code, kw
        # the C-ABI's defaults, and fsm without the filter (FloatStream turns the filter on)
        L = _lib.lib()
        o = _lib.StreamFloatOpts()
        L.edison_stream_float_default_opts(ctypes.byref(o))
        assert (o.chunk_frames, o.q15, o.clip_lo, o.clip_hi, o.filter, o.fsm, o.filter_alpha, o.true_threshold) == \
            (1, 0, -32768.0, 32767.0, 0, 0, 0.5, 0.5)
        o.fsm = 1
        h = ctypes.c_void_p()
        assert L.edison_stream_float_create(c._h, ctypes.byref(g.to_ctypes()), ctypes.byref(o), ctypes.byref(h)) == _lib.E_ARGUMENT
        # a push after edison_fnet_load replaced the network
        s = FloatStream(c, g)
        s.push(np.zeros(1024, np.int16))
        c.fnet_load(blob)
        with pytest.raises(_lib.EdisonError) as e:
            s.push(np.zeros(1024, np.int16))
        assert e.value.code == _lib.E_ARGUMENT
        s.close()
        # the state machine needs 10 outputs; the filter alone serves any count up to 256
        sblob, sg = _blob("square")
        c.fnet_load(sblob)
        with pytest.raises(_lib.EdisonError) as e:
            FloatStream(c, sg, fsm=True)
        assert e.value.code == _lib.E_NO_IMPL
        FloatStream(c, sg, output_filter=True).close()
        c.fnet_load(_import(cube_synth.cube_sources((1, 4, 1), [("dense", 300), ("softmax",)], seed=1)))   # 300 outputs
        wg = _geom(frame_len=256, frame_step=256, n_samples=256, mel_nbins=8, num_mfcc=4)
        FloatStream(c, wg).close()
        with pytest.raises(_lib.EdisonError) as e:
            FloatStream(c, wg, output_filter=True)
        assert e.value.code == _lib.E_NO_IMPL
    finally:
        c.close()


def test_kws_live_with_a_float_network(built_lib, tmp_path):
    """kws_live.run(..., net=) and `kws live host|mcu <wav> --net <file.ednf>`: one line per hop; FSM lines only for 10 outputs."""
    import contextlib
    import io
    import wave
    from edison_amd.context import Context
    from edison_amd.kws import kws_live

    def wav(x, p):
        with wave.open(p, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(x.tobytes())
        return p

    for name in ("shipped", "shipped_q15", "odd_no_softmax"):
        blob, g = _blob(name)
        x = _recording(g, 50, 2)
        p = wav(x, str(tmp_path / (name + ".wav")))
        c = Context(0, model_path=None)
        try:
            buf = io.StringIO()
            r = kws_live.run(p, q15=name.endswith("_q15"), ctx=c, out=buf, geometry=None if name.startswith("shipped") else g, net=blob)
            lines = buf.getvalue().splitlines()
            assert len(lines) == 50 and all(ln.startswith("pred: [") and " likely: " in ln for ln in lines)
            assert (r["state"] is not None) == name.startswith("shipped")
            assert all("class " in ln for ln in lines) == (name == "odd_no_softmax")
            # the filter ran at the Cube build's alpha 0.5 over the stream's probabilities
            s = _stream(c, g, name.endswith("_q15"), chunk_frames=50)
            probs = s.push(x)["probs"]
            s.close()
            _same(r["result"]["filtered"], _filter_ref(probs, 0.5, 0.5)[0], name + " live filter")
        finally:
            c.close()
    # the command line, on the default context
    p = wav(_recording(_blob("shipped")[1], 40, 3), str(tmp_path / "cli.wav"))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert kws_live.main(["live", "mcu", p, "--net", FIXTURE]) == 0
    assert len([ln for ln in buf.getvalue().splitlines() if ln.startswith("pred: [")]) == 40

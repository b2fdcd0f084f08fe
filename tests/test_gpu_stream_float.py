"""GPU tests (-m gpu) of continuous keyword spotting with float32 X-CUBE-AI networks (edison_stream_float_*, stream.FloatStream,
kws_live.run(..., net=)). Networks: the reference's own (tests/golden/cube_kws.ednf) in the host flow and in the firmware's q15 flow, and
three networks generated in X-CUBE-AI's format (tests/cube_synth.py) at geometries of geom_sweep.GEOMS: kws_small (hop longer
than the frame), square (frame longer than the hop) and odd_no_softmax's (the direct-DFT path). The reference answers are the batch call
(Context.kws_float) on the zero-led recording, and tests/fnet_host.py on windows built on the host; everything is compared bit for bit."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from geom_sweep import geom
from stream_drive import FIXTURE, Kind, cat, drive_stream, filter_ref, float_blob, host_pushes, import_sources, recording, same, tail, whole

import cube_synth
import fnet_host

pytestmark = pytest.mark.gpu

NETS = ["shipped", "shipped_q15", "kws_small", "square", "odd_no_softmax"]
OUTS = ("logits", "probs", "argmax")
KIND = Kind("float")


def _dev_stream(c, g, x, chunk, s=None, filt=False, alpha=None):
    """Device pushes of `chunk` frames, a ragged last push through push_n_dev; returns the outputs (and the filtered ones)."""
    return drive_stream(KIND, c, g, x, whole(x.shape[0] // g.frame_step, chunk), chunk=chunk, stream=s, filt=filt, alpha=alpha)[0]


def _host_pushes(s, x, n):
    return cat(KIND, host_pushes(s, x, n))


def _batch(c, g, q15, x, n_utt=None):
    """Context.kws_float on the zero-led recording, one utterance per full window (utt_stride = frame_step)."""
    z = np.concatenate([np.zeros(tail(g), np.int16), x])
    K = x.shape[0] // g.frame_step
    return c.kws_float(z, g, q15=q15, n_utt=K - g.frame_count + 1 if n_utt is None else n_utt, utt_stride=g.frame_step)


def _same_outputs(got, want, what):
    for k in OUTS:
        same(got[k], want[k], what + " " + k)


@pytest.mark.parametrize("name", NETS)
def test_full_windows_equal_the_batch_call(built_lib, name):
    """Outputs F - 1 .. of a long stream -- chunk 512, 20 device pushes (the buffers wrap several times), a ragged last one -- equal one
    kws_float batch call with utt_stride = frame_step on the same zero-led recording."""
    c, g = KIND.open(name)
    try:
        K = 512 * 19 + 37
        x = recording(g, K, 31 + len(name))
        got = _dev_stream(c, g, x, 512)
        want = _batch(c, g, KIND.q15, x)
        F = g.frame_count
        _same_outputs({k: v[F - 1:] for k, v in got.items()}, want, name)
    finally:
        c.close()


@pytest.mark.parametrize("name", NETS)
def test_every_output_equals_the_exact_model(built_lib, name):
    """Every output, the F - 1 partial windows included, equals tests/fnet_host.py on windows built on the host from F - 1 zero rows and
    the batch call's feature rows (logits); probs and argmax equal the network alone (Context.fnet) on those windows."""
    c, g = KIND.open(name)
    try:
        F, nm = g.frame_count, g.num_mfcc
        K = F + 100
        x = recording(g, K, 17 + len(name))
        got = _dev_stream(c, g, x, 7)
        feat = _batch(c, g, KIND.q15, x)["feat"].reshape(-1, F, nm)
        rows = np.concatenate([feat[0], feat[1:, F - 1]])                       # frames 0 .. K - 1
        assert rows.shape == (K, nm)
        r = np.concatenate([np.zeros((F - 1, nm), np.float32), rows])
        win = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(r, (F, nm))[:, 0].reshape(K, -1))
        same(got["logits"], fnet_host.run(KIND.model, win)[-1], name + " logits against the fmaf chain")
        alone = c.fnet(win)
        same(got["probs"], alone["probs"], name + " probs")
        same(got["argmax"], alone["argmax"], name + " argmax")
    finally:
        c.close()


@pytest.mark.parametrize("name", NETS)
def test_host_device_and_alternating_pushes_agree(built_lib, name):
    """Chunk-1 host pushes, chunk-7 device pushes, and chunk-7 pushes alternating between host and device (one history) agree."""
    c, g = KIND.open(name)
    try:
        K = 7 * 12
        x = recording(g, K, 55)
        want = _dev_stream(c, g, x, 7)
        s = KIND.stream(c, g, 1)
        _same_outputs(_host_pushes(s, x, K), want, name + " chunk-1 host pushes")
        assert s.frames_seen == K
        s.close()
        s = KIND.stream(c, g, 7)
        h = 7 * g.frame_step
        parts = []
        for i in range(K // 7):
            seg = x[i * h:(i + 1) * h]
            parts.append(s.push(seg) if i % 2 == 0 else _dev_stream(c, g, seg, 7, s=s))
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
    c, g = KIND.open(name)
    try:
        K = 7 * 30
        x = recording(g, K, 91)
        probs = _dev_stream(c, g, x, 7)["probs"]
        for alpha in (0.5, 0.9):
            ref = filter_ref(probs, alpha, 0.5)
            s = KIND.stream(c, g, 7, output_filter=True, alpha=alpha)
            host = _host_pushes(s, x, K // 7)
            s.close()
            d = _dev_stream(c, g, x, 7, filt=True, alpha=alpha)
            for k, r in zip(("filtered", "likely", "spotted"), ref):
                same(host[k], r, "%s alpha %g host %s" % (name, alpha, k))
                same(d[k], r, "%s alpha %g device %s" % (name, alpha, k))
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "shipped_q15"])
def test_state_machine(built_lib, name):
    """fsm_states equal oracle/fsm_ref.walk on the filtered maxima, dt = floor(1024 * 1e6 / 16000) us; keyword names come from the .ednf;
    reset restarts the machine."""
    from oracle import fsm_ref
    c, g = KIND.open(name)
    try:
        K = 4 * 125
        x = recording(g, K, 5)
        s = KIND.stream(c, g, 125, fsm=True)
        assert s.keywords == KIND.model["keywords"]
        for _ in range(2):
            outs = [s.push(x[i * 125 * 1024:(i + 1) * 125 * 1024]) for i in range(4)]
            filt = np.concatenate([o["filtered"] for o in outs])
            likely = np.concatenate([o["likely"] for o in outs])
            states, _ = fsm_ref.walk(filt[np.arange(K), likely], likely, 64000)
            same(np.concatenate([o["fsm_states"] for o in outs]), np.array(states, np.int32), name + " fsm states")
            assert outs[0]["keywords"] == [KIND.model["keywords"][i] for i in outs[0]["argmax"]]
            s.reset()
        s.close()
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "shipped_q15"])
def test_edison_utterance_between_silences(built_lib, name):
    """The fixture's `edison` recording streamed between silences at a frame-aligned offset: at its full window p("edison") equals the
    reference's probability (probs_edison, q15_probs_edison) within 1e-5, and the class is edison."""
    golden = np.load(os.path.join(GOLDEN, "cube_golden.npz"))
    c, g = KIND.open(name)
    try:
        a = 37
        x = np.concatenate([np.zeros(a * 1024, np.int16), golden["audio_edison"][:31 * 1024], np.zeros(40 * 1024, np.int16)])
        out = _dev_stream(c, g, x, 16)
        k = a + g.frame_count - 1
        want = golden["q15_probs_edison" if KIND.q15 else "probs_edison"]
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
        blob, g = float_blob("shipped")
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
        sblob, sg = float_blob("square")
        c.fnet_load(sblob)
        with pytest.raises(_lib.EdisonError) as e:
            FloatStream(c, sg, fsm=True)
        assert e.value.code == _lib.E_NO_IMPL
        FloatStream(c, sg, output_filter=True).close()
        c.fnet_load(import_sources(cube_synth.cube_sources((1, 4, 1), [("dense", 300), ("softmax",)], seed=1)))   # 300 outputs
        wg = geom(frame_len=256, frame_step=256, n_samples=256, mel_nbins=8, num_mfcc=4)
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
        blob, g = float_blob(name)
        x = recording(g, 50, 2)
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
            s = KIND.stream(c, g, 50, q15=name.endswith("_q15"))
            probs = s.push(x)["probs"]
            s.close()
            same(r["result"]["filtered"], filter_ref(probs, 0.5, 0.5)[0], name + " live filter")
        finally:
            c.close()
    # the command line, on the default context
    p = wav(recording(float_blob("shipped")[1], 40, 3), str(tmp_path / "cli.wav"))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert kws_live.main(["live", "mcu", p, "--net", FIXTURE]) == 0
    assert len([ln for ln in buf.getvalue().splitlines() if ln.startswith("pred: [")]) == 40

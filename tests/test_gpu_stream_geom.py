"""GPU tests (-m gpu) of continuous keyword spotting at any MFCC geometry (edison_stream_geom_*, stream.GeomStream). The reference answer
is the host flow restated frame by frame: with z = the recording behind T = max(0, frame_len - frame_step) zeros, frame k is
oracle.mfcc_numpy on z[k * frame_step:], its int8 row oracle.net_input; window k is rows k - F + 1 .. k with zero rows in front of the
recording; the graph runs on those windows through ctx.net. Graphs: the five committed alt_models at their geometry
(geom_sweep.GEOMS) and the shipped graph at edison_kws_geom_default. Everything is compared bit for bit."""
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

from geom_sweep import GEOMS, geom, header, signals
from stream_drive import Kind, drive_stream, filter_ref, oracle_rows, recording, same, tail, whole

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = ["shipped"] + sorted(GEOMS)
KIND = Kind("int8")


def _oracle_outputs(c, oracle_mod, g, x):
    rows = oracle_rows(oracle_mod, g, x)
    F = g.frame_count
    r = np.concatenate([np.zeros((F - 1, g.num_mfcc), np.int8), rows])
    win = np.lib.stride_tricks.sliding_window_view(r, (F, g.num_mfcc))[:, 0].reshape(rows.shape[0], -1)
    return c.net(np.ascontiguousarray(win))


def _dev_stream(c, g, x, chunk, s=None, filt=False):
    """Device pushes of `chunk` frames, a ragged last push through push_n_dev; returns the outputs (and the filtered ones)."""
    return drive_stream(KIND, c, g, x, whole(x.shape[0] // g.frame_step, chunk), chunk=chunk, stream=s, filt=filt)[0]


def _same_outputs(got, want, what):
    same(got["logits"], want["logits"], what + " logits")
    same(got["argmax"], want["argmax"], what + " argmax")
    if want["softmax"] is None:
        assert got["softmax"] is None, what
    else:
        same(got["softmax"], want["softmax"], what + " softmax")


@pytest.mark.parametrize("name", GRAPHS)
def test_device_pushes_equal_the_host_flow(oracle_mod, name):
    """Chunks 1, 7 and 512 with a ragged last push; chunks 1 and 7 wrap the sliding buffers many times (the shift kernel runs)."""
    c, g = KIND.open(name)
    try:
        x = recording(g, 300, 7 + len(name))
        want = _oracle_outputs(c, oracle_mod, g, x)
        for chunk in (1, 7, 512):
            _same_outputs(_dev_stream(c, g, x, chunk), want, "%s chunk %d" % (name, chunk))
    finally:
        c.close()


@pytest.mark.parametrize("name", GRAPHS)
def test_outputs_of_full_windows_equal_the_batch_call(name):
    """Outputs F - 1 .. of a long stream (chunk 512, the buffers wrapped several times) equal one kws_geom batch call with utt_stride =
    frame_step on the same zero-led recording."""
    c, g = KIND.open(name)
    try:
        K = 512 * 20 + 37
        x = recording(g, K, 31 + len(name))
        got = _dev_stream(c, g, x, 512)
        z = np.concatenate([np.zeros(tail(g), np.int16), x])
        F = g.frame_count
        n_utt = K - F + 1
        r = c.kws_geom(z, g, n_utt=n_utt, utt_stride=g.frame_step)
        for k in ("logits", "softmax", "argmax"):
            if r[k] is None:
                assert got[k] is None
            else:
                same(got[k][F - 1:], r[k], "%s %s" % (name, k))
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "square", "odd_no_softmax"])
def test_host_device_and_alternating_pushes_agree(oracle_mod, name):
    from edison_amd.stream import GeomStream
    c, g = KIND.open(name)
    try:
        chunk = 7
        K = 7 * 40
        x = recording(g, K, 55)
        want = _oracle_outputs(c, oracle_mod, g, x)
        h = g.frame_step * chunk
        s = GeomStream(c, g, chunk_frames=chunk)
        host = [s.push(x[i * h:(i + 1) * h]) for i in range(K // chunk)]
        got = {k: (None if host[0][k] is None else np.concatenate([o[k] for o in host])) for k in ("logits", "softmax", "argmax")}
        _same_outputs(got, want, name + " host pushes")
        assert s.frames_seen == K
        # alternate: even pushes from the host, odd pushes on the device, one history
        s.reset()
        assert s.frames_seen == 0
        parts = []
        for i in range(K // chunk):
            seg = x[i * h:(i + 1) * h]
            if i % 2 == 0:
                parts.append(s.push(seg))
            else:
                parts.append(_dev_stream(c, g, seg, chunk, s=s))
        got = {k: (None if parts[0][k] is None else np.concatenate([o[k] for o in parts])) for k in ("logits", "softmax", "argmax")}
        _same_outputs(got, want, name + " alternating pushes")
        s.close()
    finally:
        c.close()


def _route_outputs(c, g, x):
    return _dev_stream(c, g, x, 7)


@pytest.mark.parametrize("name", ["shipped", "square", "odd_no_softmax", "kws_small"])
def test_every_network_route(oracle_mod, name):
    """The default route, the general matrix-core kernel (EDISON_NET_FORCE_GENERAL for the shipped graph), the graph's own kernel
    (edison_net_specialize, where a compiler exists) and, in a child process with EDISON_NET_NO_MFMA=1, the layer-by-layer kernel."""
    from edison_amd import _lib
    c, g = KIND.open(name)
    try:
        x = recording(g, 120, 77)
        want = _oracle_outputs(c, oracle_mod, g, x)
        _same_outputs(_route_outputs(c, g, x), want, name + " default route")
        os.environ["EDISON_NET_FORCE_GENERAL"] = "1"
        try:
            _same_outputs(_route_outputs(c, g, x), want, name + " general matrix-core kernel")
            try:
                c.net_specialize()
                _same_outputs(_route_outputs(c, g, x), want, name + " own kernel")
            except _lib.EdisonError as e:
                assert e.code == _lib.E_NO_IMPL
        finally:
            del os.environ["EDISON_NET_FORCE_GENERAL"]
    finally:
        c.close()


def test_layer_by_layer_route_in_a_child_process(oracle_mod, tmp_path):
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_stream_geom as t
out = {}
for name in ("shipped", "square", "odd_no_softmax"):
    c, g = t.KIND.open(name)
    x = t.recording(g, 120, 77)
    r = t._dev_stream(c, g, x, 7)
    for k, v in r.items():
        if v is not None:
            out[name + "/" + k] = v
    c.close()
np.savez(%r, **out)
print("child ok")
""" % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "lbl.npz"))
    env = dict(os.environ, EDISON_NET_NO_MFMA="1", EDISON_NET_FORCE_GENERAL="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.load(tmp_path / "lbl.npz")
    for name in ("shipped", "square", "odd_no_softmax"):
        c, g = KIND.open(name)
        try:
            x = recording(g, 120, 77)
            want = _oracle_outputs(c, oracle_mod, g, x)
            sub = {k: (got[name + "/" + k] if name + "/" + k in got else None) for k in ("logits", "softmax", "argmax")}
            _same_outputs(sub, want, name + " layer-by-layer kernel")
        finally:
            c.close()


@pytest.mark.parametrize("name", GRAPHS)
def test_output_filter(oracle_mod, name):
    """filtered / likely / spotted equal the numpy recurrence on the host flow's outputs (softmax, or logits without Softmax), for host
    pushes and device pushes; alpha and threshold away from the defaults too."""
    from edison_amd.stream import GeomStream
    c, g = KIND.open(name)
    try:
        K = 7 * 30
        x = recording(g, K, 91)
        want = _oracle_outputs(c, oracle_mod, g, x)
        xin = want["softmax"] if want["softmax"] is not None else want["logits"]
        for alpha, thr in ((0.9, 0.5), (0.6, 3.0)):
            ref = filter_ref(xin, alpha, thr)
            s = GeomStream(c, g, chunk_frames=7, output_filter=True, alpha=alpha, threshold=thr)
            h = 7 * g.frame_step
            outs = [s.push(x[i * h:(i + 1) * h]) for i in range(K // 7)]
            for k, r in zip(("filtered", "likely", "spotted"), ref):
                same(np.concatenate([o[k] for o in outs]), r, "%s host %s" % (name, k))
            assert ("keywords" in outs[0]) == (c.net_info()["n_out"] == 10)
            s.close()
            s = GeomStream(c, g, chunk_frames=7, output_filter=True, alpha=alpha, threshold=thr)
            d = _dev_stream(c, g, x, 7, s=s, filt=True)
            s.close()
            for k, r in zip(("filtered", "likely", "spotted"), ref):
                same(d[k], r, "%s device %s" % (name, k))
    finally:
        c.close()


def test_state_machine_at_the_shipped_geometry(oracle_mod):
    """fsm_states of the shipped-geometry stream equal oracle/fsm_ref.walk on the filtered maxima, dt = 1024 / 16 kHz; reset restarts
    the machine."""
    from oracle import fsm_ref
    from edison_amd.stream import GeomStream
    c, g = KIND.open("shipped")
    try:
        K = 4 * 250
        x = recording(g, K, 5)
        s = GeomStream(c, g, chunk_frames=250, fsm=True)
        for _ in range(2):
            outs = [s.push(x[i * 250 * 1024:(i + 1) * 250 * 1024]) for i in range(4)]
            filt = np.concatenate([o["filtered"] for o in outs])
            likely = np.concatenate([o["likely"] for o in outs])
            states, _ = fsm_ref.walk(filt[np.arange(K), likely], likely, 64000)
            same(np.concatenate([o["fsm_states"] for o in outs]), np.array(states, np.int32), "fsm states")
            s.reset()
        s.close()
    finally:
        c.close()


def test_reset_batch_calls_and_frames_seen(oracle_mod):
    """reset reproduces a fresh stream; kws_geom batch calls at another geometry on the same context between pushes change nothing;
    frames_seen counts frames, ragged pushes included."""
    import torch
    from edison_amd.stream import GeomStream
    c, g = KIND.open("shipped")
    try:
        x = recording(g, 70, 13)
        fresh = _dev_stream(c, g, x, 7)
        s = GeomStream(c, g, chunk_frames=7)
        _dev_stream(c, g, x[:33 * 1024], 7, s=s)
        assert s.frames_seen == 33
        s.reset()
        assert s.frames_seen == 0
        # a batch call at another geometry between every two pushes: the context's table cache flips, the stream's tables stay
        other = geom(frame_len=512, frame_step=256, n_samples=512 + 30 * 256, mel_nbins=20, num_mfcc=13)
        noise = signals(4, other.n_samples, 3)
        dev = torch.device("cuda", c.device)
        lo = []
        for i in range(10):
            seg = x[i * 7 * 1024:(i + 1) * 7 * 1024]
            lo.append(_dev_stream(c, g, seg, 7, s=s)["logits"])
            c.kws_geom(noise, other)
        same(np.concatenate(lo), fresh["logits"], "logits after reset with interleaved batch calls")
        assert s.frames_seen == 70
        s.close()
        torch.cuda.synchronize(dev)
    finally:
        c.close()


def test_errors():
    from edison_amd import _lib
    from edison_amd.context import Context
    from edison_amd.stream import GeomStream
    c = Context(0, model_path=None)
    try:
        g = geom()
        with pytest.raises(_lib.EdisonError) as e:
            GeomStream(c, g)
        assert e.value.code == _lib.E_NO_MODEL
        c.load_model(_lib.DEFAULT_MODEL)
        for bad, code in ((dict(frame_len=8192), _lib.E_NO_IMPL), (dict(mel_nbins=300), _lib.E_NO_IMPL), (dict(frame_step=0), _lib.E_ARGUMENT),
                          (dict(variant=_lib.MFCC_C), _lib.E_NO_IMPL), (dict(num_mfcc=12), _lib.E_SIZE)):
            with pytest.raises(_lib.EdisonError) as e:
                GeomStream(c, replace(g, **bad))
            assert e.value.code == code, bad
        for kw, code in ((dict(chunk_frames=0), _lib.E_ARGUMENT), (dict(chunk_frames=1 << 20), _lib.E_SIZE),
                         (dict(output_filter=True, alpha=1.5), _lib.E_ARGUMENT)):
            with pytest.raises(_lib.EdisonError) as e:
                GeomStream(c, g, **kw)
            assert e.value.code == code, kw
        # fsm without the filter: only reachable through the C-ABI (GeomStream turns the filter on)
        import ctypes
        L = _lib.lib()
        o = _lib.StreamGeomOpts()
        L.edison_stream_geom_default_opts(ctypes.byref(o))
        assert (o.chunk_frames, o.filter, o.fsm, o.filter_alpha, o.true_threshold) == (1, 0, 0, 0.9, 0.5)
        o.fsm = 1
        h = ctypes.c_void_p()
        assert L.edison_stream_geom_create(c._h, ctypes.byref(g.to_ctypes()), ctypes.byref(o), ctypes.byref(h)) == _lib.E_ARGUMENT
        # a push after a model reload
        s = GeomStream(c, g)
        s.push(np.zeros(1024, np.int16))
        c.load_model(_lib.DEFAULT_MODEL)
        with pytest.raises(_lib.EdisonError) as e:
            s.push(np.zeros(1024, np.int16))
        assert e.value.code == _lib.E_ARGUMENT
        s.close()
        # the state machine needs 10 outputs
        c.load_weights_h(header("same_stride"))    # 5 outputs
        gs = geom(**GEOMS["same_stride"])
        with pytest.raises(_lib.EdisonError) as e:
            GeomStream(c, gs, fsm=True)
        assert e.value.code == _lib.E_NO_IMPL
        GeomStream(c, gs, output_filter=True).close()
    finally:
        c.close()


def test_kws_live_with_a_geometry(tmp_path):
    """kws_live.run on a wav with a retrained graph's geometry: one line per hop; FSM lines only for a graph with 10 outputs."""
    import io
    import wave
    from edison_amd.kws import kws_live
    for name in ("shipped", "odd_no_softmax"):
        c, g = KIND.open(name)
        try:
            x = recording(g, 50, 2)
            p = str(tmp_path / (name + ".wav"))
            with wave.open(p, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes(x.tobytes())
            buf = io.StringIO()
            r = kws_live.run(p, ctx=c, out=buf, geometry=g)
            lines = buf.getvalue().splitlines()
            assert len(lines) == 50
            assert (r["state"] is not None) == (name == "shipped")
            assert all("class " in ln for ln in lines) == (name != "shipped")
        finally:
            c.close()

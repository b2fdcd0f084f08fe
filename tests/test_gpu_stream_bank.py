"""GPU tests (-m gpu) of the stream bank (edison_stream_bank_*, stream.StreamBank): n_mics continuous streams advancing in lockstep
through one graph. The reference is always the existing single-microphone stream: one stream.GeomStream per microphone in the same
process, created with the same geometry, options and model and fed that microphone's samples with the same push schedule. Every
comparison is exact (stream_drive.same). Graphs and geometries: the committed alt_models and the shipped graph, as test_gpu_stream_geom;
the recordings are seeded and differ per microphone."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import stream_drive as sd
from geom_sweep import GEOMS, geom, header
from stream_drive import recording, recordings, schedule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = sd.Kind("int8")


@pytest.mark.parametrize("chunk", [1, 3])
@pytest.mark.parametrize("name", ["shipped", "square", "odd_no_softmax"])
@pytest.mark.parametrize("n_mics", [3, 5])
def test_bank_equals_independent_streams(n_mics, name, chunk):
    """24 pushes: the sliding buffers hold 8, so the history is shifted to the front three times. Chunk 3 has ragged pushes of 1 and 2
    frames in between. Filter on; the shipped graph (10 classes) with edisonFSM: states at every push and the final machines."""
    c, g = KIND.open(name)
    try:
        sd.check_bank_equals_independent_streams(KIND, c, g, n_mics, chunk, name == "shipped", name)
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "square", "odd_no_softmax"])
def test_one_microphone_equals_a_stream(name):
    c, g = KIND.open(name)
    try:
        sd.check_one_microphone_equals_a_stream(KIND, c, g, name == "shipped", 3.0, name)
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "square", "odd_no_softmax"])
def test_host_device_and_alternating_pushes_agree(name):
    """Host pushes run on the bank's own HIP stream, device pushes on torch's: alternating them shares one history."""
    c, g = KIND.open(name)
    try:
        def after_host(b, host):
            assert ("keywords" in host[0]) == (c.net_info()["n_out"] == 10)

        sd.check_host_device_and_alternating_pushes(KIND, c, g, name == "shipped", name, after_host)
    finally:
        c.close()


def _route(c, g, x, what, ref=None):
    sched = schedule(3, 12)
    got, _ = sd.drive_bank(KIND, c, g, x, sched, chunk=3)
    ref = ref or sd.reference(KIND, c, g, x, sched, chunk=3)[0]
    sd.same_as_streams(KIND, got, ref, what)
    return ref


def test_network_routes_fast_forced_general_and_specialised(tmp_path, monkeypatch):
    """The shipped graph on its fast kernel, on the general kernel (EDISON_NET_FORCE_GENERAL=1) and on its own specialised kernel
    (edison_net_specialize, where a compiler exists; the JIT cache in tmp_path). 5 microphones: a fast-kernel wavefront takes four."""
    from edison_amd import _lib
    monkeypatch.setenv("EDISON_JIT_CACHE", str(tmp_path))
    c, g = KIND.open("shipped")
    try:
        x = recordings(g, 5, 3 * 12, 77)
        ref = _route(c, g, x, "fast kernel")
        monkeypatch.setenv("EDISON_NET_FORCE_GENERAL", "1")
        _route(c, g, x, "forced general kernel", ref)
        try:
            c.net_specialize()
        except _lib.EdisonError as e:
            assert e.code == _lib.E_NO_IMPL
        else:
            _route(c, g, x, "specialised kernel", ref)
    finally:
        c.close()


def test_network_route_general_kernel():
    c, g = KIND.open("kws_small")
    try:
        _route(c, g, recordings(g, 5, 3 * 12, 78), "general kernel")
    finally:
        c.close()


def test_layer_by_layer_route_in_a_child_process(tmp_path):
    """EDISON_NET_NO_MFMA=1 is read when the library loads its graph: bank and reference streams both run in a fresh process."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_stream_bank as t
for name in ("shipped", "odd_no_softmax"):
    c, g = t.KIND.open(name)
    t._route(c, g, t.recordings(g, 3, 3 * 12, 79), name + " layer by layer")
    c.close()
print("child ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, EDISON_NET_NO_MFMA="1", EDISON_NET_FORCE_GENERAL="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_reset_mic_reset_and_frames_seen():
    """After 10 pushes microphone 1 of 3 is reset: from then on it equals a new GeomStream fed the rest of its samples, microphones 0
    and 2 equal their uninterrupted streams. The buffers wrap before and after the reset (chunk 1: every 8 pushes)."""
    c, g = KIND.open("shipped")
    try:
        sd.check_reset_mic_reset_and_frames_seen(KIND, c, g)
    finally:
        c.close()


def test_errors():
    import torch
    from edison_amd import _lib
    from edison_amd.context import Context
    from edison_amd.stream import StreamBank
    L = _lib.lib()
    c = Context(0)
    try:
        g = geom()

        def fails(code, call):
            with pytest.raises(_lib.EdisonError) as e:
                call()
            assert e.value.code == code and "stream_bank" in str(e.value), str(e.value)

        o = _lib.StreamBankOpts()
        L.edison_stream_bank_default_opts(ctypes.byref(o))
        assert (o.n_mics, o.stream.chunk_frames, o.stream.filter, o.stream.fsm, o.stream.filter_alpha, o.stream.true_threshold) == (1, 1, 0, 0, 0.9, 0.5)
        for n_mics in (0, 4097):
            fails(_lib.E_ARGUMENT, lambda: StreamBank(c, g, n_mics))
        fails(_lib.E_ARGUMENT, lambda: StreamBank(c, g, 2, chunk_frames=0))
        fails(_lib.E_ARGUMENT, lambda: StreamBank(c, g, 2, output_filter=True, alpha=1.5))
        # NULL arguments and handles
        gc, h = g.to_ctypes(), ctypes.c_void_p()
        assert L.edison_stream_bank_create(None, ctypes.byref(gc), ctypes.byref(o), ctypes.byref(h)) == _lib.E_ARGUMENT
        assert L.edison_stream_bank_create(c._h, None, ctypes.byref(o), ctypes.byref(h)) == _lib.E_ARGUMENT
        assert L.edison_stream_bank_create(c._h, ctypes.byref(gc), None, ctypes.byref(h)) == _lib.E_ARGUMENT
        assert L.edison_stream_bank_create(c._h, ctypes.byref(gc), ctypes.byref(o), None) == _lib.E_ARGUMENT
        n64 = ctypes.c_int64()
        for r in (L.edison_stream_bank_reset(None), L.edison_stream_bank_reset_mic(None, 0), L.edison_stream_bank_push(None, None, None, None, None),
                  L.edison_stream_bank_push_dev(None, None, None, None, None), L.edison_stream_bank_push_n_dev(None, None, 1, None, None, None),
                  L.edison_stream_bank_filtered(None, None, None, None), L.edison_stream_bank_filtered_dev(None, None, None, None),
                  L.edison_stream_bank_fsm(None, None, None), L.edison_stream_bank_fsm_dev(None, None, None),
                  L.edison_stream_bank_frames_seen(None, ctypes.byref(n64))):
            assert r == _lib.E_ARGUMENT
        L.edison_stream_bank_destroy(None)
        b = StreamBank(c, g, 3, chunk_frames=2)
        assert L.edison_stream_bank_push(b._h, None, None, None, None) == _lib.E_ARGUMENT
        assert L.edison_stream_bank_frames_seen(b._h, None) == _lib.E_ARGUMENT
        # n_frames outside 1 .. chunk, a microphone outside 0 .. n_mics - 1, getters of stages the bank was made without
        xt = torch.zeros((3, 3 * 1024), dtype=torch.int16, device=torch.device("cuda", c.device))
        for n in (0, 3):
            fails(_lib.E_ARGUMENT, lambda: c._check(L.edison_stream_bank_push_n_dev(b._h, ctypes.c_void_p(xt.data_ptr()), n, None, None, None)))
        for m in (-1, 3):
            fails(_lib.E_ARGUMENT, lambda: b.reset_mic(m))
        fails(_lib.E_ARGUMENT, lambda: c._check(L.edison_stream_bank_filtered(b._h, None, None, None)))
        fails(_lib.E_ARGUMENT, lambda: c._check(L.edison_stream_bank_fsm(b._h, None, None)))
        with pytest.raises(ValueError):
            b.push(np.zeros((2, 2048), np.int16))
        # a push after a model reload
        b.push(np.zeros((3, 2048), np.int16))
        c.load_model(_lib.DEFAULT_MODEL)
        fails(_lib.E_ARGUMENT, lambda: b.push(np.zeros((3, 2048), np.int16)))
        b.close()
        # fsm without the filter: only reachable through the C-ABI
        o.n_mics, o.stream.fsm = 2, 1
        assert L.edison_stream_bank_create(c._h, ctypes.byref(gc), ctypes.byref(o), ctypes.byref(h)) == _lib.E_ARGUMENT
        assert "stream_bank" in (L.edison_last_error(c._h) or b"").decode()
        # the state machine needs 10 outputs; the geometry must fit the graph
        c.load_weights_h(header("same_stride"))    # 5 outputs
        gs = geom(**GEOMS["same_stride"])
        fails(_lib.E_NO_IMPL, lambda: StreamBank(c, gs, 2, fsm=True))
        fails(_lib.E_SIZE, lambda: StreamBank(c, g, 2))
        StreamBank(c, gs, 2, output_filter=True).close()
    finally:
        c.close()


def test_kws_live_with_two_recordings(tmp_path):
    """kws_live.run on two wav files of different length: under each microphone's heading the lines a run on that file alone prints."""
    import io
    import wave
    from edison_amd.kws import kws_live
    for name in ("shipped", "odd_no_softmax"):
        c, g = KIND.open(name)
        try:
            paths, alone = [], []
            for m, frames in enumerate((50, 37)):
                x = recording(g, frames, 2 + m)[:frames * g.frame_step - 100 * m]    # the second one ends inside a hop
                p = str(tmp_path / ("%s_%d.wav" % (name, m)))
                with wave.open(p, "wb") as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(16000)
                    w.writeframes(x.tobytes())
                paths.append(p)
                buf = io.StringIO()
                alone.append((kws_live.run(p, ctx=c, out=buf, geometry=g), buf.getvalue().splitlines()))
                assert len(alone[-1][1]) == frames
            buf = io.StringIO()
            r = kws_live.run(paths, ctx=c, out=buf, geometry=g)
            lines = buf.getvalue().splitlines()
            want = []
            for m, (ra, la) in enumerate(alone):
                want += ["mic %d: %s" % (m, paths[m])] + la
                assert r["mics"][m] == dict(commands=ra["commands"], state=ra["state"])
            assert lines == want
        finally:
            c.close()

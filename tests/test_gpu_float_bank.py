"""GPU tests (-m gpu) of the float bank (edison_float_bank_*, stream.FloatBank, kws_live.run([wav, ...], net=)): n_mics continuous
streams advancing in lockstep through one float32 X-CUBE-AI network. The reference is always the existing single-microphone stream: one
stream.FloatStream per microphone on the same context, created with the same geometry, flow and options and fed that microphone's samples
with the same push schedule. Every comparison is bit for bit (float32 compared as uint32): there is no tolerance. Networks and geometries
are test_gpu_stream_float's; the recordings are stream_drive.recordings, seeded and different per microphone."""
import contextlib
import ctypes
import io
import wave

import numpy as np
import pytest

import stream_drive as sd
from stream_drive import FIXTURE, float_blob, recording, recordings

pytestmark = pytest.mark.gpu

NETS = ["shipped", "shipped_q15", "kws_small", "odd_no_softmax"]
KIND = sd.Kind("float")


def _batch(c):
    return int(c.fnet_info()["batch"])


@pytest.mark.parametrize("chunk", [1, 3])
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("name", NETS)
def test_bank_equals_independent_streams(built_lib, name, big, chunk):
    """n_mics 3 and batch + 1 (a partial last tile of the network launch), 24 device pushes: the sliding buffers hold 8, so the history
    is shifted to the front three times. Chunk 3 has ragged pushes of 1 and 2 frames in between. Filter on; the 10-class networks with
    edisonFSM: states at every push and the final machines."""
    c, g = KIND.open(name)
    try:
        sd.check_bank_equals_independent_streams(KIND, c, g, _batch(c) + 1 if big else 3, chunk, name.startswith("shipped"), name)
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "shipped_q15", "odd_no_softmax"])
def test_tiles_that_straddle_frames(built_lib, name):
    """chunk = 2 B + 3 frames of n_mics = max(2, B - 1) microphones (B = the network kernel's utterances per workgroup): the smallest
    shape in which a tile of B windows spans a frame boundary at every offset and the last tile is partial. Three pushes, the last
    ragged with B + 1 frames."""
    c, g = KIND.open(name)
    try:
        B = _batch(c)
        chunk, n_mics = 2 * B + 3, max(2, B - 1)
        sched = [chunk, chunk, B + 1]
        offsets = {(t * B) % n_mics for t in range(-(-chunk * n_mics // B))}
        assert offsets == set(range(n_mics)) and (B == 1 or (chunk * n_mics) % B != 0 or ((B + 1) * n_mics) % B != 0), (B, offsets)
        x = recordings(g, n_mics, sum(sched), 7)
        ref, _ = sd.reference(KIND, c, g, x, sched, chunk=chunk, filt=True)
        got, _ = sd.drive_bank(KIND, c, g, x, sched, chunk=chunk, filt=True)
        sd.same_as_streams(KIND, got, ref, "%s straddling tiles" % name)
    finally:
        c.close()


@pytest.mark.parametrize("name", NETS)
def test_one_microphone_equals_a_stream(built_lib, name):
    c, g = KIND.open(name)
    try:
        sd.check_one_microphone_equals_a_stream(KIND, c, g, name.startswith("shipped"), 0.3, name)
    finally:
        c.close()


@pytest.mark.parametrize("name", NETS)
def test_host_device_and_alternating_pushes_agree(built_lib, name):
    """Host pushes run on the bank's own HIP stream, device pushes on torch's: alternating them shares one history."""
    c, g = KIND.open(name)
    try:
        def after_host(b, host):
            assert (b.keywords or []) == (KIND.model["keywords"] or [])   # the names of the .ednf, where it has any
            names = b.keywords or None
            if names:
                assert host[0]["keywords"] == [[names[i] for i in row] for row in host[0]["argmax"]]

        sd.check_host_device_and_alternating_pushes(KIND, c, g, name.startswith("shipped"), name, after_host)
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "shipped_q15"])
def test_reset_mic_reset_and_frames_seen(built_lib, name):
    """After 10 pushes microphone 1 of 3 is reset: from then on it equals a new FloatStream fed the rest of its samples, microphones 0
    and 2 equal their uninterrupted streams. The buffers wrap before and after the reset (chunk 1: every 8 pushes)."""
    c, g = KIND.open(name)
    try:
        sd.check_reset_mic_reset_and_frames_seen(KIND, c, g)
    finally:
        c.close()


def test_errors(built_lib):
    import torch
    from dataclasses import replace
    from edison_amd import _lib
    from edison_amd.context import Context
    from edison_amd.stream import FloatBank
    L = _lib.lib()
    c = Context(0, model_path=None)
    try:
        blob, g = float_blob("shipped")

        def fails(code, call, named=True):
            with pytest.raises(_lib.EdisonError) as e:
                call()
            assert e.value.code == code and (not named or "float_bank" in str(e.value)), str(e.value)

        # no float network loaded
        fails(_lib.E_NO_MODEL, lambda: FloatBank(c, 2, g), named=False)
        c.fnet_load(blob)
        for n_mics in (0, 4097):
            fails(_lib.E_ARGUMENT, lambda: FloatBank(c, n_mics, g))
        fails(_lib.E_ARGUMENT, lambda: FloatBank(c, 2, g, chunk_frames=0))
        fails(_lib.E_ARGUMENT, lambda: FloatBank(c, 2, g, output_filter=True, alpha=1.5))
        fails(_lib.E_ARGUMENT, lambda: FloatBank(c, 2, g, clip_min=1.0, clip_max=-1.0), named=False)
        # q15 off the shipped framing; a geometry whose window is not the network's input
        fails(_lib.E_NO_IMPL, lambda: FloatBank(c, 2, replace(g, frame_len=512, frame_step=512, n_samples=16384), q15=True), named=False)
        fails(_lib.E_SIZE, lambda: FloatBank(c, 2, replace(g, num_mfcc=12)), named=False)
        # NULL arguments
        o = _lib.FloatBankOpts()
        L.edison_float_bank_default_opts(ctypes.byref(o))
        gc, h = g.to_ctypes(), ctypes.c_void_p()
        assert L.edison_float_bank_create(None, ctypes.byref(gc), ctypes.byref(o), ctypes.byref(h)) == _lib.E_ARGUMENT
        assert L.edison_float_bank_create(c._h, None, ctypes.byref(o), ctypes.byref(h)) == _lib.E_ARGUMENT
        assert L.edison_float_bank_create(c._h, ctypes.byref(gc), None, ctypes.byref(h)) == _lib.E_ARGUMENT
        assert L.edison_float_bank_create(c._h, ctypes.byref(gc), ctypes.byref(o), None) == _lib.E_ARGUMENT
        b = FloatBank(c, 3, g, chunk_frames=2)
        assert L.edison_float_bank_push(b._h, None, None, None, None) == _lib.E_ARGUMENT
        assert L.edison_float_bank_frames_seen(b._h, None) == _lib.E_ARGUMENT
        # n_frames outside 1 .. chunk, a microphone outside 0 .. n_mics - 1, getters of stages the bank was made without
        xt = torch.zeros((3, 3 * 1024), dtype=torch.int16, device=torch.device("cuda", c.device))
        for n in (0, 3):
            fails(_lib.E_ARGUMENT, lambda: c._check(L.edison_float_bank_push_n_dev(b._h, ctypes.c_void_p(xt.data_ptr()), n, None, None, None)))
        for m in (-1, 3):
            fails(_lib.E_ARGUMENT, lambda: b.reset_mic(m))
        fails(_lib.E_ARGUMENT, lambda: c._check(L.edison_float_bank_filtered(b._h, None, None, None)))
        fails(_lib.E_ARGUMENT, lambda: c._check(L.edison_float_bank_fsm(b._h, None, None)))
        with pytest.raises(ValueError):
            b.push(np.zeros((2, 2048), np.int16))
        # a push after edison_fnet_load replaced the network
        b.push(np.zeros((3, 2048), np.int16))
        c.fnet_load(blob)
        fails(_lib.E_ARGUMENT, lambda: b.push(np.zeros((3, 2048), np.int16)))
        b.close()
        # fsm without the filter: only reachable through the C-ABI
        o.n_mics, o.stream.fsm = 2, 1
        assert L.edison_float_bank_create(c._h, ctypes.byref(gc), ctypes.byref(o), ctypes.byref(h)) == _lib.E_ARGUMENT
        assert "float_bank" in (L.edison_last_error(c._h) or b"").decode()
        # the state machine needs 10 outputs; the filter alone serves any count up to 256
        sblob, sg = float_blob("kws_small")
        c.fnet_load(sblob)
        fails(_lib.E_NO_IMPL, lambda: FloatBank(c, 2, sg, fsm=True))
        FloatBank(c, 2, sg, output_filter=True).close()
    finally:
        c.close()


def _wav(x, p):
    with wave.open(p, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(x.tobytes())
    return p


def test_kws_live_with_two_recordings(built_lib, tmp_path):
    """kws_live.run on two wav files of different length with a float network: under each microphone's heading the lines a run on that
    file alone prints. The same through the command line, on the default context."""
    from edison_amd.context import Context
    from edison_amd.kws import kws_live
    for name in ("shipped", "shipped_q15", "odd_no_softmax"):
        blob, g = float_blob(name)
        q15 = name.endswith("_q15")
        geometry = None if name.startswith("shipped") else g
        c = Context(0, model_path=None)
        try:
            paths, alone = [], []
            for m, frames in enumerate((50, 37)):
                x = recording(g, frames, 2 + m)[:frames * g.frame_step - 100 * m]    # the second one ends inside a hop
                paths.append(_wav(x, str(tmp_path / ("%s_%d.wav" % (name, m)))))
                buf = io.StringIO()
                alone.append((kws_live.run(paths[-1], q15=q15, ctx=c, out=buf, geometry=geometry, net=blob), buf.getvalue().splitlines()))
                assert len(alone[-1][1]) == frames
            buf = io.StringIO()
            r = kws_live.run(paths, q15=q15, ctx=c, out=buf, geometry=geometry, net=blob)
            want = []
            for m, (ra, la) in enumerate(alone):
                want += ["mic %d: %s" % (m, paths[m])] + la
                assert r["mics"][m] == dict(commands=ra["commands"], state=ra["state"])
            assert buf.getvalue().splitlines() == want
        finally:
            c.close()
    # the command line
    g = float_blob("shipped")[1]
    paths = [_wav(recording(g, frames, 5 + m)[:frames * 1024 - 300 * m], str(tmp_path / ("cli_%d.wav" % m))) for m, frames in enumerate((40, 23))]
    want = []
    for m, p in enumerate(paths):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            assert kws_live.main(["live", "mcu", p, "--net", FIXTURE]) == 0
        want += ["mic %d: %s" % (m, p)] + buf.getvalue().splitlines()
    assert len(want) == 2 + 40 + 23
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert kws_live.main(["live", "mcu"] + paths + ["--net", FIXTURE]) == 0
    assert buf.getvalue().splitlines() == want

"""GPU tests (-m gpu) of the float bank (edison_float_bank_*, stream.FloatBank, kws_live.run([wav, ...], net=)): n_mics continuous
streams advancing in lockstep through one float32 X-CUBE-AI network. The reference is always the existing single-microphone stream: one
stream.FloatStream per microphone on the same context, created with the same geometry, flow and options and fed that microphone's samples
with the same push schedule. Every comparison is bit for bit (float32 compared as uint32): there is no tolerance. Networks and geometries
are test_gpu_stream_float's; the recordings are test_gpu_stream_bank's, seeded and different per microphone."""
import contextlib
import ctypes
import io
import wave

import numpy as np
import pytest

from test_gpu_stream_bank import _recordings, _schedule, _to_host, _torch_stream
from test_gpu_stream_float import FIXTURE, _blob, _open
from test_gpu_stream_geom import _recording

pytestmark = pytest.mark.gpu

NETS = ["shipped", "shipped_q15", "kws_small", "odd_no_softmax"]
KEYS = ("logits", "probs", "argmax", "filtered", "likely", "spotted", "fsm_states")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.shape[0] == 0, "%s: %d of %d differ, first at %s: %r != %r" % (what, bad.shape[0], got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                             want[tuple(bad[0])])


def _empty_outputs(torch, dev, shape, no, filt, fsm):
    """Device tensors for the outputs of K frames: shape = (K,) for one stream, (K, n_mics) for a bank."""
    z = lambda tail, dt: torch.zeros(shape + tail, dtype=dt, device=dev)
    o = dict(logits=z((no,), torch.float32), probs=z((no,), torch.float32), argmax=z((), torch.int32))
    if filt:
        o.update(filtered=z((no,), torch.float32), likely=z((), torch.int32), spotted=z((), torch.int32))
    if fsm:
        o.update(fsm_states=z((), torch.int32))
    return o


def _kw(o, sl, filt):
    kw = dict(logits=o["logits"][sl], probs=o["probs"][sl], argmax=o["argmax"][sl])
    if filt:
        kw.update(filtered=o["filtered"][sl], likely=o["likely"][sl], spotted=o["spotted"][sl])
    return kw


def _reference(c, g, q15, x, chunk, sched, filt=False, fsm=False, alpha=0.5, threshold=0.5):
    """One FloatStream per microphone, device pushes by the schedule. Returns ([per microphone: dict of [K][..]], [final FSM raw])."""
    from edison_amd import _lib
    from edison_amd.stream import FloatStream
    torch, dev = _torch_stream(c)
    L = _lib.lib()
    outs, snaps = [], []
    try:
        for m in range(x.shape[0]):
            s = FloatStream(c, g, q15=q15, chunk_frames=chunk, output_filter=filt, alpha=alpha, threshold=threshold, fsm=fsm)
            xt = torch.from_numpy(x[m]).to(dev)
            o = _empty_outputs(torch, dev, (sum(sched),), s.n_out, filt, fsm)
            k0 = 0
            for n in sched:
                sl = slice(k0, k0 + n)
                s.push_t(xt[k0 * s.hop:(k0 + n) * s.hop], n_frames=None if n == chunk else n, **_kw(o, sl, filt))
                if fsm:
                    c._check(L.edison_stream_float_fsm_dev(s._h, ctypes.c_void_p(o["fsm_states"][sl].data_ptr())))
                k0 += n
            torch.cuda.synchronize(dev)
            if fsm:
                c._check(L.edison_stream_float_fsm(s._h, ctypes.byref(s._fsm), None))
                snaps.append(s.fsm_snapshot()["raw"])
            assert s.frames_seen == k0
            s.close()
            outs.append(_to_host(o))
    finally:
        c.use_own_stream()
    return outs, snaps


def _bank(c, g, q15, x, chunk, sched, filt=False, fsm=False, alpha=0.5, threshold=0.5, bank=None):
    """The bank on the same samples by the same schedule. Returns (dict of [K][n_mics][..], [final FSM raw per microphone])."""
    from edison_amd.stream import FloatBank
    torch, dev = _torch_stream(c)
    M = x.shape[0]
    try:
        b = bank or FloatBank(c, M, g, q15=q15, chunk_frames=chunk, output_filter=filt, alpha=alpha, threshold=threshold, fsm=fsm)
        X = torch.from_numpy(x).to(dev)
        o = _empty_outputs(torch, dev, (sum(sched), M), b.n_out, filt, fsm)
        k0 = 0
        for n in sched:
            sl = slice(k0, k0 + n)
            kw = _kw(o, sl, filt)
            if fsm:
                kw.update(fsm_states=o["fsm_states"][sl])
            b.push_t(X[:, k0 * b.hop:(k0 + n) * b.hop].contiguous(), n_frames=None if n == b.chunk else n, **kw)
            k0 += n
        torch.cuda.synchronize(dev)
        snaps = []
        if fsm:
            c._check(b._c("fsm")(b._h, ctypes.byref(b._fsms), None))
            snaps = [s["raw"] for s in b.fsm_snapshot()]
        if bank is None:
            assert b.frames_seen() == k0
            b.close()
    finally:
        c.use_own_stream()
    return _to_host(o), snaps


def _same_as_streams(got, ref, what, mics=None, rows=slice(None)):
    """Microphone m of the bank's outputs equals reference stream m's, in every output the reference has."""
    for m in (range(len(ref)) if mics is None else mics):
        for k in KEYS:
            if k not in ref[m]:
                assert k not in got, (what, k)
            else:
                _same(got[k][rows, m], ref[m][k], "%s microphone %d %s" % (what, m, k))


def _batch(c):
    return int(c.fnet_info()["batch"])


@pytest.mark.parametrize("chunk", [1, 3])
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("name", NETS)
def test_bank_equals_independent_streams(built_lib, name, big, chunk):
    """n_mics 3 and batch + 1 (a partial last tile of the network launch), 24 device pushes: the sliding buffers hold 8, so the history
    is shifted to the front three times. Chunk 3 has ragged pushes of 1 and 2 frames in between. Filter on; the 10-class networks with
    edisonFSM: states at every push and the final machines."""
    c, g, q15, _ = _open(name)
    try:
        n_mics = _batch(c) + 1 if big else 3
        fsm = name.startswith("shipped")
        sched = _schedule(chunk, 24)
        assert chunk == 1 or (min(sched) < chunk and max(sched) == chunk)
        x = _recordings(g, n_mics, sum(sched), 100 + n_mics)
        ref, ref_snaps = _reference(c, g, q15, x, chunk, sched, filt=True, fsm=fsm)
        got, snaps = _bank(c, g, q15, x, chunk, sched, filt=True, fsm=fsm)
        _same_as_streams(got, ref, "%s x%d chunk %d" % (name, n_mics, chunk))
        assert snaps == ref_snaps
        assert any(not np.array_equal(ref[0]["logits"], r["logits"]) for r in ref[1:])   # the microphones do differ
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "shipped_q15", "odd_no_softmax"])
def test_tiles_that_straddle_frames(built_lib, name):
    """chunk = 2 B + 3 frames of n_mics = max(2, B - 1) microphones (B = the network kernel's utterances per workgroup): the smallest
    shape in which a tile of B windows spans a frame boundary at every offset and the last tile is partial. Three pushes, the last
    ragged with B + 1 frames."""
    c, g, q15, _ = _open(name)
    try:
        B = _batch(c)
        chunk, n_mics = 2 * B + 3, max(2, B - 1)
        sched = [chunk, chunk, B + 1]
        offsets = {(t * B) % n_mics for t in range(-(-chunk * n_mics // B))}
        assert offsets == set(range(n_mics)) and (B == 1 or (chunk * n_mics) % B != 0 or ((B + 1) * n_mics) % B != 0), (B, offsets)
        x = _recordings(g, n_mics, sum(sched), 7)
        ref, _ = _reference(c, g, q15, x, chunk, sched, filt=True)
        got, _ = _bank(c, g, q15, x, chunk, sched, filt=True)
        _same_as_streams(got, ref, "%s straddling tiles" % name)
    finally:
        c.close()


@pytest.mark.parametrize("name", NETS)
def test_one_microphone_equals_a_stream(built_lib, name):
    c, g, q15, _ = _open(name)
    try:
        fsm = name.startswith("shipped")
        sched = _schedule(3, 24)
        x = _recordings(g, 1, sum(sched), 9)
        ref, ref_snaps = _reference(c, g, q15, x, 3, sched, filt=True, fsm=fsm, alpha=0.6, threshold=0.3)
        got, snaps = _bank(c, g, q15, x, 3, sched, filt=True, fsm=fsm, alpha=0.6, threshold=0.3)
        _same_as_streams(got, ref, name + " one microphone")
        assert snaps == ref_snaps
    finally:
        c.close()


def _host_pushes(b, x, pushes, first=0):
    h = b.chunk * b.hop
    return [b.push(x[:, i * h:(i + 1) * h]) for i in range(first, first + pushes)]


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in KEYS if k in parts[0]}


@pytest.mark.parametrize("name", NETS)
def test_host_device_and_alternating_pushes_agree(built_lib, name):
    """Host pushes run on the bank's own HIP stream, device pushes on torch's: alternating them shares one history."""
    from edison_amd.stream import FloatBank
    c, g, q15, model = _open(name)
    try:
        chunk, pushes, M = 3, 20, 3
        fsm = name.startswith("shipped")
        sched = [chunk] * pushes
        x = _recordings(g, M, chunk * pushes, 55)
        ref, ref_snaps = _reference(c, g, q15, x, chunk, sched, filt=True, fsm=fsm)
        b = FloatBank(c, M, g, q15=q15, chunk_frames=chunk, output_filter=True, fsm=fsm)
        assert (b.keywords or []) == (model["keywords"] or [])   # the names of the .ednf, where it has any
        host = _host_pushes(b, x, pushes)
        _same_as_streams(_cat(host), ref, name + " host pushes")
        names = b.keywords or None
        if names:
            assert host[0]["keywords"] == [[names[i] for i in row] for row in host[0]["argmax"]]
        assert b.frames_seen() == chunk * pushes
        if fsm:
            assert [f["raw"] for f in host[-1]["fsm"]] == ref_snaps
        b.reset()
        assert b.frames_seen() == 0
        dev, _ = _bank(c, g, q15, x, chunk, sched, filt=True, fsm=fsm, bank=b)
        _same_as_streams(dev, ref, name + " device pushes after reset")
        b.reset()
        parts = []
        h = chunk * g.frame_step
        for i in range(pushes):
            if i % 2 == 0:
                parts.append(_host_pushes(b, x, 1, first=i)[0])
            else:
                parts.append(_bank(c, g, q15, x[:, i * h:(i + 1) * h], chunk, [chunk], filt=True, fsm=fsm, bank=b)[0])
        _same_as_streams(_cat(parts), ref, name + " alternating pushes")
        b.close()
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "shipped_q15"])
def test_reset_mic_reset_and_frames_seen(built_lib, name):
    """After 10 pushes microphone 1 of 3 is reset: from then on it equals a new FloatStream fed the rest of its samples, microphones 0
    and 2 equal their uninterrupted streams. The buffers wrap before and after the reset (chunk 1: every 8 pushes)."""
    from edison_amd.stream import FloatBank
    c, g, q15, _ = _open(name)
    try:
        K, cut = 30, 10
        x = _recordings(g, 3, K, 41)
        whole, whole_snaps = _reference(c, g, q15, x, 1, [1] * K, filt=True, fsm=True)
        rest, rest_snaps = _reference(c, g, q15, x[1:2, cut * g.frame_step:], 1, [1] * (K - cut), filt=True, fsm=True)
        b = FloatBank(c, 3, g, q15=q15, chunk_frames=1, fsm=True)
        head, _ = _bank(c, g, q15, x[:, :cut * g.frame_step], 1, [1] * cut, filt=True, fsm=True, bank=b)
        _same_as_streams(head, [{k: v[:cut] for k, v in w.items()} for w in whole], "before reset_mic")
        b.reset_mic(1)
        assert b.frames_seen() == cut
        tail, snaps = _bank(c, g, q15, x[:, cut * g.frame_step:], 1, [1] * (K - cut), filt=True, fsm=True, bank=b)
        assert b.frames_seen() == K
        _same_as_streams(tail, [{k: v[cut:] for k, v in w.items()} for w in whole], "after reset_mic", mics=(0, 2))
        for k in KEYS:
            _same(tail[k][:, 1], rest[0][k], "the reset microphone " + k)
        assert [snaps[0], snaps[2]] == [whole_snaps[0], whole_snaps[2]] and snaps[1] == rest_snaps[0]
        # reset: the whole bank equals new streams again
        b.reset()
        assert b.frames_seen() == 0
        again, again_snaps = _bank(c, g, q15, x, 1, [1] * K, filt=True, fsm=True, bank=b)
        _same_as_streams(again, whole, "after reset")
        assert again_snaps == whole_snaps
        b.close()
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
        blob, g = _blob("shipped")

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
        sblob, sg = _blob("kws_small")
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
        blob, g = _blob(name)
        q15 = name.endswith("_q15")
        geometry = None if name.startswith("shipped") else g
        c = Context(0, model_path=None)
        try:
            paths, alone = [], []
            for m, frames in enumerate((50, 37)):
                x = _recording(g, frames, 2 + m)[:frames * g.frame_step - 100 * m]    # the second one ends inside a hop
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
    g = _blob("shipped")[1]
    paths = [_wav(_recording(g, frames, 5 + m)[:frames * 1024 - 300 * m], str(tmp_path / ("cli_%d.wav" % m))) for m, frames in enumerate((40, 23))]
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

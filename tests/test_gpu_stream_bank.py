"""GPU tests (-m gpu) of the stream bank (edison_stream_bank_*, stream.StreamBank): n_mics continuous streams advancing in lockstep
through one graph. The reference is always the existing single-microphone stream: one stream.GeomStream per microphone in the same
process, created with the same geometry, options and model and fed that microphone's samples with the same push schedule. Every
comparison is exact (np.array_equal). Graphs and geometries: the committed alt_models and the shipped graph, as test_gpu_stream_geom;
the recordings are seeded and differ per microphone."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_kws_geom import GEOMS, _geom, _header, _same, _signals
from test_gpu_stream_geom import _open, _recording

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("logits", "softmax", "argmax", "filtered", "likely", "spotted", "fsm_states")


def _recordings(g, n_mics, n_frames, seed):
    """int16 [n_mics][n_frames * hop]: another recording for every microphone -- the _signals mix (silence, noise, tones, clipping, the
    `edison` utterance) in stretches of five hops, seeded per microphone and starting at another kind."""
    per = 5 * g.frame_step
    rows = -(-n_frames // 5) + 5
    return np.stack([_signals(rows, per, seed + 17 * m)[1 + m % 4:].ravel()[:n_frames * g.frame_step] for m in range(n_mics)])


def _schedule(chunk, pushes):
    """Frames per push: full pushes with ragged ones (n < chunk) in between where the chunk allows them."""
    return [chunk if chunk == 1 or i % 4 != 2 else 1 + i % (chunk - 1) for i in range(pushes)]


def _torch_stream(c):
    import torch
    dev = torch.device("cuda", c.device)
    c.use_torch_stream(torch.cuda.current_stream(dev))
    return torch, dev


def _empty_outputs(torch, dev, shape, no, has_softmax, filt, fsm):
    """Device tensors for the outputs of K frames: shape = (K,) for one stream, (K, n_mics) for a bank."""
    z = lambda tail, dt: torch.zeros(shape + tail, dtype=dt, device=dev)
    o = dict(logits=z((no,), torch.int8), softmax=z((no,), torch.int8) if has_softmax else None, argmax=z((), torch.int32))
    if filt:
        o.update(filtered=z((no,), torch.float32), likely=z((), torch.int32), spotted=z((), torch.int32))
    if fsm:
        o.update(fsm_states=z((), torch.int32))
    return o


def _to_host(o):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _push_stream(s, L, xt, k0, n, o, filt, fsm):
    """Device push of frames k0 .. k0 + n of one microphone's samples xt into the GeomStream s, outputs to rows k0 .. of o."""
    sl = slice(k0, k0 + n)
    kw = dict(logits=o["logits"][sl], softmax=None if o["softmax"] is None else o["softmax"][sl], argmax=o["argmax"][sl])
    if filt:
        kw.update(filtered=o["filtered"][sl], likely=o["likely"][sl], spotted=o["spotted"][sl])
    s.push_t(xt[k0 * s.hop:(k0 + n) * s.hop], n_frames=None if n == s.chunk else n, **kw)
    if fsm:
        s.ctx._check(L.edison_stream_geom_fsm_dev(s._h, ctypes.c_void_p(o["fsm_states"][sl].data_ptr())))


def _push_bank(b, X, k0, n, o, filt, fsm):
    """Device push of frames k0 .. k0 + n of every microphone (X device [n_mics][K * hop]) into the bank, outputs to slabs k0 .. of o."""
    sl = slice(k0, k0 + n)
    kw = dict(logits=o["logits"][sl], softmax=None if o["softmax"] is None else o["softmax"][sl], argmax=o["argmax"][sl])
    if filt:
        kw.update(filtered=o["filtered"][sl], likely=o["likely"][sl], spotted=o["spotted"][sl])
    if fsm:
        kw.update(fsm_states=o["fsm_states"][sl])
    b.push_t(X[:, k0 * b.hop:(k0 + n) * b.hop].contiguous(), n_frames=None if n == b.chunk else n, **kw)


def _reference(c, g, x, chunk, sched, filt=False, fsm=False, alpha=0.9, threshold=0.5):
    """One GeomStream per microphone, device pushes by the schedule. Returns ([per microphone: dict of [K][..]], [final FSM raw])."""
    from edison_amd import _lib
    from edison_amd.stream import GeomStream
    torch, dev = _torch_stream(c)
    L = _lib.lib()
    info = c.net_info()
    outs, snaps = [], []
    try:
        for m in range(x.shape[0]):
            s = GeomStream(c, g, chunk_frames=chunk, output_filter=filt, alpha=alpha, threshold=threshold, fsm=fsm)
            xt = torch.from_numpy(x[m]).to(dev)
            o = _empty_outputs(torch, dev, (sum(sched),), info["n_out"], info["has_softmax"], filt, fsm)
            k0 = 0
            for n in sched:
                _push_stream(s, L, xt, k0, n, o, filt, fsm)
                k0 += n
            torch.cuda.synchronize(dev)
            if fsm:
                c._check(L.edison_stream_geom_fsm(s._h, ctypes.byref(s._fsm), None))
                snaps.append(s.fsm_snapshot()["raw"])
            assert s.frames_seen == k0
            s.close()
            outs.append(_to_host(o))
    finally:
        c.use_own_stream()
    return outs, snaps


def _bank(c, g, x, chunk, sched, filt=False, fsm=False, alpha=0.9, threshold=0.5, bank=None):
    """The bank on the same samples by the same schedule. Returns (dict of [K][n_mics][..], [final FSM raw per microphone])."""
    from edison_amd.stream import StreamBank
    torch, dev = _torch_stream(c)
    info = c.net_info()
    M = x.shape[0]
    try:
        b = bank or StreamBank(c, g, M, chunk_frames=chunk, output_filter=filt, alpha=alpha, threshold=threshold, fsm=fsm)
        X = torch.from_numpy(x).to(dev)
        o = _empty_outputs(torch, dev, (sum(sched), M), info["n_out"], info["has_softmax"], filt, fsm)
        k0 = 0
        for n in sched:
            _push_bank(b, X, k0, n, o, filt, fsm)
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
            elif ref[m][k] is None:
                assert got[k] is None, (what, k)
            else:
                _same(got[k][rows, m], ref[m][k], "%s microphone %d %s" % (what, m, k))


@pytest.mark.parametrize("chunk", [1, 3])
@pytest.mark.parametrize("name", ["shipped", "square", "odd_no_softmax"])
@pytest.mark.parametrize("n_mics", [3, 5])
def test_bank_equals_independent_streams(n_mics, name, chunk):
    """24 pushes: the sliding buffers hold 8, so the history is shifted to the front three times. Chunk 3 has ragged pushes of 1 and 2
    frames in between. Filter on; the shipped graph (10 classes) with edisonFSM: states at every push and the final machines."""
    c, g = _open(name)
    try:
        fsm = name == "shipped"
        sched = _schedule(chunk, 24)
        assert chunk == 1 or (min(sched) < chunk and max(sched) == chunk)
        x = _recordings(g, n_mics, sum(sched), 100 + n_mics)
        ref, ref_snaps = _reference(c, g, x, chunk, sched, filt=True, fsm=fsm)
        got, snaps = _bank(c, g, x, chunk, sched, filt=True, fsm=fsm)
        _same_as_streams(got, ref, "%s x%d chunk %d" % (name, n_mics, chunk))
        assert snaps == ref_snaps
        assert any(not np.array_equal(ref[0]["logits"], r["logits"]) for r in ref[1:])   # the microphones do differ
    finally:
        c.close()


@pytest.mark.parametrize("name", ["shipped", "square", "odd_no_softmax"])
def test_one_microphone_equals_a_stream(name):
    c, g = _open(name)
    try:
        fsm = name == "shipped"
        sched = _schedule(3, 24)
        x = _recordings(g, 1, sum(sched), 9)
        ref, ref_snaps = _reference(c, g, x, 3, sched, filt=True, fsm=fsm, alpha=0.6, threshold=3.0)
        got, snaps = _bank(c, g, x, 3, sched, filt=True, fsm=fsm, alpha=0.6, threshold=3.0)
        _same_as_streams(got, ref, name + " one microphone")
        assert snaps == ref_snaps
    finally:
        c.close()


def _host_pushes(b, x, pushes, first=0):
    """Host pushes `first` .. of chunk frames each; returns the list of push dicts."""
    h = b.chunk * b.hop
    return [b.push(x[:, i * h:(i + 1) * h]) for i in range(first, first + pushes)]


def _cat(parts):
    return {k: (None if parts[0].get(k) is None else np.concatenate([p[k] for p in parts])) for k in KEYS if k in parts[0]}


@pytest.mark.parametrize("name", ["shipped", "square", "odd_no_softmax"])
def test_host_device_and_alternating_pushes_agree(name):
    """Host pushes run on the bank's own HIP stream, device pushes on torch's: alternating them shares one history."""
    from edison_amd.stream import StreamBank
    c, g = _open(name)
    try:
        chunk, pushes, M = 3, 20, 3
        fsm = name == "shipped"
        sched = [chunk] * pushes
        x = _recordings(g, M, chunk * pushes, 55)
        ref, ref_snaps = _reference(c, g, x, chunk, sched, filt=True, fsm=fsm)
        b = StreamBank(c, g, M, chunk_frames=chunk, output_filter=True, fsm=fsm)
        host = _host_pushes(b, x, pushes)
        _same_as_streams(_cat(host), ref, name + " host pushes")
        assert ("keywords" in host[0]) == (c.net_info()["n_out"] == 10)
        assert b.frames_seen() == chunk * pushes
        if fsm:
            assert [f["raw"] for f in host[-1]["fsm"]] == ref_snaps
        b.reset()
        assert b.frames_seen() == 0
        dev, _ = _bank(c, g, x, chunk, sched, filt=True, fsm=fsm, bank=b)
        _same_as_streams(dev, ref, name + " device pushes after reset")
        b.reset()
        parts = []
        h = chunk * g.frame_step
        for i in range(pushes):
            if i % 2 == 0:
                parts.append(_host_pushes(b, x, 1, first=i)[0])
            else:
                parts.append(_bank(c, g, x[:, i * h:(i + 1) * h], chunk, [chunk], filt=True, fsm=fsm, bank=b)[0])
        _same_as_streams(_cat(parts), ref, name + " alternating pushes")
        b.close()
    finally:
        c.close()


def _route(c, g, x, what, ref=None):
    sched = _schedule(3, 12)
    got, _ = _bank(c, g, x, 3, sched)
    ref = ref or _reference(c, g, x, 3, sched)[0]
    _same_as_streams(got, ref, what)
    return ref


def test_network_routes_fast_forced_general_and_specialised(tmp_path, monkeypatch):
    """The shipped graph on its fast kernel, on the general kernel (EDISON_NET_FORCE_GENERAL=1) and on its own specialised kernel
    (edison_net_specialize, where a compiler exists; the JIT cache in tmp_path). 5 microphones: a fast-kernel wavefront takes four."""
    from edison_amd import _lib
    monkeypatch.setenv("EDISON_JIT_CACHE", str(tmp_path))
    c, g = _open("shipped")
    try:
        x = _recordings(g, 5, 3 * 12, 77)
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
    c, g = _open("kws_small")
    try:
        _route(c, g, _recordings(g, 5, 3 * 12, 78), "general kernel")
    finally:
        c.close()


def test_layer_by_layer_route_in_a_child_process(tmp_path):
    """EDISON_NET_NO_MFMA=1 is read when the library loads its graph: bank and reference streams both run in a fresh process."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_stream_bank as t
for name in ("shipped", "odd_no_softmax"):
    c, g = t._open(name)
    t._route(c, g, t._recordings(g, 3, 3 * 12, 79), name + " layer by layer")
    c.close()
print("child ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, EDISON_NET_NO_MFMA="1", EDISON_NET_FORCE_GENERAL="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_reset_mic_reset_and_frames_seen():
    """After 10 pushes microphone 1 of 3 is reset: from then on it equals a new GeomStream fed the rest of its samples, microphones 0
    and 2 equal their uninterrupted streams. The buffers wrap before and after the reset (chunk 1: every 8 pushes)."""
    from edison_amd.stream import StreamBank
    c, g = _open("shipped")
    try:
        K, cut = 30, 10
        x = _recordings(g, 3, K, 41)
        whole, whole_snaps = _reference(c, g, x, 1, [1] * K, filt=True, fsm=True)
        rest, rest_snaps = _reference(c, g, x[1:2, cut * g.frame_step:], 1, [1] * (K - cut), filt=True, fsm=True)
        b = StreamBank(c, g, 3, chunk_frames=1, fsm=True)
        head, _ = _bank(c, g, x[:, :cut * g.frame_step], 1, [1] * cut, filt=True, fsm=True, bank=b)
        _same_as_streams(head, [{k: v[:cut] for k, v in w.items()} for w in whole], "before reset_mic")
        b.reset_mic(1)
        assert b.frames_seen() == cut
        tail, snaps = _bank(c, g, x[:, cut * g.frame_step:], 1, [1] * (K - cut), filt=True, fsm=True, bank=b)
        assert b.frames_seen() == K
        _same_as_streams(tail, [{k: v[cut:] for k, v in w.items()} for w in whole], "after reset_mic", mics=(0, 2))
        for k in KEYS:
            _same(tail[k][:, 1], rest[0][k], "the reset microphone " + k)
        assert [snaps[0], snaps[2]] == [whole_snaps[0], whole_snaps[2]] and snaps[1] == rest_snaps[0]
        # reset: the whole bank equals new streams again
        b.reset()
        assert b.frames_seen() == 0
        again, again_snaps = _bank(c, g, x, 1, [1] * K, filt=True, fsm=True, bank=b)
        _same_as_streams(again, whole, "after reset")
        assert again_snaps == whole_snaps
        b.close()
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
        g = _geom()

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
        c.load_weights_h(_header("same_stride"))    # 5 outputs
        gs = _geom(**GEOMS["same_stride"])
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
        c, g = _open(name)
        try:
            paths, alone = [], []
            for m, frames in enumerate((50, 37)):
                x = _recording(g, frames, 2 + m)[:frames * g.frame_step - 100 * m]    # the second one ends inside a hop
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

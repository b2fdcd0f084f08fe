"""GPU tests (-m gpu) of bank pushes that leave microphones out (edison_bank_push_present*, edison_fbank_push_present*,
StreamBank / FloatBank .push(present=), .push_t(present=), .frames_seen_mics()), for both banks.

The defining property is tested as it is stated: push k carries a set P_k of present microphones and n_k frames; the reference for
microphone m is ONE single stream S_m in the same process (a GeomStream for the stream bank, a FloatStream for the float bank, same
geometry, options and model) that is pushed exactly the pushes k with m in P_k, with m's samples of those pushes. For m in P_k the bank's
rows [i][m] of push k equal S_m's outputs of that push; after every push m's state machine equals S_m's and m's frame count equals
S_m.frames_seen; for m outside P_k the rows hold the fill. Every comparison is byte for byte (float32 compared as uint32): there is no
tolerance. A stream that has not been pushed yet has no outputs to copy a machine from: its machine is edison_fsm_init's, which is what
the stream starts its first push with."""
import ctypes

import numpy as np
import pytest

import stream_drive as sd
from geom_sweep import GEOMS
from stream_drive import HOST, DEV, DEV_NO_OUT, recordings, same, schedule, start_machine

pytestmark = pytest.mark.gpu

M = 4                                    # microphones of the main schedule
SYNTH10 = [("conv", 8, (3, 3), (1, 1), (2, 2), 1), ("dense", 16), ("relu",), ("dense", 10), ("softmax",)]   # 10 outputs: edisonFSM runs
# frame_len > 2 * frame_step: T = 720 history samples are held in three rounds of 256 and overlap their destination at n = 1 and 2;
# 64 rows of 16 coefficients, so the committed `square` graph and a synthetic float network both fit
LONG = dict(GEOMS["square"], frame_len=960, frame_step=240, n_samples=16080)
# name -> (graph or network, geometry): tail = 0 / T <= n * hop / frame_len > 2 * frame_step. F - 1 > n in all of them.
INT8 = {"shipped": ("shipped", None), "even_same": ("even_same", GEOMS["even_same"]), "long": ("square", LONG)}
FLOAT = {"shipped_q15": ("shipped_q15", None), "even_same": ("synth", GEOMS["even_same"]), "long": ("synth", LONG)}
CASES = [("int8", n) for n in INT8] + [("float", n) for n in FLOAT]


def _open(kind, name):
    """(one bank type and its single stream behind the same calls, context with the model loaded, geometry)."""
    K = sd.Kind(kind)
    model, gk = (INT8 if kind == "int8" else FLOAT)[name]
    c, g = K.open(name if model == "synth" else model, gk, SYNTH10)
    return K, c, g


def _bank(K, c, g, n_mics, chunk):
    return K.bank(c, g, n_mics, chunk, output_filter=True, fsm=K.fsm)


# ---- the schedule ------------------------------------------------------------------------------------------------------------------
def _frames(chunk, pushes, ragged):
    """Frames per push: full pushes, with ragged ones of 1 .. chunk - 1 frames in between where asked for."""
    return schedule(chunk, pushes, sd.by_round if ragged else None)


def _schedule(F, chunk, ragged, n_mics=M, seed=5):
    """[(n_k, mask or None)]: at least three wraps of the sliding buffers (8 pushes of room) and, seeded, the cases a mask can be in:
         microphone 0   absent from the first push (zero history is carried), then by chance
         microphone 1   absent across the first wrap (the push before it, the wrapping push and the one after)
         microphone 2   absent for more than F frames in a row, then present to the end
         microphone 3   by chance
       one push with everyone absent, one with an all-ones mask, and every fifth push without a mask (None)."""
    long_gap = -(-(F + 1) // chunk) + 4                  # pushes that hold more than F frames even if some are ragged
    pushes = max(30, 6 + long_gap + 6)
    frames = _frames(chunk, pushes, ragged)
    wraps = sd.wraps(frames, chunk)
    assert len(wraps) >= 3, wraps
    rng = np.random.default_rng(seed)
    masks = (rng.random((pushes, n_mics)) < 0.6).astype(np.uint8)
    masks[0, 0] = 0
    if n_mics > 1:
        masks[wraps[0] - 1:wraps[0] + 2, 1] = 0
    if n_mics > 2:
        masks[:, 2] = 1
        masks[6:6 + long_gap, 2] = 0
        assert sum(frames[6:6 + long_gap]) > F and 6 + long_gap <= pushes - 4
    empty, ones = 3, 4
    masks[empty, :] = 0
    masks[ones, :] = 1
    out = [(n, None if k % 5 == 2 and not (n_mics > 2 and 6 <= k < 6 + long_gap) and k not in (0, empty, ones, wraps[0] - 1, wraps[0], wraps[0] + 1)
            else masks[k].copy()) for k, n in enumerate(frames)]
    assert any(p is None for _, p in out) and any(p is not None and p.all() for _, p in out) and any(p is not None and not p.any() for _, p in out)
    return out


def _present(p, m):
    return p is None or bool(p[m])


# ---- the reference: one single stream per microphone, pushed the pushes it is present in ---------------------------------------------
def _reference(K, c, g, x, chunk, sched, resets=None):
    """Per microphone m, per push k: None where m is absent, else S_m's outputs of that push (dict of [n_k][..]); the machine and
    S_m.frames_seen after every push. resets {k: [m, ..]}: before push k these microphones start over as new streams (reset_mic)."""
    resets = resets or {}
    on = dict(output_filter=True, fsm=K.fsm)
    outs, snaps, counts = [], [], []
    for m in range(x.shape[0]):
        s = K.stream(c, g, chunk, **on)
        o_m, s_m, c_m = [], [], []
        snap, k0 = start_machine(), 0
        for k, (n, p) in enumerate(sched):
            if m in resets.get(k, ()):
                s.close()
                s, snap = K.stream(c, g, chunk, **on), start_machine()
            if _present(p, m):
                o, machine = sd.drive_stream(K, c, g, x[m, k0 * s.hop:(k0 + n) * s.hop], [n], chunk=chunk, stream=s, filt=True, fsm=K.fsm)
                snap = machine if K.fsm else snap
                o_m.append({key: v for key, v in o.items() if v is not None})
            else:
                o_m.append(None)
            s_m.append(snap)
            c_m.append(s.frames_seen)
            k0 += n
        s.close()
        outs.append(o_m)
        snaps.append(s_m)
        counts.append(c_m)
    return outs, snaps, counts


def _garbage(x, sched, hop, seed=11):
    """The push buffers: x with the samples of every absent microphone replaced by noise over the whole int16 range."""
    rng = np.random.default_rng(seed)
    y, k0 = x.copy(), 0
    for n, p in sched:
        for m in range(x.shape[0]):
            if not _present(p, m):
                y[m, k0 * hop:(k0 + n) * hop] = rng.integers(-32768, 32768, n * hop).astype(np.int16)
        k0 += n
    return y


# ---- the bank ----------------------------------------------------------------------------------------------------------------------
def _bank_push(K, c, b, y, k0, n, p, mode):
    """One push of the bank in `mode`. Returns the dict of this push's outputs [n][n_mics][..] (host arrays), `fsm` among them."""
    got, machines = sd.drive_bank(K, c, b.geometry, y[:, k0 * b.hop:(k0 + n) * b.hop], [n], chunk=b.chunk, bank=b, filt=True, fsm=K.fsm,
                                  present=[p], mode=mode)
    got = {k: v for k, v in got.items() if v is not None}
    if K.fsm:
        got["fsm"] = machines
    return got


def _check_push(K, got, ref, k, n, p, n_mics, what):
    """Push k of the bank against the streams: the rows of the present microphones, the fill of the absent ones, every machine."""
    outs, snaps, _ = ref
    for m in range(n_mics):
        w = "%s push %d microphone %d " % (what, k, m)
        before = snaps[m][k - 1] if k else start_machine()
        for key, a in got.items():
            if key == "fsm":
                assert a[m] == snaps[m][k], (w + "machine", a[m], snaps[m][k])
            elif _present(p, m):
                same(a[:, m], outs[m][k][key], w + key)
            elif key == "fsm_states":
                same(a[:, m], np.full(n, before[0], np.int32), w + "fill of fsm_states")
            elif key in ("argmax", "likely", "spotted"):
                same(a[:, m], np.full(n, -1, np.int32), w + "fill of " + key)
            else:
                same(a[:, m], np.zeros((n, K.n_out), a.dtype), w + "fill of " + key)   # +0.0f: zero bytes
        if not _present(p, m) and K.fsm:
            assert snaps[m][k] == before


def _run(K, c, b, x, sched, ref, modes, what):
    """The whole schedule through a new or reset bank, push k in modes[k % len(modes)], checked push by push with the frame counts."""
    y = _garbage(x, sched, b.hop)
    k0 = 0
    for k, (n, p) in enumerate(sched):
        got = _bank_push(K, c, b, y, k0, n, p, modes[k % len(modes)])
        _check_push(K, got, ref, k, n, p, b.n_mics, what)
        k0 += n
        want = np.array([sum(nn for nn, pp in sched[:k + 1] if _present(pp, m)) for m in range(b.n_mics)], np.int64)
        counts = b.frames_seen_mics()
        assert counts.dtype == np.int64 and np.array_equal(counts, want), (what, k, counts, want)
        assert [int(v) for v in counts] == [ref[2][m][k] for m in range(b.n_mics)], (what, k)      # S_m.frames_seen
        assert b.frames_seen() == k0                                                              # the bank's: every push counts
    return k0


@pytest.mark.parametrize("chunk", [1, 3])
@pytest.mark.parametrize("kind,name", CASES)
def test_masked_pushes_equal_streams_pushed_when_present(built_lib, kind, name, chunk):
    """Filter and (10 outputs) machine on. Four phases on one bank with a reset in between, so that reset is tested with them: host
    pushes, device pushes into the caller's tensors, device pushes without output pointers, and the three alternating. The device
    phases of chunk 3 have ragged pushes; host pushes are always whole."""
    K, c, g = _open(kind, name)
    try:
        F = g.frame_count
        assert F - 1 > chunk
        full, ragged = _schedule(F, chunk, False), _schedule(F, chunk, True)
        x = recordings(g, M, sum(n for n, _ in full), 300 + chunk)      # the ragged schedule has fewer frames
        ref_full = _reference(K, c, g, x, chunk, full)
        ref_ragged = ref_full if chunk == 1 else _reference(K, c, g, x, chunk, ragged)
        b = _bank(K, c, g, M, chunk)
        assert np.array_equal(b.frames_seen_mics(), np.zeros(M, np.int64))
        for sched, ref, modes in ((full, ref_full, [HOST]), (ragged, ref_ragged, [DEV]), (ragged, ref_ragged, [DEV_NO_OUT]),
                                 (full, ref_full, [HOST, DEV, DEV_NO_OUT])):
            total = _run(K, c, b, x, sched, ref, modes, "%s %s chunk %d, %s:" % (kind, name, chunk, " / ".join(modes)))
            assert b.frames_seen() == total
            b.reset()
            assert b.frames_seen() == 0 and np.array_equal(b.frames_seen_mics(), np.zeros(M, np.int64))
        b.close()
    finally:
        c.close()


@pytest.mark.parametrize("kind,name", [("int8", "long"), ("float", "long"), ("float", "shipped_q15")])
def test_all_ones_mask_equals_the_maskless_push(built_lib, kind, name):
    """Two banks on the same samples, 20 pushes of chunk 3 with ragged ones (two wraps): one with an all-ones mask in every push, one
    without a mask. Host and device pushes."""
    K, c, g = _open(kind, name)
    try:
        chunk = 3
        for ragged, mode in ((False, HOST), (True, DEV)):
            frames = _frames(chunk, 20, ragged)
            x = recordings(g, 3, sum(frames), 71)
            a, b = _bank(K, c, g, 3, chunk), _bank(K, c, g, 3, chunk)
            k0 = 0
            for k, n in enumerate(frames):
                ga = _bank_push(K, c, a, x, k0, n, np.ones(3, np.uint8), mode)
                gb = _bank_push(K, c, b, x, k0, n, None, mode)
                for key in ga:
                    if key == "fsm":
                        assert ga[key] == gb[key]
                    else:
                        same(ga[key], gb[key], "%s push %d %s" % (mode, k, key))
                k0 += n
            assert np.array_equal(a.frames_seen_mics(), b.frames_seen_mics()) and list(a.frames_seen_mics()) == [k0] * 3
            a.close()
            b.close()
    finally:
        c.close()


@pytest.mark.parametrize("kind,name", [("int8", "shipped"), ("float", "shipped_q15"), ("float", "long")])
def test_reset_mic_of_an_absent_and_of_a_present_microphone(built_lib, kind, name):
    """Before push 9 microphone 1 (absent in pushes 8 and 9) and microphone 2 (present in both) are reset: from then on each equals a new
    stream pushed the later pushes it is present in; microphones 0 and 3 do not notice. reset_mic keeps the per-microphone counts."""
    K, c, g = _open(kind, name)
    try:
        chunk, cut = 1, 9
        sched = _schedule(g.frame_count, chunk, False, seed=9)[:30]
        for k in (cut - 1, cut):
            p = sched[k][1] if sched[k][1] is not None else np.ones(M, np.uint8)
            p[1], p[2] = 0, 1
            sched[k] = (sched[k][0], p)
        x = recordings(g, M, sum(n for n, _ in sched), 88)
        ref = _reference(K, c, g, x, chunk, sched, resets={cut: [1, 2]})
        b = _bank(K, c, g, M, chunk)
        _run(K, c, b, x, sched[:cut], ref, [DEV, HOST], "before reset_mic:")
        before = b.frames_seen_mics()
        b.reset_mic(1)
        b.reset_mic(2)
        assert np.array_equal(b.frames_seen_mics(), before) and b.frames_seen() == cut
        # the pushes from `cut` on: the same references, indexed from there
        rest = tuple([r_m[cut:] for r_m in r] for r in ref)
        y = _garbage(x, sched, b.hop)[:, cut * b.hop:]
        k0 = 0
        for k, (n, p) in enumerate(sched[cut:]):
            got = _bank_push(K, c, b, y, k0, n, p, (DEV, HOST)[k % 2])
            if k == 0:
                # push `cut` follows the resets. Microphones 0 and 3 go on; 1 is absent and holds a new stream's machine; 2 is present
                # and puts out a new stream's first push
                assert not p[1] and p[2]
                others = {key: ([a[0], a[3]] if key == "fsm" else a[:, [0, 3]]) for key, a in got.items()}
                _check_push(K, others, tuple([r[0], r[3]] for r in ref), cut, n, p[[0, 3]], 2, "push after reset_mic:")
                for key in K.keys(True, K.fsm):
                    same(got[key][:, 2], rest[0][2][0][key], "the reset present microphone " + key)
                if K.fsm:
                    assert got["fsm"][2] == rest[1][2][0] and got["fsm"][1] == start_machine() == rest[1][1][0]
                    assert (got["fsm_states"][:, 1] == start_machine()[0]).all()
                assert (got["argmax"][:, 1] == -1).all() and not sd.bits(got["filtered"][:, 1]).any()
            else:
                _check_push(K, got, rest, k, n, p, M, "after reset_mic:")
            k0 += n
        want = before + np.array([sum(n for n, p in sched[cut:] if _present(p, m)) for m in range(M)], np.int64)
        assert np.array_equal(b.frames_seen_mics(), want)
        b.close()
    finally:
        c.close()


@pytest.mark.parametrize("kind,name", [("int8", "long"), ("float", "long"), ("float", "shipped_q15")])
def test_a_bank_of_one_microphone_with_a_mask(built_lib, kind, name):
    """n_mics 1: the mask-less push and the masked one run the core's kernels at grid 1, the filter with a NULL mask and with the mask."""
    K, c, g = _open(kind, name)
    try:
        chunk = 3
        sched = [(n, None if k % 4 == 3 else np.array([k % 3 != 1], np.uint8)) for k, n in enumerate(_frames(chunk, 24, True))]
        assert len(sd.wraps([n for n, _ in sched], chunk)) >= 2
        x = recordings(g, 1, sum(n for n, _ in sched), 13)
        ref = _reference(K, c, g, x, chunk, sched)
        b = _bank(K, c, g, 1, chunk)
        _run(K, c, b, x, sched, ref, [DEV, DEV_NO_OUT], "one microphone:")
        b.close()
    finally:
        c.close()


@pytest.mark.parametrize("kind,name", [("int8", "shipped"), ("float", "shipped_q15")])
def test_errors(built_lib, kind, name):
    import torch
    from edison_amd import _lib
    L = _lib.lib()
    K, c, g = _open(kind, name)
    try:
        P = "edison_bank_" if kind == "int8" else "edison_fbank_"
        push, push_n, seen = (getattr(L, P + n) for n in ("push_present", "push_present_n_dev", "frames_seen_mics"))

        def fails(call):
            with pytest.raises(_lib.EdisonError) as e:
                call()
            assert e.value.code == _lib.E_ARGUMENT and K.who in str(e.value), str(e.value)

        b = _bank(K, c, g, 3, 2)
        dev = torch.device("cuda", c.device)
        x = np.zeros((3, 2 * g.frame_step), np.int16)
        xt = torch.from_numpy(x).to(dev)
        ok = torch.ones(3, dtype=torch.uint8, device=dev)
        counts = np.zeros(3, np.int64)
        # NULL bank, samples, counts
        assert push(None, x.ctypes.data, None, None, None, None) == _lib.E_ARGUMENT
        assert push(b._h, None, None, None, None, None) == _lib.E_ARGUMENT
        assert push_n(None, ctypes.c_void_p(xt.data_ptr()), None, 1, None, None, None) == _lib.E_ARGUMENT
        assert push_n(b._h, None, ctypes.c_void_p(ok.data_ptr()), 1, None, None, None) == _lib.E_ARGUMENT
        assert seen(None, counts.ctypes.data) == _lib.E_ARGUMENT and seen(b._h, None) == _lib.E_ARGUMENT
        # n_frames outside 1 .. chunk
        for n in (0, 3):
            fails(lambda: c._check(push_n(b._h, ctypes.c_void_p(xt.data_ptr()), ctypes.c_void_p(ok.data_ptr()), n, None, None, None)))
        # a mask of the wrong length or type
        for bad in (np.ones(2, np.uint8), np.ones(4, np.uint8), np.ones((3, 1), np.uint8), np.ones(3, np.int32), np.ones(3, np.float32)):
            fails(lambda: b.push(x, present=bad))
        for bad in (torch.ones(2, dtype=torch.uint8, device=dev), torch.ones(3, dtype=torch.int32, device=dev), torch.ones(3, dtype=torch.uint8)):
            fails(lambda: b.push_t(xt, present=bad))
        # nothing of that was counted, and the bank still works: a bool mask is a uint8 mask
        assert b.frames_seen() == 0 and list(b.frames_seen_mics()) == [0, 0, 0]
        out = b.push(x, present=np.array([True, False, True]))
        assert out["present"].dtype == np.uint8 and list(out["present"]) == [1, 0, 1] and list(out["argmax"][0] >= 0) == [True, False, True]
        assert b.frames_seen() == 2 and list(b.frames_seen_mics()) == [2, 0, 2]
        b.close()
    finally:
        c.close()

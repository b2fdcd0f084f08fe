"""MFCC variant C (the firmware's Q15 audioCalcMFCCs) on the GPU over every kernel instance, work split and DCT batch: the rows of
tests/q15_sweep.py at every frame count of q15_sweep.counts, which tests/test_q15_sweep_cpu.py proves to reach every case.

Per row and count, through the row's entry, every output inside three sentinel rows on either side:
  * hops below 1024: every output equals the oracle's on the same stream -- int16 coefficients, the int8 net input, the float output
    where the entry has one, and for the stages entries FFT, spectrum (bin 512 included) and mel rows;
  * hop 0 and hops from 1024 on: every frame's outputs are the bits of its base frame in the row's 64-frame call, at any position and
    in any DCT batch; the 64-frame call itself equals the oracle;
  * the host entry, the device entry at an even sample offset and (for the rows that run it) the device entry at an odd offset give
    the same bits on the same samples;
  * each optional output as NULL leaves the others unchanged and writes nothing.
The largest count, which forces a wave of every workgroup to park a full DCT batch and go on, runs once per shape x Nyquist through
the device entry, its audio tiled on the device. Then the KWS entry (31 frames per group) at two odd utterance strides.
All integer: every comparison is equality."""
import time

import numpy as np
import pytest

import q15_sweep as qs

pytestmark = pytest.mark.gpu

G = 3                                       # sentinel rows on either side of every output
FILL = dict(i16=0x5a5a, feat=99, f32=4321.0, fft=0x5a5a, spec=0x5a5a, mel=0x5a5a)
STATE = {"fb": None}


@pytest.fixture(scope="module")
def qctx(built_lib):
    """The one context of this module: its filterbank changes from row to row, which the session's shared context must not see"""
    from edison_amd.context import Context
    c = Context(0)
    STATE["fb"] = qs.SHIPPED
    yield c
    c.close()


def _configure(c, fb):
    if STATE["fb"] != fb:
        c.configure_mfcc(*fb)
        STATE["fb"] = fb


def _cols(row, stages):
    if stages:
        return dict(fft=(513, 2), spec=(513,), mel=(32,), i16=(32,))
    return dict(i16=(row["n_coef"],), feat=(row["n_coef"],), f32=(row["n_coef"],))


def _outputs_of(entry):
    if entry in qs.STAGE_ENTRIES:
        return ("fft", "spec", "mel", "i16")
    return ("f32", "feat") if entry == "float" else ("i16", "feat")


def _dtype(k):
    return np.int8 if k == "feat" else np.float32 if k == "f32" else np.int16


def _check_guards(what, bufs, n):
    for k, b in bufs.items():
        assert bool((b[:G] == FILL[k]).all()) and bool((b[G + n:] == FILL[k]).all()), (what, k, n, "a sentinel row changed")


def call_host(c, row, x, n, hop, kind, want):
    """kind "batch" / "float" / "stages" through the host entry points, outputs `want` (the others NULL) inside sentinel rows"""
    from edison_amd import _lib
    from edison_amd.context import _np_ptr
    x = np.ascontiguousarray(x)
    keys = _outputs_of("stages" if kind == "stages" else "float" if kind == "float" else "host")
    cols = _cols(row, kind == "stages")
    bufs = {k: np.full((n + 2 * G,) + cols[k], FILL[k], _dtype(k)) for k in keys}
    p = {k: (_np_ptr(bufs[k][G:G + n]) if k in want else None) for k in keys}
    if kind == "stages":
        r = c._L.edison_mfcc_q15_stages(c._h, _np_ptr(x), n, hop, p["fft"], p["spec"], p["mel"], p["i16"])
    elif kind == "float":
        r = c._L.edison_mfcc_batch(c._h, _np_ptr(x), n, hop, _lib.MFCC_C, row["n_coef"], p["f32"], p["feat"], 1.0)
    else:
        r = c._L.edison_mfcc_q15_batch(c._h, _np_ptr(x), n, hop, row["n_coef"], p["i16"], p["feat"])
    c._check(r)
    _check_guards((row["name"], "host", kind), bufs, n)
    for k in keys:
        if k not in want:
            assert (bufs[k] == FILL[k]).all(), (row["name"], k, "a NULL output was written")
    return {k: bufs[k][G:G + n] for k in want}


def call_dev(c, row, a, n, hop, kind, want):
    """The same through the device entry points on the int16 CUDA tensor `a` (a view at the offset under test)"""
    import torch
    from edison_amd import _lib
    keys = _outputs_of("stages" if kind == "stages" else "float" if kind == "float" else "host")
    cols = _cols(row, kind == "stages")
    tt = {np.int8: torch.int8, np.int16: torch.int16, np.float32: torch.float32}
    bufs = {k: torch.full((n + 2 * G,) + cols[k], FILL[k], dtype=tt[_dtype(k)], device=a.device) for k in keys}
    p = {k: (bufs[k][G:G + n] if k in want else None) for k in keys}
    c.use_torch_stream()
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "stages":
            c.mfcc_q15_stages_t(a, n, hop, fft=p["fft"], spec=p["spec"], mel=p["mel"], mfcc=p["i16"])
        elif kind == "float":
            c.mfcc_t(a, n, hop, variant=_lib.MFCC_C, n_coef=row["n_coef"], out=p["f32"], feat=p["feat"])
        else:
            c.mfcc_q15_t(a, n, hop, row["n_coef"], out=p["i16"], feat=p["feat"])
        torch.cuda.synchronize()
        STATE["last_call_s"] = time.perf_counter() - t0
    finally:
        c.use_own_stream()
    _check_guards((row["name"], "device", kind), bufs, n)
    for k in keys:
        if k not in want:
            assert bool((bufs[k] == FILL[k]).all()), (row["name"], k, "a NULL output was written")
    return {k: bufs[k][G:G + n] for k in want}


def _to_dev(c, x, offset):
    """x on the device at `offset` samples into a fresh (256-byte aligned) allocation"""
    import torch
    buf = torch.zeros(x.size + offset, dtype=torch.int16, device=torch.device("cuda", c.device))
    buf[offset:] = torch.from_numpy(x)
    a = buf[offset:]
    assert a.data_ptr() % 4 == (2 * offset) % 4
    return a


def _kind(row):
    return "stages" if row["entry"] in qs.STAGE_ENTRIES else "float" if row["entry"] == "float" else "batch"


def _np(d):
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in d.items()}


def _same(what, got, want, idx=None):
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        same = a.view(np.uint32) == b.view(np.uint32) if a.dtype == np.float32 else a == b
        if not same.all():
            at = np.argwhere(~same)[0]
            f = int(at[0])
            raise AssertionError("%s: %s of frame %d%s at %s: got %r want %r (%d values differ)" % (
                what, k, f, "" if idx is None else " (base %d)" % idx[f], at[1:].tolist(), a[tuple(at)], b[tuple(at)], int((~same).sum())))


def oracle_ref(row, x, n, hop, keys):
    """What the oracle says the outputs `keys` of n frames of x are"""
    stages = "fft" in keys
    r = qs.oracle_outputs(row, x, n, stages=stages, hop=hop)
    mfcc, st = r if stages else (r, None)
    nc = 32 if stages else row["n_coef"]
    out = dict(i16=np.ascontiguousarray(mfcc[:, :nc]), feat=qs.net_input(mfcc, nc), f32=mfcc[:, :nc].astype(np.float32))
    if stages:
        out.update(fft=st["fft"], spec=st["spectrogram"], mel=st["mel_spectrogram"])
    return {k: out[k] for k in keys}


@pytest.mark.parametrize("name", list(qs.ROWS))
def test_row(qctx, oracle_mod, name):
    import torch
    c, row = qctx, qs.ROWS[name]
    hop, kind, keys = row["hop"], _kind(row), _outputs_of(row["entry"])
    n_cu = c.device_info()["n_cu"]
    _configure(c, row["fb"])
    base, where = qs.base_frames(row)
    own = qs.ptr_offset(row)
    device = row["entry"] in qs.DEVICE_ENTRIES

    def primary(x, n, h, want=keys):
        return _np(call_dev(c, row, _to_dev(c, x, 2 if own == 0 else own), n, h, kind, want) if device else call_host(c, row, x, n, h, kind, want))
    B = None
    if qs.whole(row):                                   # the 64 base frames alone: what every later frame must equal, itself the oracle's
        B = primary(base.reshape(-1), qs.N_BASE, qs.FRAME_LEN)
        _same(name + " 64-frame call against the oracle", B, oracle_ref(row, base.reshape(-1), qs.N_BASE, qs.FRAME_LEN, keys))
    counts = qs.counts(row, n_cu)
    small = [n for n in counts if n <= 5 * qs.eq_wpb() * n_cu + 7]
    print("%s: instance %s, counts %s" % (name, qs.instance(row), counts))
    for n in small:
        assert qs.cases(row, n, n_cu), (name, n)
        x, idx = qs.audio(row, n, base)
        got = primary(x, n, hop)
        if B is None:
            _same("%s n=%d against the oracle" % (name, n), got, oracle_ref(row, x, n, hop, keys), idx)
        else:
            _same("%s n=%d against its base frame" % (name, n), got, {k: B[k][idx] for k in keys}, idx)
        # the other entries on the same samples: host, device at an even offset (the row's own is one of them unless it is odd)
        if device:
            _same("%s n=%d host against the row's entry" % (name, n), _np(call_host(c, row, x, n, hop, kind, keys)), got, idx)
        if not device or own:
            _same("%s n=%d device at an even offset against the row's entry" % (name, n), _np(call_dev(c, row, _to_dev(c, x, 0), n, hop, kind, keys)), got, idx)
        # each optional output as NULL leaves the others unchanged (call_* also checks that nothing was written for it)
        if n in (qs.eq_wpb() + 1, small[-1]):
            for drop in keys:
                rest = tuple(k for k in keys if k != drop)
                _same("%s n=%d with %s NULL" % (name, n, drop), primary(x, n, hop, rest), {k: got[k] for k in rest}, idx)
    if row["big"]:
        n = counts[-1]
        assert qs.BIG_CASE in qs.cases(row, n, n_cu) and n > small[-1]
        dev = torch.device("cuda", c.device)
        if hop == 0:
            a, idx = _to_dev(c, base[where["hop0"]], own), np.full(n, where["hop0"])
        else:
            assert hop == qs.FRAME_LEN
            idx = qs.tile_index(n)
            buf = torch.empty(n * qs.FRAME_LEN + own, dtype=torch.int16, device=dev)
            buf[own:].copy_(torch.from_numpy(base).to(dev)[torch.from_numpy(idx).to(dev)].reshape(-1))
            a = buf[own:]
        got = _np(call_dev(c, row, a, n, hop, kind, keys))
        print("%s: the largest count, %d frames (%d workgroups of at least %d): %.2f ms wall for the call" % (
            name, n, qs.blocks(n, n_cu, row["shape"]), min(cnt for _, cnt in qs.split(n, n_cu, row["shape"])), 1e3 * STATE["last_call_s"]))
        _same("%s n=%d against its base frame" % (name, n), got, {k: B[k][idx] for k in keys}, idx)


@pytest.mark.parametrize("stride", qs.KWS_STRIDES)
def test_kws_q15_at_odd_strides(qctx, oracle_mod, oracle_model, stride):
    """edison_kws_batch_q15*: 31 frames per group, group_stride = utt_stride odd, so every utterance but the first starts on an odd
    sample and the unaligned instance runs; features = net_input_q15(mfcc_q15(utterance)), logits and argmax = oracle.cnn"""
    import torch
    c, row = qctx, qs.ROWS["shipped"]
    _configure(c, qs.SHIPPED)
    n_cu = c.device_info()["n_cu"]
    base, _ = qs.base_frames(row)
    L = qs.UTT_FRAMES * qs.FRAME_LEN
    dev = torch.device("cuda", c.device)
    for n_utt in qs.kws_n_utt(n_cu):
        tags = qs.cases(row, qs.UTT_FRAMES * n_utt, n_cu)
        total = (n_utt - 1) * stride + L
        x = base[qs.tile_index(-(-total // qs.FRAME_LEN))].reshape(-1)[:total].copy()
        frames = x[(np.arange(n_utt) * stride)[:, None] + np.arange(L)[None, :]].reshape(-1)
        mfcc = qs.oracle_outputs(row, frames, n_utt * qs.UTT_FRAMES, hop=qs.FRAME_LEN)
        feat = qs.net_input(mfcc, 13).reshape(n_utt, -1)
        o = oracle_mod.cnn(oracle_model, feat, n_threads=8)
        r = c.kws(x, n_utt=n_utt, utt_stride=stride, q15=True)
        print("stride %d, %d utterances (%d frames): %s" % (stride, n_utt, 31 * n_utt, sorted(tags)))
        what = "stride %d n_utt %d" % (stride, n_utt)
        _same(what + " host", dict(feat=r["feat"], logits=r["logits"], softmax=r["softmax"], argmax=r["argmax"]),
              dict(feat=feat, logits=o["logits"], softmax=o["softmax"], argmax=o["argmax"].astype(np.int32)))
        # the device entry, features inside sentinel rows
        fb = torch.full((n_utt + 2 * G, feat.shape[1]), 99, dtype=torch.int8, device=dev)
        lg = torch.zeros((n_utt, 10), dtype=torch.int8, device=dev)
        am = torch.zeros(n_utt, dtype=torch.int32, device=dev)
        c.use_torch_stream()
        try:
            c.kws_t(_to_dev(c, x, 0), n_utt, stride, feat=fb[G:G + n_utt], logits=lg, argmax=am, q15=True)
            torch.cuda.synchronize()
        finally:
            c.use_own_stream()
        assert bool((fb[:G] == 99).all()) and bool((fb[G + n_utt:] == 99).all()), (what, "a sentinel row changed")
        _same(what + " device", dict(feat=fb[G:G + n_utt].cpu().numpy(), logits=lg.cpu().numpy(), argmax=am.cpu().numpy()),
              dict(feat=feat, logits=o["logits"], argmax=o["argmax"].astype(np.int32)))

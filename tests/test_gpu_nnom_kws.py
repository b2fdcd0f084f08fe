"""GPU tests of the NNoM example end to end on MFCC variant D: the rows form of the extractor (edison_mfcc_f32_rows*), audio to label
in one call (edison_kws_f32_batch*, Context.kws_f32), the example's loop continuously (edison_f32_stream_predict*,
NnomKwsFrontEnd.predict) and aiNnomPredict on top of edison_nnom_predict. Every comparison is bit for bit.

  * rows form: each row against one flat edison_mfcc_f32_batch_dev call of its own (out, out_f32, logmel), at 1, 2, 3, 12 and 13 frames per
    row, row counts that give the frame totals of f32_sweep.counts (every work split of both kernels, odd and even totals, pairs that
    straddle rows), a row stride above and below a row's length, guard rows, NULL optional outputs; the generic kernel at a length
    padded to 256, and at padded 512 in a child process with EDISON_F32_GENERIC=1;
  * batch: feat = the rows form; logits / softmax / label = Context.net on it and tests/dscnn_ref.py on it (the reference-pinned half;
    the feature half keeps the bars of the f32 sweep); label / prob = edison_nnom_predict; a graph without Softmax and one with a single
    output; NULL feat; hop 0;
  * stream: any split of the events gives the same outputs; windows against the batch call, the restatement (tests/nnom_kws_ref.py)
    and a twin stream's push; push and predict mixed; reset; the event limit;
  * refusals leave every output untouched.
The graph is tests/golden/alt_models/dscnn_kws.h (input 12 x 10 x 1), the extractor mfcc_create(11, 1, 512, 8, 0.97): 10 features.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import f32_sweep as fs
import nnom_kws_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "golden", "alt_models", "dscnn_kws.h")
EXTRACTOR = dict(num_mfcc_features=11, feature_offset=1, frame_len=512, mfcc_dec_bits=8, preemph=0.97)
GENERIC = dict(num_mfcc_features=13, feature_offset=1, frame_len=200, mfcc_dec_bits=8, preemph=0.97)      # padded 256: the generic kernel
ROWS, N_OUT, HOP, UTT = 12, 10, 256, 256 * 13
FPRS = [1, 2, 3, 12, 13]
G = 3                                                                     # guard rows around every output


_BASE = []


def _audio(n, seed):
    """Speech-like int16 noise at a level that keeps the features off the saturation bounds: 2^18 samples made once, rotated by the
    seed and tiled"""
    if not _BASE:
        rng = np.random.default_rng(2026)
        w = rng.normal(0, 1, 1 << 18)
        for i in range(1, w.size):
            w[i] += 0.9 * w[i - 1]
        _BASE.append(np.clip(np.rint(w * (2500.0 / w.std())), -32768, 32767).astype(np.int16))
    return np.resize(np.roll(_BASE[0], -((seed * 9973) % (1 << 18))), n)


# ---- the rows form -------------------------------------------------------------------------------------------------------------------------
def row_counts(frame_len, fpr, n_cu, generic_env=False):
    """Row counts whose frame totals are f32_sweep's split-covering counts, rounded down and up to whole rows"""
    counts = fs.counts(dict(frame_len=frame_len), n_cu, generic_env)
    return sorted({max(1, c // fpr) for c in counts} | {-(-c // fpr) for c in counts} | {c // fpr + 1 for c in counts if c < 200})


def rows_against_flat(ctx, m, fpr, n_rows, stride, step, null_optional=False):
    """edison_mfcc_f32_rows_dev inside guard rows against one flat device call per row; returns the three outputs as numpy"""
    import torch
    dev = torch.device("cuda", ctx.device)
    n = n_rows * fpr
    x = _audio(ref.rows_staged(n_rows, stride, fpr, step, m.frame_len), 1000 * fpr + n_rows)
    a = torch.from_numpy(x).to(dev)
    bo = torch.full((n + 2 * G, m.n_out), 99, dtype=torch.int8, device=dev)
    bf = torch.full((n + 2 * G, m.n_out), 4321.0, dtype=torch.float32, device=dev)
    bl = torch.full((n + 2 * G, fs.N_FBANK), 4321.0, dtype=torch.float32, device=dev)
    wo, wf, wl = torch.empty((n, m.n_out), dtype=torch.int8, device=dev), torch.empty((n, m.n_out), dtype=torch.float32, device=dev), \
        torch.empty((n, fs.N_FBANK), dtype=torch.float32, device=dev)
    ctx.use_torch_stream()
    try:
        m.rows_t(a, n_rows, stride, fpr, step, bo[G:G + n], None if null_optional else bf[G:G + n], None if null_optional else bl[G:G + n])
        if fpr == 1:                                                      # one frame per row is the flat call with frame_step = row_stride
            m.compute_t(a, n_rows, stride, wo, wf, wl)
        else:
            for u in range(n_rows):
                s = slice(u * fpr, (u + 1) * fpr)
                m.compute_t(a[u * stride:], fpr, step, wo[s], wf[s], wl[s])
        torch.cuda.synchronize()
    finally:
        ctx.use_own_stream()
    tag = (fpr, n_rows, stride, step)
    for what, b, g in (("out", bo, 99), ("out_f32", bf, 4321.0), ("logmel", bl, 4321.0)):
        assert bool((b[:G] == g).all()) and bool((b[G + n:] == g).all()), (tag, what, "a guard row changed")
    assert torch.equal(bo[G:G + n], wo), (tag, "int8", torch.nonzero(bo[G:G + n] != wo)[:1].tolist())
    if null_optional:
        assert bool((bf == 4321.0).all()) and bool((bl == 4321.0).all()), (tag, "a NULL output was written")
    else:
        assert torch.equal(bf[G:G + n].view(torch.int32), wf.view(torch.int32)), (tag, "float")
        assert torch.equal(bl[G:G + n].view(torch.int32), wl.view(torch.int32)), (tag, "log-mel")
    return x, bo[G:G + n].cpu().numpy(), bf[G:G + n].cpu().numpy(), bl[G:G + n].cpu().numpy()


def rows_sweep(ctx, m, fpr, generic_env=False, strides=("gap", "overlap", "hop")):
    """One extractor at `fpr` frames per row over every row count of row_counts; returns the frame totals it ran"""
    n_cu = ctx.device_info()["n_cu"]
    step = m.frame_len // 2
    span = (fpr - 1) * step + m.frame_len
    counts = row_counts(m.frame_len, fpr, n_cu, generic_env)
    totals = []
    for kind in strides:
        stride = {"gap": span + 37, "overlap": max(span // 3, 1), "hop": fpr * step}[kind]
        for n_rows in (counts if kind == "gap" else [c for c in counts if c * fpr < 200] + counts[-2:-1]):
            rows_against_flat(ctx, m, fpr, n_rows, stride, step)
            totals.append(n_rows * fpr)
        rows_against_flat(ctx, m, fpr, counts[1 % len(counts)], stride, step, null_optional=True)
    return totals


@pytest.mark.parametrize("fpr", FPRS)
def test_rows_form_fast_kernel(ctx, fpr):
    from edison_amd.mfcc.mfcc_f32 import MfccF32
    m = MfccF32(ctx=ctx, **EXTRACTOR)
    n_cu = ctx.device_info()["n_cu"]
    totals = rows_sweep(ctx, m, fpr)
    seen = set().union(*(fs.cases(dict(frame_len=512), t, n_cu) for t in totals))
    print("fast kernel, %d frames per row: totals %s" % (fpr, sorted(set(totals))))
    if fpr == 1:
        assert seen == set(fs.FAST_CASES), set(fs.FAST_CASES) - seen
    assert {t % 2 for t in totals} == ({0, 1} if fpr % 2 else {0})
    assert "fast: at least three queue draws per wave" in seen and "fast: uneven slices" in seen
    # the host entry point, and frames_per_row = 1 as the flat call with frame_step = row_stride
    n_rows, stride = 7, (fpr - 1) * 256 + 512 + 37
    x, o, f, l = rows_against_flat(ctx, m, fpr, n_rows, stride, 256)
    ho, hf, hl = m.rows(x, n_rows, stride, fpr, 256, want_float=True)
    assert np.array_equal(ho.reshape(o.shape), o) and np.array_equal(hf.reshape(f.shape).view(np.uint32), f.view(np.uint32)) \
        and np.array_equal(hl.reshape(l.shape).view(np.uint32), l.view(np.uint32))
    assert np.array_equal(m.rows(x, n_rows, stride, fpr, 256).reshape(o.shape), o)             # NULL out_f32 / logmel, host
    if fpr == 1:
        fo, ff, fl = m.compute(x, n_frames=n_rows, frame_step=stride, want_float=True)
        assert np.array_equal(fo, o) and np.array_equal(ff.view(np.uint32), f.view(np.uint32)) and np.array_equal(fl.view(np.uint32), l.view(np.uint32))
    m.close()


@pytest.mark.parametrize("fpr", FPRS)
def test_rows_form_generic_kernel(ctx, fpr):
    from edison_amd.mfcc.mfcc_f32 import MfccF32
    m = MfccF32(ctx=ctx, **GENERIC)
    assert fs.kernel(dict(frame_len=m.frame_len)) == "generic"
    n_cu = ctx.device_info()["n_cu"]
    totals = rows_sweep(ctx, m, fpr, strides=("gap", "overlap"))
    seen = set().union(*(fs.cases(dict(frame_len=m.frame_len), t, n_cu) for t in totals))
    if fpr == 1:
        assert seen == set(fs.GENERIC_CASES), set(fs.GENERIC_CASES) - seen
    assert any("grid stride" in c for c in seen)
    m.close()


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch
import test_gpu_nnom_kws as T
from edison_amd.context import default_context
from edison_amd.mfcc.mfcc_f32 import MfccF32
ctx = default_context()
m = MfccF32(ctx=ctx, **T.EXTRACTOR)
for fpr in T.FPRS:
    T.rows_sweep(ctx, m, fpr, generic_env=True, strides=("gap",))
x, o, f, l = T.rows_against_flat(ctx, m, 3, 7, 1500, 256)
np.savez(sys.argv[2], o=o, f=f)
print("ok")
"""


def test_rows_form_generic_kernel_at_padded_512(ctx, tmp_path):
    """EDISON_F32_GENERIC=1 is read once per process: a fresh child runs the rows form on the generic kernel at the fast kernel's length"""
    from edison_amd.mfcc.mfcc_f32 import MfccF32
    script, out = tmp_path / "rows_generic.py", tmp_path / "rows_generic.npz"
    script.write_text(CHILD)
    env = dict(os.environ, EDISON_F32_GENERIC="1")
    p = subprocess.run([sys.executable, "-u", str(script), os.path.dirname(HERE), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-1000:] + p.stderr[-3000:]
    m = MfccF32(ctx=ctx, **EXTRACTOR)
    _, o, f, _ = rows_against_flat(ctx, m, 3, 7, 1500, 256)
    d = np.load(str(out))
    assert np.abs(d["o"].astype(int) - o.astype(int)).max() <= 1
    assert (d["f"].view(np.uint32) != f.view(np.uint32)).any(), "the child did not run the other kernel: EDISON_F32_GENERIC was not honoured"
    m.close()


# ---- graphs --------------------------------------------------------------------------------------------------------------------------------
def _layers():
    from edison_amd import nnom_import
    with open(HEADER) as f:
        return nnom_import.parse_weights_h(f.read())


def blob_kws():
    from edison_amd import nnom_import
    shape, layers = _layers()
    return nnom_import.build_blob(shape, layers)


def blob_without_softmax():
    from edison_amd import nnom_import
    shape, layers = _layers()
    assert layers[-1]["type"] == nnom_import.T_SOFTMAX
    return nnom_import.build_blob(shape, layers[:-1])


def blob_one_output():
    """The graph's body in front of a Dense layer with a single output and no Softmax"""
    from edison_amd import nnom_import
    shape, layers = _layers()
    d = layers[-2]
    assert d["type"] == nnom_import.T_DENSE
    rng = np.random.default_rng(5)
    one = dict(type=nnom_import.T_DENSE, out=1, w=rng.integers(-40, 41, d["w"].size // d["out"]).astype(np.int8), b=np.array([3], np.int8),
               out_rshift=d["out_rshift"] - 2, bias_lshift=d["bias_lshift"], relu=0)
    return nnom_import.build_blob(shape, layers[:-2] + [one])


def blob_dense_only(in_shape):
    """Input in_shape -> Dense(4) -> Softmax: a graph of another input shape, for the refusals"""
    from edison_amd import nnom_import
    rng = np.random.default_rng(in_shape[0] * 100 + in_shape[1])
    n_in = in_shape[0] * in_shape[1] * in_shape[2]
    dn = dict(type=nnom_import.T_DENSE, out=4, w=rng.integers(-40, 41, 4 * n_in).astype(np.int8), b=np.zeros(4, np.int8), out_rshift=9, bias_lshift=0, relu=0)
    return nnom_import.build_blob(in_shape, [dn, dict(type=nnom_import.T_SOFTMAX)])


def _open(blob):
    from edison_amd.context import Context
    from edison_amd.mfcc.mfcc_f32 import MfccF32
    c = Context(0, model_path=None)
    if blob is not None:
        c.load_model_bytes(blob)
    return c, MfccF32(ctx=c, **EXTRACTOR)


@pytest.fixture(scope="module")
def kws(built_lib):
    """(context with the DS-CNN loaded, its extractor, the blob): shared, nothing in it is changed by a test"""
    blob = blob_kws()
    c, m = _open(blob)
    assert m.n_out == N_OUT
    yield c, m, blob
    m.close(); c.close()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_batch(c, m, blob, audio, n, stride):
    """One edison_kws_f32_batch call against the rows form, Context.net, the numpy restatement of the graph and edison_nnom_predict"""
    import dscnn_ref
    from edison_amd.mfcc.mfcc_f32 import nnom_predict
    info = c.net_info()
    r = c.kws_f32(m, audio, n_utt=n, utt_stride=stride, hop=HOP)
    feat = m.rows(audio, n, stride, ROWS, HOP).reshape(n, -1)
    assert np.array_equal(r["feat"], feat)
    o, want = c.net(feat), dscnn_ref.run(blob, feat)
    assert np.array_equal(r["logits"], o["logits"]) and np.array_equal(r["logits"], want["logits"])
    if info["has_softmax"]:
        assert np.array_equal(r["softmax"], o["softmax"]) and np.array_equal(r["softmax"], want["softmax"])
    else:
        assert r["softmax"] is None and want["softmax"] is None
    last = r["softmax"] if info["has_softmax"] else r["logits"]
    label, prob = nnom_predict(last, info["n_out"])
    wl, wp = ref.predict_rule(last)
    assert np.array_equal(r["label"], label) and np.array_equal(label, wl) and _same_bits(r["prob"], prob) and _same_bits(prob, wp)
    if info["n_out"] > 1:
        assert np.array_equal(r["label"], o["argmax"].astype(np.uint32)) and np.array_equal(o["argmax"], want["argmax"])
    for other in (c.kws_f32(m, audio, n_utt=n, utt_stride=stride, hop=HOP, want_feat=False), c.kws_f32(m, audio, n_utt=n, utt_stride=stride, hop=0)):
        for k in ("logits", "softmax", "label"):
            assert (r[k] is None and other[k] is None) or np.array_equal(r[k], other[k]), k
        assert _same_bits(r["prob"], other["prob"])
    return r


def _batches(blob):
    import plan_emulator
    ipw = int(plan_emulator.Plan(blob).M.batch)
    return sorted({1, max(ipw - 1, 1), ipw + 1, 3 * ipw + 2})


def test_batch(kws):
    c, m, blob = kws
    ns = _batches(blob)
    stride = UTT + 19
    audio = _audio((ns[-1] - 1) * stride + UTT, 31)
    for n in ns:
        r = check_batch(c, m, blob, audio, n, stride)
    print("labels", r["label"].tolist(), "prob", r["prob"].tolist())
    # default stride: utterances back to back; and the device form with every optional output NULL
    import torch
    n = ns[-1]
    back = c.kws_f32(m, audio, n_utt=n)
    assert np.array_equal(back["feat"], m.rows(audio, n, UTT, ROWS, HOP).reshape(n, -1))
    dev = torch.device("cuda", c.device)
    a, lab = torch.from_numpy(audio).to(dev), torch.full((n + 2,), 77, dtype=torch.int32, device=dev)
    c.use_torch_stream()
    try:
        c.kws_f32_t(m, a, n, stride, lab[1:n + 1])
        torch.cuda.synchronize()
    finally:
        c.use_own_stream()
    assert lab[0] == 77 and lab[-1] == 77 and np.array_equal(lab[1:n + 1].cpu().numpy().astype(np.uint32), r["label"])


def test_batch_graph_without_softmax_and_single_output():
    for make, n_out in ((blob_without_softmax, 10), (blob_one_output, 1)):
        blob = make()
        c, m = _open(blob)
        try:
            info = c.net_info()
            assert info["n_out"] == n_out and not info["has_softmax"]
            ns = _batches(blob)
            audio = _audio(ns[-1] * UTT, 32 + n_out) // (3 if n_out == 1 else 1)
            for n in ns:
                r = check_batch(c, m, blob, audio, n, UTT)
            print("%d outputs, no Softmax: logits %s labels %s prob %s" % (n_out, r["logits"][:, 0].tolist(), r["label"].tolist(), r["prob"].tolist()))
            if n_out == 1:
                assert np.array_equal(r["label"], (r["logits"][:, 0] >= 64).astype(np.uint32))
        finally:
            m.close(); c.close()


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
N_EV = 14


def _front_end(c, max_events=16):
    from edison_amd.mfcc.mfcc_f32 import NnomKwsFrontEnd
    return NnomKwsFrontEnd(ctx=c, window_rows=ROWS, max_events=max_events, num_mfcc_features=11, feature_offset=1)


def _cat(parts):
    return {k: (None if parts[0][k] is None else np.concatenate([p[k] for p in parts])) for k in ("logits", "softmax", "label", "prob")}


def _equal(a, b, lo=0, hi=None):
    for k in ("logits", "softmax", "label"):
        assert np.array_equal(a[k][lo:hi], b[k]), k
    assert _same_bits(a["prob"][lo:hi], b["prob"])


@pytest.fixture(scope="module")
def streamed(kws):
    """14 events pushed at once: the outputs every other split must reproduce, and the samples"""
    c, m, blob = kws
    x = _audio(N_EV * 512, 33)
    fe = _front_end(c)
    whole = fe.predict(x, labels=["c%d" % i for i in range(10)])
    assert fe.events_seen == N_EV and whole["names"] == ["c%d" % i for i in whole["label"]]
    for v in whole.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    yield x, whole, fe
    fe.close()


def test_stream_splits_and_reset(kws, streamed):
    c, m, blob = kws
    x, whole, fe = streamed
    for split in ([1, 2, 5, 6], [1] * N_EV):
        fe.reset()
        assert fe.events_seen == 0
        parts, at = [], 0
        for k in split:
            parts.append(fe.predict(x[at * 512:(at + k) * 512]))
            at += k
        _equal(whole, _cat(parts))
        assert fe.events_seen == N_EV


def test_stream_windows(kws, streamed):
    c, m, blob = kws
    x, whole, _ = streamed
    import dscnn_ref
    y = np.concatenate([np.zeros(256, np.int16), x])
    # windows 5 .. 13 are whole utterances of the batch call over [256 zeros | x] at a stride of one event
    b = c.kws_f32(m, y, n_utt=N_EV - 5, utt_stride=512, hop=HOP)
    _equal(whole, b, 5)
    # every window, the first five with their zero rows: the restatement of the firmware's ring over the GPU's own feature rows
    seq = m.compute(y, n_frames=2 * N_EV, frame_step=256)
    windows = ref.sliding_windows(seq, ROWS)
    ring = ref.ring_loop(lambda fr: m.compute(fr, n_frames=1)[0], x, ROWS, N_OUT)
    assert np.array_equal(ring, windows) and not windows[0, :ROWS - 2].any() and not windows[4, :2].any() and windows[5].any(axis=1).all()
    assert np.array_equal(windows[5:].reshape(N_EV - 5, -1), b["feat"])
    twin = _front_end(c)
    pushed = twin.push(x)
    twin.close()
    assert np.array_equal(pushed, windows)
    o, want = c.net(pushed.reshape(N_EV, -1)), dscnn_ref.run(blob, pushed.reshape(N_EV, -1))
    for k in ("logits", "softmax"):
        assert np.array_equal(whole[k], o[k]) and np.array_equal(whole[k], want[k]), k
    assert np.array_equal(whole["label"], o["argmax"].astype(np.uint32))
    wl, wp = ref.predict_rule(whole["softmax"])
    assert np.array_equal(whole["label"], wl) and _same_bits(whole["prob"], wp)


def test_stream_push_and_predict_mixed(kws, streamed):
    c, m, blob = kws
    x, whole, fe = streamed
    twin = _front_end(c)
    pushed = twin.push(x)
    twin.close()
    fe.reset()
    p1 = fe.predict(x[:3 * 512])
    w = fe.push(x[3 * 512:7 * 512])
    p2 = fe.predict(x[7 * 512:])
    assert fe.events_seen == N_EV
    _equal(whole, p1, 0, 3)
    _equal(whole, p2, 7)
    assert np.array_equal(w, pushed[3:7])


def _stream_call(fe, x, n, n_out=10):
    """edison_f32_stream_predict with sentinel-filled outputs: (status, outputs)"""
    lo, so = np.full((max(n, 1), n_out), 99, np.int8), np.full((max(n, 1), n_out), 99, np.int8)
    lb, pr = np.full(max(n, 1), 0xabcd, np.uint32), np.full(max(n, 1), -3.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    r = fe._L.edison_f32_stream_predict(fe._h, p(x), n, p(lo), p(so), p(lb), p(pr))
    return r, (lo, so, lb, pr)


def _untouched(outs):
    lo, so, lb, pr = outs
    return bool((lo == 99).all() and (so == 99).all() and (lb == 0xabcd).all() and (pr == -3.0).all())


def test_stream_event_limit_and_empty_push(kws, streamed):
    from edison_amd import _lib
    c, m, blob = kws
    x, whole, _ = streamed
    fe = _front_end(c, max_events=4)
    first = fe.predict(x[:2 * 512])
    r, outs = _stream_call(fe, x, 5)
    assert r == _lib.E_SIZE and _untouched(outs) and fe.events_seen == 2
    r, outs = _stream_call(fe, x, 0)
    assert r == _lib.OK and _untouched(outs) and fe.events_seen == 2
    assert fe._L.edison_f32_stream_predict(fe._h, None, 0, None, None, None, None) == _lib.OK
    rest = fe.predict(x[2 * 512:])                                        # 12 events through a stream of 4: three calls inside predict()
    _equal(whole, first, 0, 2)
    _equal(whole, rest, 2)
    fe.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _batch_call(c, m, audio, n, n_out=10, in_n=120):
    ft, lo, so = np.full((n, in_n), 99, np.int8), np.full((n, n_out), 99, np.int8), np.full((n, n_out), 99, np.int8)
    lb, pr = np.full(n, 0xabcd, np.uint32), np.full(n, -3.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    r = c._L.edison_kws_f32_batch(c._h, m._h, p(audio), n, UTT, 0, p(ft), p(lo), p(so), p(lb), p(pr))
    return r, (ft == 99).all() and _untouched((lo, so, lb, pr)), (c._L.edison_last_error(c._h) or b"").decode()


def test_refusals(kws, ctx):
    from edison_amd import _lib
    from edison_amd.mfcc.mfcc_f32 import MfccF32
    audio = _audio(3 * UTT + 512, 34)
    # no model loaded
    c, m = _open(None)
    try:
        r, clean, msg = _batch_call(c, m, audio, 3)
        assert r == _lib.E_ARGUMENT and clean and "no int8 graph" in msg, (r, msg)
        fe = _front_end(c)
        r, outs = _stream_call(fe, audio, 2)
        assert r == _lib.E_ARGUMENT and _untouched(outs) and fe.events_seen == 0
        fe.close()
    finally:
        m.close(); c.close()
    # a graph of 12 x 12 x 1: refused by both; one of 13 x 10 x 1: a 12-row stream refuses it (for the batch call the graph gives the
    # window, so 13 rows of 10 features are simply another window length)
    c, m = _open(blob_dense_only((12, 12, 1)))
    try:
        r, clean, msg = _batch_call(c, m, audio, 3, n_out=4)
        assert r == _lib.E_SIZE and clean and "12 x 12 x 1" in msg and "x 10 x 1" in msg, (r, msg)
        fe = _front_end(c)
        r, outs = _stream_call(fe, audio, 2, n_out=4)
        msg = (c._L.edison_last_error(c._h) or b"").decode()
        assert r == _lib.E_SIZE and _untouched(outs) and fe.events_seen == 0 and "12 x 12 x 1" in msg and "12 x 10 x 1" in msg, (r, msg)
        fe.close()
        c.load_model_bytes(blob_dense_only((13, 10, 1)))
        fe = _front_end(c)
        r, outs = _stream_call(fe, audio, 2, n_out=4)
        msg = (c._L.edison_last_error(c._h) or b"").decode()
        assert r == _lib.E_SIZE and _untouched(outs) and fe.events_seen == 0 and "13 x 10 x 1" in msg and "12 x 10 x 1" in msg, (r, msg)
        fe.close()
        b = c.kws_f32(m, audio, n_utt=2, utt_stride=UTT)
        assert np.array_equal(b["feat"], m.rows(audio, 2, UTT, 13, HOP).reshape(2, -1)) and np.array_equal(b["softmax"], c.net(b["feat"])["softmax"])
        # an extractor with 12 features against the 12 x 10 graph of the shared context
        kc, km, _ = kws
        m12 = MfccF32(ctx=kc, num_mfcc_features=13, feature_offset=1)
        r, clean, msg = _batch_call(kc, m12, audio, 3)
        assert r == _lib.E_SIZE and clean and "12 x 10 x 1" in msg and "x 12 x 1" in msg, (r, msg)
        m12.close()
        # an extractor from another context
        other = MfccF32(ctx=ctx, **EXTRACTOR)
        r, clean, msg = _batch_call(kc, other, audio, 3)
        assert r == _lib.E_ARGUMENT and clean and "another context" in msg, (r, msg)
        other.close()
        assert kc.kws_f32(km, audio, n_utt=1)["label"].shape == (1,)      # the shared context still works
    finally:
        m.close(); c.close()


# ---- aiNnomPredict -------------------------------------------------------------------------------------------------------------------------
def test_ai_nnom_predict_on_the_shipped_model(built_lib, ctx, cnn_golden):
    """aiNnomPredict (now edison_nnom_predict on the softmax) returns what its inline formula returned: first maximum, max / sum in float32"""
    L = built_lib
    assert L.aiInitialize() == 0
    feats = np.ascontiguousarray(cnn_golden["feats"][:8], dtype=np.int8).reshape(8, -1)
    buf_in, buf_out = L.aiNnomGetInputBuffer(), L.aiNnomGetOutputBuffer()
    for f in feats:
        ctypes.memmove(buf_in, f.ctypes.data, f.size)
        label, prob = ctypes.c_uint32(123), ctypes.c_float(-1)
        assert L.aiNnomPredict(ctypes.byref(label), ctypes.byref(prob)) == 0
        out = np.frombuffer(ctypes.string_at(buf_out, 10), np.int8)
        s = int(out.astype(np.int32).sum())
        am = int(np.argmax(out))                                           # numpy's argmax is the first maximum
        want = np.float32(int(out[am])) / np.float32(s) if s != 0 else np.float32(0)
        assert label.value == am and np.float32(prob.value).view(np.uint32) == np.float32(want).view(np.uint32), (label.value, am, prob.value, want)
        assert np.array_equal(out, ctx.cnn(f)["softmax"][0])

"""The fast MFCC loop (ed_mfcc2_body, csrc/mfcc_kernels.hip) over every instance and work split it has: the rows of
tests/mfcc_sweep.py, which tests/test_mfcc_sweep_cpu.py proves to launch all 28 instances.

Every launch is made of the same 64 seeded frames (speech-level noise, the bench's two tones, quiet noise, silence, the two rails,
clipped noise). Per row:
  1. a base launch (64 frames, or the next whole number of rows / utterances / batches) against the float64 oracle with the project's
     bars (A and TF |d| <= 1e-3 + 1e-4 |ref|, B |d| <= 1e-2 + 1e-5 |ref|; TF on frames that pass the conditioning test
     of test_mfcc_tf_variant_against_the_float64_restatement); exact KWS mode bit for bit against oracle.net_input(oracle.mfcc());
     int8 features bit for bit round_half_even(clip(float32(coef) * feat_scale)) of the float32 the same launch wrote;
  2. at every frame count of mfcc_sweep.row_counts the batch is the base set at rotating positions, (f + f // 64) % 64 by frame slot,
     and every output row equals the base launch's row bit for bit;
  3. the outputs are views inside larger allocations: the guard rows in front and behind never change.
Across instances (test_addressing_does_not_change_a_bit): aligned / unaligned, plain / grouped / list on the same samples, variant and
table give the same float32 bits; the 2+5 and the forced 3+6 table of the shipped bank agree within 2e-6 x max |one|."""

import numpy as np
import pytest

import mfcc_sweep as ms

pytestmark = pytest.mark.gpu

TOL = {"A": (1e-3, 1e-4), "B": (1e-2, 1e-5), "TF": (1e-3, 1e-4)}      # B with the logarithm: variant A's bar (test_mfcc_overlap_unaligned_ncoef_log)
GUARD_F, GUARD_Q, GUARD_ROWS = 4321.0, 99, 2
RATIO = {}                                                            # variant -> largest |d| / (atol + rtol |ref|) seen


def base_frames():
    """[64, 1024] int16, seeded: 0 silence, 1 / 2 the rails, 3 / 4 noise clipped at both rails, 5..12 quiet (1 % of full scale),
    13..28 the bench's mix (noise + 1 kHz + 125 Hz tones), the rest speech-level noise; then shuffled."""
    rng = np.random.default_rng(2028)
    t = np.arange(ms.FRAME) / 16000.0
    f = rng.normal(0, 3000, (ms.N_BASE, ms.FRAME))
    f[0] = 0
    f[1], f[2] = 32767, -32768
    f[3:5] = rng.normal(0, 30000, (2, ms.FRAME))
    f[5:13] = rng.normal(0, 0.01 * 32767, (8, ms.FRAME))
    ph = rng.uniform(0, 2 * np.pi, (16, 2))
    f[13:29] += 1000 * np.cos(2 * np.pi * 1000 * t + ph[:, :1]) + 500 * np.cos(2 * np.pi * 125 * t + ph[:, 1:])
    x = np.clip(np.rint(f), -32768, 32767).astype(np.int16)
    assert (x[3:5] == 32767).any() and (x[3:5] == -32768).any()
    return x[rng.permutation(ms.N_BASE)]


def _oracle(oracle_mod, row, base):
    """float64 [64, 32] of the row's variant, logarithm and filterbank on the base frames, and which frames are held to it"""
    fs, lo, hi, _ = ms.FILTERBANKS[row["bank"]]
    ov = {"A": oracle_mod.VARIANT_A, "B": oracle_mod.VARIANT_B, "TF": oracle_mod.VARIANT_TF}[row["variant"]]
    kw = dict(use_log=row["log"], n_threads=4, sample_rate=fs, lower_edge_hertz=lo, upper_edge_hertz=hi)
    if row["variant"] != "TF":
        return oracle_mod.mfcc(base.reshape(-1), ov, **kw), np.ones(ms.N_BASE, bool)
    ref, st = oracle_mod.mfcc(base.reshape(-1), ov, stages=True, **kw)
    ok = st["mel_spectrogram"].min(axis=1) > 1e-5 * st["spectrogram"].max(axis=1)
    assert ok.sum() >= ms.N_BASE - 8, ok
    return ref, ok


class Dev:
    """The device side of a test: torch for memory only"""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx = torch, ctx
        self.dev = torch.device("cuda", ctx.device)
        self.base_np = base_frames()
        self.base = torch.from_numpy(self.base_np).to(self.dev)
        self.ar = torch.arange(ms.FRAME, device=self.dev)
        self.gen = torch.Generator(device=self.dev)
        self.gen.manual_seed(7)

    def index(self, n, shift=0):
        f = self.torch.arange(n, device=self.dev, dtype=self.torch.int64)
        return (f + f // ms.N_BASE + shift) % ms.N_BASE

    def audio(self, idx, off, hop, fpg, gstride):
        """A view `off` samples into an allocation of filler samples, with frame slot f = (g, i) = base[idx[f]] at g * gstride + i * hop"""
        torch, n = self.torch, idx.numel()
        f = torch.arange(n, device=self.dev, dtype=torch.int64)
        pos = (f // fpg) * gstride + (f % fpg) * hop
        span = int(pos.max()) + ms.FRAME
        buf = torch.randint(-3000, 3000, (off + span + 8,), generator=self.gen, device=self.dev, dtype=torch.int16)
        assert buf.data_ptr() % 4 == 0
        view = buf[off:]
        view[(pos[:, None] + self.ar[None, :]).reshape(-1)] = self.base[idx].reshape(-1)
        return view

    def guarded(self, n, nc, dtype):
        t = self.torch
        buf = t.full((n + 2 * GUARD_ROWS, nc), GUARD_F if dtype == t.float32 else GUARD_Q, dtype=dtype, device=self.dev)
        return buf, buf[GUARD_ROWS:GUARD_ROWS + n]

    def guards_intact(self, buf, n):
        g = GUARD_F if buf.dtype == self.torch.float32 else GUARD_Q
        return bool((buf[:GUARD_ROWS] == g).all()) and bool((buf[GUARD_ROWS + n:] == g).all())


def launch(d, ctx, row, n, shape, shift=0, outs=None):
    """Row `row` at n frames: (float32 [n, n_coef] or None, int8 or None, idx [n]) as device tensors; checks the guard rows and that
    the call is the instance the restated launch code says"""
    from edison_amd import _lib
    torch = d.torch
    outs = row["outs"] if outs is None else outs
    nc, hop = row["n_coef"], row["hop"]
    variant = ms.VARIANT_CODE[row["variant"]]
    vlog = variant | (_lib.MFCC_USE_LOG if row["log"] else 0)
    idx = d.index(n, shift)
    fpg, gs = ms.geometry(row, n)
    host = row["entry"] in ms.HOST_ENTRIES
    call = ms.call(row, n, shape)
    fbuf = qbuf = fo = qo = None
    if not host:
        if "f" in outs:
            fbuf, fo = d.guarded(n, nc, torch.float32)
        if "q" in outs and not ms.is_kws(row):
            qbuf, qo = d.guarded(n, nc, torch.int8)
    if row["entry"] == "mfcc_batches_t":
        each = n // ms.LIST_BATCHES
        audios = [d.audio(idx[b * each:(b + 1) * each], row["off"][b], hop, each, 0) for b in range(ms.LIST_BATCHES)]
        call["ptrs"] = [a.data_ptr() for a in audios]
        fl = [d.guarded(each, nc, torch.float32) for _ in audios] if "f" in outs else None
        ql = [d.guarded(each, nc, torch.int8) for _ in audios] if "q" in outs else None
        ctx.mfcc_batches_t(audios, each, hop, variant, nc, outs=[v for _, v in fl] if fl else None, feats=[v for _, v in ql] if ql else None,
                           feat_scale=row["feat_scale"], use_log=row["log"])
        torch.cuda.synchronize()
        for lst in (fl, ql):
            assert lst is None or all(d.guards_intact(b, each) for b, _ in lst), (row["name"], n, "a guard row of a batch's output changed")
        fo = torch.cat([v for _, v in fl]) if fl else None
        qo = torch.cat([v for _, v in ql]) if ql else None
    else:
        a = d.audio(idx, row["off"], hop, fpg, gs)
        call["ptr"] = 0 if host else a.data_ptr()
        if row["entry"] == "mfcc_t":
            ctx.mfcc_t(a, n, hop, variant, nc, out=fo, feat=qo, feat_scale=row["feat_scale"], use_log=row["log"])
        elif row["entry"] == "mfcc_rows_t":
            ctx.mfcc_rows_t(a, n // fpg, gs, fpg, hop, vlog, nc, out=fo, feat=qo, feat_scale=row["feat_scale"])
        elif row["entry"] == "mfcc":
            r = ctx.mfcc(a.cpu().numpy(), n_frames=n, frame_step=hop, variant=variant, n_coef=nc, use_log=row["log"], want_feat="q" in outs,
                         feat_scale=row["feat_scale"])
            fo, qo = (r if "q" in outs else (r, None))
            fo, qo = torch.from_numpy(fo).to(d.dev), (None if qo is None else torch.from_numpy(qo).to(d.dev))
        elif row["entry"] == "mfcc_rows":
            x = a.cpu().numpy()
            need = n // fpg * gs
            rows = np.concatenate([x, np.zeros(max(0, need - x.size), np.int16)])[:need].reshape(n // fpg, gs)
            fo = torch.from_numpy(ctx.mfcc_rows(rows, fpg, frame_step=hop, variant=variant, n_coef=nc, use_log=row["log"]).reshape(n, nc)).to(d.dev)
        elif row["entry"] == "kws_t":
            n_utt = n // ms.UTT_FRAMES
            qbuf, qo = d.guarded(n_utt, 13 * ms.UTT_FRAMES, torch.int8)
            am = torch.zeros((n_utt,), dtype=torch.int32, device=d.dev)
            ctx.kws_t(a, n_utt, gs, feat=qo, argmax=am, exact=True)
        elif row["entry"] == "kws":
            n_utt = n // ms.UTT_FRAMES
            x = a.cpu().numpy()
            qo = torch.from_numpy(ctx.kws(x, n_utt=n_utt, utt_stride=gs, exact=True)["feat"]).to(d.dev)
        else:
            raise ValueError(row["entry"])
        torch.cuda.synchronize()
        if ms.is_kws(row):
            if qbuf is not None:
                assert d.guards_intact(qbuf, n // ms.UTT_FRAMES), (row["name"], n, "a guard row of the features changed")
            qo = qo.reshape(n, 13)
        else:
            assert fbuf is None or d.guards_intact(fbuf, n), (row["name"], n, "a guard row of the float32 output changed")
            assert qbuf is None or d.guards_intact(qbuf, n), (row["name"], n, "a guard row of the int8 output changed")
    if row["note"]:
        assert ms.instance(call) == ms.note_instance(row["note"]), (row["name"], n, ms.instance(call))
    return fo, qo, idx


def _quantised(d, fo, scale):
    """round_half_even(clip(float32(coef) * float32(scale), -128, 127)) as int8"""
    torch = d.torch
    s = torch.tensor(np.float32(scale), device=d.dev)
    return torch.round(torch.clamp(fo * s, -128.0, 127.0)).to(torch.int8)


def _gather_base(d, outs):
    """[(tensor [n, c], idx)] -> [64, c]: the row of every base frame; a frame that came twice gave the same row twice"""
    torch = d.torch
    c = outs[0][0].shape[1]
    R = torch.zeros((ms.N_BASE, c), dtype=outs[0][0].dtype, device=d.dev)
    seen = torch.zeros(ms.N_BASE, dtype=torch.bool, device=d.dev)
    for o, idx in outs:
        R[idx] = o
        seen[idx] = True
    assert bool(seen.all())
    for o, idx in outs:
        assert torch.equal(R[idx], o), "one frame, two results within the base launches"
    return R


class _Ctx:
    """The context of a bank: the session's for the shipped bank, otherwise one of its own (EDISON_FORCE_WIDE_MEL is read when a
    context builds its tables)"""

    def __init__(self, ctx, bank, monkeypatch):
        from edison_amd.context import Context
        fs, lo, hi, force = ms.FILTERBANKS[bank]
        self.own = bank != "shipped"
        if not self.own:
            self.c = ctx
            return
        if force:
            monkeypatch.setenv("EDISON_FORCE_WIDE_MEL", "1")
        self.c = Context(ctx.device)
        if not force:
            self.c.configure_mfcc(fs, lo, hi)

    def __enter__(self):
        self.c.use_torch_stream()
        return self.c

    def __exit__(self, *a):
        if self.own:
            self.c.close()
        else:
            self.c.use_own_stream()


@pytest.mark.parametrize("name", list(ms.ROWS))
def test_row(ctx, built_lib, oracle_mod, monkeypatch, name):
    row = ms.ROWS[name]
    d = Dev(ctx)
    torch = d.torch
    shape = ms.bank_shape(built_lib, row["bank"], row["variant"])
    n_cu = ctx.device_info()["n_cu"]
    u = ms.unit(row)
    with _Ctx(ctx, row["bank"], monkeypatch) as c:
        # ---- 1. the base launch(es) against the oracle
        if row["n_utt_one"]:
            base_runs = [launch(d, c, row, ms.UTT_FRAMES, shape, shift=s) for s in (0, 31, 33)]     # 31 frames a launch: three cover the 64
        else:
            base_runs = [launch(d, c, row, max(-(-ms.N_BASE // u) * u, 2 * u), shape)]
        ref, ok = _oracle(oracle_mod, row, d.base_np)
        nc = row["n_coef"]
        Rf = Rq = None
        if base_runs[0][0] is not None:
            Rf = _gather_base(d, [(f, i) for f, _, i in base_runs])
            got = Rf.cpu().numpy().astype(np.float64)
            atol, rtol = TOL["A" if row["log"] else row["variant"]]
            ratio = np.abs(got - ref[:, :nc])[ok] / (atol + rtol * np.abs(ref[:, :nc][ok]))
            key = row["variant"] + ("+log" if row["log"] else "")
            RATIO[key] = max(RATIO.get(key, 0.0), float(ratio.max()))
            print("%s: largest |d| / (atol + rtol |ref|) = %.4f (%s, %d of 64 frames held)" % (name, ratio.max(), key, ok.sum()))
            assert ratio.max() <= 1.0, (name, float(ratio.max()), np.argwhere(ratio > 1.0)[:4].tolist())
        if base_runs[0][1] is not None:
            Rq = _gather_base(d, [(q, i) for _, q, i in base_runs])
            if ms.is_kws(row):
                want = oracle_mod.net_input(ref[:, :13])
                bad = np.argwhere(Rq.cpu().numpy() != want)
                assert not bad.size, (name, "exact-mode features differ from oracle.net_input(oracle.mfcc())", bad[:4].tolist())
            elif Rf is not None:
                for f, q, _ in base_runs:
                    assert torch.equal(q, _quantised(d, f, row["feat_scale"])), (name, "int8 is not the rounded float32 of the same launch")
            else:
                f, q, _ = launch(d, c, row, base_runs[0][2].numel(), shape, outs="fq")      # int8 only: the same call with both outputs
                assert torch.equal(q, base_runs[0][1]) and torch.equal(q, _quantised(d, f, row["feat_scale"])), name
                got = _gather_base(d, [(f, base_runs[0][2])]).cpu().numpy().astype(np.float64)
                atol, rtol = TOL["A" if row["log"] else row["variant"]]
                ratio = np.abs(got - ref[:, :nc])[ok] / (atol + rtol * np.abs(ref[:, :nc][ok]))
                print("%s: largest |d| / (atol + rtol |ref|) = %.4f" % (name, ratio.max()))
                assert ratio.max() <= 1.0, (name, float(ratio.max()))
        # ---- 2. + 3. position independence at every count (the guard rows are checked inside launch)
        for n in ms.row_counts(row, n_cu):
            f, q, idx = launch(d, c, row, n, shape, shift=7 if row["n_utt_one"] else 0)
            if Rf is not None:
                assert f is not None
                bad = (f != Rf[idx]).any(dim=1).nonzero()
                assert bad.numel() == 0, (name, n, "float32 rows depend on the frame's position", bad[:6, 0].tolist())
            if Rq is not None:
                bad = (q != Rq[idx]).any(dim=1).nonzero()
                assert bad.numel() == 0, (name, n, "int8 rows depend on the frame's position", bad[:6, 0].tolist())
                if f is not None:
                    assert torch.equal(q, _quantised(d, f, row["feat_scale"])), (name, n)
            del f, q, idx


@pytest.mark.parametrize("variant,log", [("A", False), ("B", False), ("B", True), ("TF", False)])
def test_addressing_does_not_change_a_bit(ctx, built_lib, monkeypatch, variant, log):
    """A frame's float32 coefficients do not depend on how it was addressed: every form of mfcc_sweep.FORMS (aligned or not, one batch,
    rows, a list of batches) on the same 66 frame slots, per bank, bit for bit against the flat aligned call. The 2+5 and the forced
    3+6 table of the shipped bank are two summation texts of the same products: held to 2e-6 x max |one|, the bar of
    test_two_frame_kernel_agrees_with_one_frame_kernel."""
    d = Dev(ctx)
    torch = d.torch
    flat = {}
    for bank in ms.FILTERBANKS:
        shape = ms.bank_shape(built_lib, bank, variant)
        with _Ctx(ctx, bank, monkeypatch) as c:
            monkeypatch.delenv("EDISON_FORCE_WIDE_MEL", raising=False)
            for form in ms.FORMS:
                row = ms.form_row(form, variant, log, bank)
                if variant == "TF" and row["entry"] == "mfcc_batches_t":
                    continue
                f, _, idx = launch(d, c, row, 66, shape)
                got = _gather_base(d, [(f, idx)])
                if form == "flat":
                    flat[bank] = got
                else:
                    bad = (got != flat[bank]).any(dim=1).nonzero()
                    assert bad.numel() == 0, (variant, log, bank, form, "differs from the flat aligned call", bad[:6, 0].tolist(),
                                              float((got - flat[bank]).abs().max()))
    a, b = flat["shipped"], flat["shipped_forced"]
    diff = float((a - b).abs().max())
    print("%s%s: 2+5 against the forced 3+6 table, max |d| = %.3e, max |one| = %.3e" % (variant, "+log" if log else "", diff, float(a.abs().max())))
    assert diff <= 2e-6 * float(a.abs().max())
    assert float((flat["wide6"] - a).abs().max()) > 1e-3 and float((flat["narrow3"] - a).abs().max()) > 1e-3      # the banks are different banks


def test_frame_step_zero_gives_equal_rows(ctx):
    """frame_step = 0: every frame is the first one (of the batch, of its row, of its batch in a list)"""
    from edison_amd import _lib
    d = Dev(ctx)
    torch = d.torch
    n_cu = ctx.device_info()["n_cu"]
    n = 2 * ms.ed2_wpb() * n_cu + 3
    n -= n % 3
    ctx.use_torch_stream()
    try:
        for variant in (_lib.MFCC_A, _lib.MFCC_B, _lib.MFCC_TF):
            one = torch.empty((3, 32), dtype=torch.float32, device=d.dev)
            ctx.mfcc_t(d.base[5:8].reshape(-1), 3, 1024, variant, 32, out=one)
            buf, out = d.guarded(n, 32, torch.float32)
            ctx.mfcc_t(d.base[5].clone(), n, 0, variant, 32, out=out)
            torch.cuda.synchronize()
            assert torch.equal(out, one[:1].expand(n, 32)) and d.guards_intact(buf, n)
            buf, out = d.guarded(n, 32, torch.float32)
            ctx.mfcc_rows_t(d.base[5:8].reshape(-1), 3, 1024, n // 3, 0, variant, 32, out=out)       # three rows of n / 3 frames, all the row's first
            torch.cuda.synchronize()
            assert torch.equal(out.reshape(3, n // 3, 32), one[:, None, :].expand(3, n // 3, 32)) and d.guards_intact(buf, n)
            if variant != _lib.MFCC_TF:
                outs = [d.guarded(n // 3, 32, torch.float32) for _ in range(3)]
                ctx.mfcc_batches_t([d.base[5 + b].clone() for b in range(3)], n // 3, 0, variant, 32, outs=[v for _, v in outs])
                torch.cuda.synchronize()
                for b, (g, v) in enumerate(outs):
                    assert torch.equal(v, one[b:b + 1].expand(n // 3, 32)) and d.guards_intact(g, n // 3)
    finally:
        ctx.use_own_stream()


def test_zz_report_the_error_ratios():
    """Not a check of its own: the largest |d| / (atol + rtol |ref|) per variant that the rows above saw (DESIGN.md section 4.1 quotes
    them; the bars are about a hundred times the error)"""
    print("largest |d| / (atol + rtol |ref|) per variant:", {k: round(v, 4) for k, v in sorted(RATIO.items())})
    assert all(v <= 1.0 for v in RATIO.values())

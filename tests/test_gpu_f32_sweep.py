"""MFCC variant D (the firmware's float32 mfcc_create / mfcc_compute) on the GPU over both its kernels and every work split: the rows
of tests/f32_sweep.py at every frame count of f32_sweep.counts, which tests/test_f32_sweep_cpu.py proves to reach every case.

Per row and count, through the host entry point (compute) and the device entry point (compute_t on the context's stream):
  * band energies (linear domain, relative to the frame's largest bin), log-mel energies on clear bands and the pre-rounding floats on
    frames of clear bands within f32_sweep.BARS of the float64 reference -- bars measured on the two CPU references, not on the GPU;
  * int8 = round_half_away(clip(reference64)) outside the boundary band, never more than one apart on the held frames, and the band
    holds at most 10 % of the held values;
  * on EVERY frame, whatever its conditioning: the pre-rounding float is the float64 DCT of the call's own log-mel energies x 2^dec_bits
    within BARS["dct"], and int8 is that float rounded half away from zero and saturated, bit for bit;
  * both entry points give the same bits; NULL for the optional outputs does not change `out`; sentinel rows around all three outputs
    stay untouched (odd counts: the duplicate B half of the last pair writes nothing);
  * hop >= frame_len (and hop 0): every frame's int8, floats and log-mel are the bits of its base frame from a 64-frame call, at any
    position, in either half of a pair, at any count.
Then: silence next to a full-scale rail, mfcc_compute under the firmware's name, the generic kernel at padded 512 in a child process
with EDISON_F32_GENERIC=1 against the fast kernel, and the NNoM example's stream front end over its window sizes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import f32_sweep as fs

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3
FAST_ROWS = [n for n, r in fs.ROWS.items() if fs.kernel(r) == "fast"]
CHILD = {"failed": None, "data": None}


def _mfcc(ctx, row):
    from edison_amd.mfcc.mfcc_f32 import MfccF32
    return MfccF32(ctx=ctx, **fs.create_args(row))


def _first_bad(bad):
    f, c = np.argwhere(bad)[0]
    return int(f), int(c)


def check_accuracy(name, n, row, x, idx, i8, f32, lm, tag="fast/generic as dispatched"):
    """The accuracy section of the module docstring for one call; returns the share of the held values inside the boundary band"""
    ref = fs.reference64(row, x, n, row["hop"])
    C, LM, SM = ref
    lin, dlog, dco, held = fs.errors(row, ref, lm, f32)
    print("%s n=%d (%s): lin %.3g log %.3g coef %.3g dct %.3g of bars %.3g %.3g %.3g %.3g; %d frames held" % (
        name, n, tag, lin.max(), dlog.max(), dco.max(), fs.dct_stage(row, lm, f32).max(), fs.BARS["lin"], fs.BARS["log"], fs.BARS["coef"], fs.BARS["dct"], held.sum()))
    for what, err, got, want in (("band energy / largest bin", lin, np.exp(lm.astype(np.float64)), np.exp(LM)), ("log-mel", dlog, lm, LM)):
        bar = fs.BARS["lin" if what != "log-mel" else "log"]
        if (err > bar).any():
            f, b = _first_bad(err > bar)
            raise AssertionError("%s n=%d: %s of frame %d (base %d) band %d: got %.9g want %.9g, error %.3g > %.3g" % (
                name, n, what, f, idx[f], b, got[f, b], want[f, b], err[f, b], bar))
    if (dco > fs.BARS["coef"]).any():
        f, c = _first_bad(dco > fs.BARS["coef"])
        raise AssertionError("%s n=%d: pre-rounding float of frame %d (base %d) coefficient %d: got %.9g want %.9g, error / 2^dec_bits %.3g > %.3g" % (
            name, n, f, idx[f], c, f32[f, c], C[f, c], dco[f, c], fs.BARS["coef"]))
    # the last stage on EVERY frame, rails, square wave and silence included: the pre-rounding float is the float64 DCT of the same
    # call's log-mel energies within the DCT bar, and int8 is that float rounded half away and saturated, bit for bit
    dd = fs.dct_stage(row, lm, f32)
    if (dd > fs.BARS["dct"]).any():
        f, c = _first_bad(dd > fs.BARS["dct"])
        raise AssertionError("%s n=%d: DCT stage of frame %d (base %d) coefficient %d: float %.9g, float64 DCT of its log-mel %.9g, error / 2^dec_bits %.3g > %.3g" % (
            name, n, f, idx[f], c, f32[f, c], (lm[f].astype(np.float64) @ fs.tables(row)[2][c]) * float(1 << row["dec_bits"]), dd[f, c], fs.BARS["dct"]))
    own = fs.round_half_away(f32.astype(np.float64))
    if (own != i8).any():
        f, c = _first_bad(own != i8)
        raise AssertionError("%s n=%d: int8 of frame %d (base %d) coefficient %d is %d, its own pre-rounding float %.9g rounds to %d" % (
            name, n, f, idx[f], c, i8[f, c], f32[f, c], own[f, c]))
    want, near = fs.round_half_away(C), fs.boundary_band(row, C)
    d = np.abs(want.astype(int) - i8.astype(int)) * held[:, None]
    if (d * ~near).any() or d.max() > 1:
        f, c = _first_bad((d * ~near > 0) | (d > 1))
        raise AssertionError("%s n=%d: int8 of frame %d (base %d) coefficient %d: got %d want %d (reference %.6f, float %.6f)" % (
            name, n, f, idx[f], c, i8[f, c], want[f, c], C[f, c], f32[f, c]))
    share = float(near[held].mean()) if held.any() else 0.0
    assert share <= fs.INT8_CAP, (name, n, "share of the held values inside the boundary band", share)
    return share


def device_call(ctx, m, x, n, hop, outs=True):
    """compute_t with sentinel rows around out, out_f32 and logmel inside one allocation each: (int8, float32, log-mel) as numpy"""
    import torch
    dev = torch.device("cuda", ctx.device)
    a = torch.from_numpy(x).to(dev)
    G = GUARD_ROWS
    bo = torch.full((n + 2 * G, m.n_out), 99, dtype=torch.int8, device=dev)
    bf = torch.full((n + 2 * G, m.n_out), 4321.0, dtype=torch.float32, device=dev)
    bl = torch.full((n + 2 * G, fs.N_FBANK), 4321.0, dtype=torch.float32, device=dev)
    ctx.use_torch_stream()
    try:
        m.compute_t(a, n, hop, bo[G:G + n], bf[G:G + n] if outs else None, bl[G:G + n] if outs else None)
        torch.cuda.synchronize()
    finally:
        ctx.use_own_stream()
    for what, b, g in (("out", bo, 99), ("out_f32", bf, 4321.0), ("logmel", bl, 4321.0)):
        assert bool((b[:G] == g).all()) and bool((b[G + n:] == g).all()), (what, n, "a sentinel row changed")
    if not outs:
        assert bool((bf == 4321.0).all()) and bool((bl == 4321.0).all())
    return bo[G:G + n].cpu().numpy(), bf[G:G + n].cpu().numpy(), bl[G:G + n].cpu().numpy()


def _bits_equal(name, n, what, got, want, idx):
    same = got.view(np.uint8 if got.dtype == np.int8 else np.uint32) == want.view(np.uint8 if want.dtype == np.int8 else np.uint32)
    if not same.all():
        f, c = _first_bad(~same)
        raise AssertionError("%s n=%d: %s of frame %d (base %d) value %d: got %r want %r" % (name, n, what, f, idx[f], c, got[f, c], want[f, c]))


@pytest.mark.parametrize("name", list(fs.ROWS))
def test_row(ctx, oracle_mod, name):
    row = fs.ROWS[name]
    N, hop = row["frame_len"], row["hop"]
    n_cu = ctx.device_info()["n_cu"]
    assert n_cu <= fs.MEASURE_N_CU, "the bars were measured on the streams of a device of at most %d CUs: raise f32_sweep.MEASURE_N_CU and re-measure" % fs.MEASURE_N_CU
    m = _mfcc(ctx, row)
    base, where = fs.base_frames(row)
    whole = hop >= N or hop == 0
    if whole:                                                          # the 64 base frames alone, one call: what every later frame must equal
        B = m.compute(base.reshape(-1), n_frames=fs.N_BASE, frame_step=N, want_float=True)
    shares = []
    counts = fs.counts(row, n_cu)
    print("%s: %s kernel, counts %s" % (name, fs.kernel(row), counts))
    for n in counts:
        assert fs.cases(row, n, n_cu), (name, n)
        x, idx = fs.audio(row, n, base)
        i8, f32, lm = m.compute(x, n_frames=n, frame_step=hop, want_float=True)
        shares.append(check_accuracy(name, n, row, x, idx, i8, f32, lm))
        d8, df, dl = device_call(ctx, m, x, n, hop)
        for what, a, b in (("int8", d8, i8), ("float", df, f32), ("log-mel", dl, lm)):
            _bits_equal(name + " device against host entry point", n, what, a, b, idx)
        if n % 2 or n == counts[-1]:
            _bits_equal(name + " out alone (NULL out_f32 / logmel), host", n, "int8", m.compute(x, n_frames=n, frame_step=hop), i8, idx)
            _bits_equal(name + " out alone (NULL out_f32 / logmel), device", n, "int8", device_call(ctx, m, x, n, hop, outs=False)[0], i8, idx)
        if whole:
            for what, a, b in (("int8", i8, B[0]), ("float", f32, B[1]), ("log-mel", lm, B[2])):
                _bits_equal(name + " against its base frame", n, what, a, b[idx], idx)
    print("%s: largest share of the held int8 values inside the boundary band %.2f %%" % (name, 100 * max(shares)))
    m.close()


@pytest.mark.parametrize("name", FAST_ROWS)
def test_guard_rows_at_odd_counts(ctx, name):
    """The device entry point alone, every output inside sentinel rows (device_call asserts them): for an odd count the fast kernel
    runs a duplicate B half on the last frame, which must write nothing past row n - 1 of out, out_f32 or logmel."""
    row = fs.ROWS[name]
    m = _mfcc(ctx, row)
    base, _ = fs.base_frames(row)
    for n in [c for c in fs.counts(row, ctx.device_info()["n_cu"]) if c % 2]:
        x, _ = fs.audio(row, n, base)
        device_call(ctx, m, x, n, row["hop"])
        device_call(ctx, m, x, n, row["hop"], outs=False)
    m.close()


@pytest.mark.parametrize("name", ["firmware_whole", "f400_over", "g1024_sat", "g128"])
def test_silence_next_to_a_rail_stays_silent(ctx, name):
    """A zero frame beside the full-scale rail gives the bits of an all-zero batch, in either half of a pair (fast kernel) or in a
    neighbouring wave (generic); all 26 log-mels are logf(FLT_MIN); the rail's bits are those it gives beside itself."""
    row = dict(fs.ROWS[name], hop=fs.ROWS[name]["frame_len"])
    N = row["frame_len"]
    m = _mfcc(ctx, row)
    zero, rail = np.zeros(N, np.int16), np.full(N, 32767, np.int16)
    Z = m.compute(np.concatenate([zero, zero]), n_frames=2, frame_step=N, want_float=True)
    R = m.compute(np.concatenate([rail, rail]), n_frames=2, frame_step=N, want_float=True)
    want_lm = np.float32(np.log(np.float64(fs.FLT_MIN)))
    ulp = np.abs(Z[2].view(np.int32).astype(np.int64) - want_lm.view(np.int32))
    print("%s: log-mel of silence %r, logf(FLT_MIN) correctly rounded %r" % (name, Z[2][0, 0], want_lm))
    assert len(set(Z[2].view(np.uint32).ravel().tolist())) == 1 and ulp.max() <= 1, (Z[2][0, 0], want_lm)       # logf: 1 ulp (ocml)
    for what, a in zip(("int8", "float", "log-mel"), R):
        _bits_equal(name + " rail beside itself: both frames", 2, what, a[:1], a[1:], [0])
    for order in ((zero, rail), (rail, zero), (rail, zero, rail), (zero, rail, zero), (zero, rail, rail, zero, zero)):
        got = m.compute(np.concatenate(order), n_frames=len(order), frame_step=N, want_float=True)
        for f, fr in enumerate(order):
            for what, a, z, r in zip(("int8", "float", "log-mel"), got, Z, R):
                _bits_equal("%s %s beside the other, %d frames" % (name, "silence" if fr is zero else "rail", len(order)), len(order), what,
                            a[f:f + 1], (z if fr is zero else r)[:1], [f] * (f + 1))
    m.close()


@pytest.mark.parametrize("name", ["firmware_whole", "f400_over", "g256"])
def test_mfcc_compute_is_the_batch_call_of_one_frame(built_lib, ctx, name):
    """mfcc_create / mfcc_compute / mfcc_delete, the firmware's names on the process-global context: the bits of the batch call, n = 1"""
    row = fs.ROWS[name]
    L = built_lib
    L.mfcc_create.restype = ctypes.c_void_p
    L.mfcc_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float]
    L.mfcc_compute.restype = None
    L.mfcc_compute.argtypes = [ctypes.c_void_p] * 3
    L.mfcc_delete.restype = None
    L.mfcc_delete.argtypes = [ctypes.c_void_p]
    h = L.mfcc_create(row["n_features"], row["offset"], row["frame_len"], row["dec_bits"], row["preemph"])
    assert h
    m = _mfcc(ctx, row)
    base, _ = fs.base_frames(row)
    B = m.compute(base.reshape(-1), n_frames=fs.N_BASE, frame_step=row["frame_len"])
    for f in range(fs.N_BASE):
        fr = np.ascontiguousarray(base[f])
        out = np.full(m.n_out, 99, np.int8)
        L.mfcc_compute(h, fr.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
        one = m.compute(fr, n_frames=1)
        _bits_equal(name + " mfcc_compute against the batch call with n = 1", 1, "int8", out[None], one, [f])
        _bits_equal(name + " n = 1 against the 64-frame call", 1, "int8", one, B[f:f + 1], [f])
    L.mfcc_delete(h)
    m.close()


# ---- the generic kernel at padded 512: EDISON_F32_GENERIC=1 is read once per process, so a fresh one -------------------------------------


def _child(tmp_path_factory):
    """One child process for all padded-512 rows; a failure is remembered and nothing that depends on it starts further GPU work"""
    if CHILD["failed"]:
        pytest.fail("the EDISON_F32_GENERIC=1 child process failed before: " + CHILD["failed"])
    if CHILD["data"] is None:
        out = str(tmp_path_factory.mktemp("f32_generic") / "generic.npz")
        env = dict(os.environ, EDISON_F32_GENERIC="1")
        try:
            r = subprocess.run([sys.executable, os.path.join(fs.ROOT, "tests", "f32_sweep.py"), out, ",".join(FAST_ROWS)], env=env, timeout=600,
                               capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            CHILD["failed"] = "timed out"
            pytest.fail("the EDISON_F32_GENERIC=1 child process timed out")
        if r.returncode != 0:
            CHILD["failed"] = "exit status %d" % r.returncode
            pytest.fail("the EDISON_F32_GENERIC=1 child process: exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
        CHILD["data"] = dict(np.load(out))
    return CHILD["data"]


@pytest.mark.parametrize("name", FAST_ROWS)
def test_generic_kernel_at_padded_512(ctx, oracle_mod, tmp_path_factory, name):
    """The fast kernel's A/B partner on the same rows: inside the same bars, int8 never more than one from the fast kernel's on the held frames"""
    data = _child(tmp_path_factory)
    row = fs.ROWS[name]
    n_cu = ctx.device_info()["n_cu"]
    assert int(data["n_cu"]) == n_cu
    m = _mfcc(ctx, row)
    base, _ = fs.base_frames(row)
    differ = 0
    for n in fs.counts(row, n_cu, generic_env=True):
        assert fs.cases(row, n, n_cu, generic_env=True)
        x, idx = fs.audio(row, n, base)
        i8, f32, lm = (data["%s/%d/%s" % (name, n, k)] for k in ("i8", "f32", "lm"))
        check_accuracy(name, n, row, x, idx, i8, f32, lm, tag="generic kernel, child process")
        fast = m.compute(x, n_frames=n, frame_step=row["hop"])
        # on the frames held to the int8 bar: where a band holds nothing but the transform's rounding noise (the square wave, the rails)
        # two correct float32 transforms give unrelated int8 -- the two CPU references are 70 apart there (tests/test_f32_sweep_cpu.py)
        _, LM, SM = fs.reference64(row, x, n, row["hop"])
        d = np.abs(fast.astype(int) - i8.astype(int)) * fs.clear_bands(LM, SM).all(axis=1)[:, None]
        assert d.max() <= 1, (name, n, "fast and generic int8 more than one apart: frame, coefficient", _first_bad(d > 1))
        differ += int((f32 != m.compute(x, n_frames=n, frame_step=row["hop"], want_float=True)[1]).sum())
    print("%s: %d floats differ in bits between the two kernels" % (name, differ))
    if name == "firmware":
        assert differ > 0, "the child did not run the other kernel: EDISON_F32_GENERIC was not honoured"
    m.close()


# ---- the stream front end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_events", [1, 16])
@pytest.mark.parametrize("feat", [(1, 0), (13, 1), (26, 0)])
@pytest.mark.parametrize("rows", [2, 63, 64, 1024])
def test_stream_front_end(ctx, rows, feat, max_events):
    """edison_f32_stream_* at the ends of the window sizes it accepts and at 1, 12 and 26 outputs, against the host replay of the ring
    that test_nnom_example_front_end uses (app.c:545-623), features from the batch path: bit for bit, for pushes of one event, of
    exactly max_events and of many, and again after a reset in mid-stream."""
    from edison_amd.mfcc.mfcc_f32 import MfccF32, NnomKwsFrontEnd
    n_out = feat[0] - feat[1]
    n_ev = rows // 2 + 40                                                # the ring wraps
    rng = np.random.default_rng(1000 * rows + 10 * n_out + max_events)
    x = np.clip(rng.normal(0, 3000, n_ev * 512), -32768, 32767).astype(np.int16)
    m = MfccF32(ctx=ctx, num_mfcc_features=feat[0], feature_offset=feat[1])
    assert m.n_out == n_out

    def replay(x, n_ev):
        # 256 old samples (zeros at the start) + 512 new per event, two frames at offsets 0 and 256: the stream at hop 256
        f = m.compute(np.concatenate([np.zeros(256, np.int16), x[:n_ev * 512]]), n_frames=2 * n_ev, frame_step=256)
        ring, idx, want = np.zeros((rows, n_out), np.int8), 0, []
        for e in range(n_ev):
            for i in range(2):
                ring[idx] = f[2 * e + i]
                idx = (idx + 1) % rows
            want.append(np.concatenate([ring[idx:], ring[:idx]]))
        return np.stack(want)
    want = replay(x, n_ev)
    fe = NnomKwsFrontEnd(ctx=ctx, window_rows=rows, max_events=max_events, num_mfcc_features=feat[0], feature_offset=feat[1])
    k = 1 + max_events
    got = np.concatenate([fe.push(x[:512]), fe.push(x[512:512 * k]), fe.push(x[512 * k:])])        # 1 event, exactly max_events, many
    assert fe.events_seen == n_ev and got.shape == (n_ev, rows, n_out)
    bad = np.argwhere(got != want)
    assert not bad.size, (rows, n_out, max_events, "event, row, feature", bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))
    fe.reset()
    assert fe.events_seen == 0
    y = x[512 * 7:]
    assert np.array_equal(fe.push(y[:512 * 5]), replay(y, 5)), (rows, n_out, max_events, "after a reset in mid-stream")
    fe.close(); m.close()

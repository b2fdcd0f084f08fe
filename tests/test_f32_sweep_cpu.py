"""The sweep of MFCC variant D without a GPU (tests/f32_sweep.py): the rows cover the table of DESIGN.md section 4.6a, every note names
the kernel the restated dispatch gives its row, counts() reaches every case of both work splits, the restated constants are the
source's, reference64 agrees with the reference-made fixture and with both references, and BARS are what the two references measure:
their largest errors against reference64 over the frames the sweep runs, times the margin, rounded up to one significant digit. The
checks that need the reference's compiled mfcc_compute (oracle/_ref/libmfcc_f32_ref.so) skip where it is not built."""
import ctypes
import os

import numpy as np
import pytest

import f32_sweep as fs

N_CUS = (8, 256, 304)


@pytest.fixture(scope="module")
def f32ref(oracle_mod):
    if not os.path.exists(oracle_mod.F32_REF_SO):
        pytest.skip("oracle/_ref/libmfcc_f32_ref.so is not built here (it is compiled from the reference tree)")
    return oracle_mod.mfcc_f32_ref()


def test_the_rows_cover_the_table():
    have = set().union(*(fs.row_items(r) for r in fs.ROWS.values()))
    assert sorted(fs.full_items() - have, key=str) == [], "values of the table no row has"
    # the configuration the firmware runs is there, at its own hop
    assert fs.create_args(fs.ROWS["firmware"]) == dict(num_mfcc_features=13, feature_offset=1, frame_len=512, mfcc_dec_bits=8, preemph=0.97)
    assert fs.ROWS["firmware"]["hop"] == 256


@pytest.mark.parametrize("name", list(fs.ROWS))
def test_note_names_the_kernel(name):
    row = fs.ROWS[name]
    assert fs.note_kernel(row["note"]) == (fs.kernel(row), fs.padded(row["frame_len"])), name
    assert fs.kernel(row, generic_env=True) == "generic"
    assert (fs.kernel(row) == "fast") == (257 <= row["frame_len"] <= 512)


def test_restated_constants_are_the_source_ones():
    text = open(os.path.join(fs.CSRC, "mfcc_f32_kernels.hip")).read()
    assert fs.ef_wpb() == 4 and fs.ef2_wpb() == 16
    for line in ("int64_t blocks = (args->n_frames + EF_WPB - 1) / EF_WPB;", "const size_t lds = (size_t)EF_WPB * (size_t)padded * sizeof(float2);",
                 "int per_cu = (int)((160u * 1024u) / (lds + 12u * 1024u));", "if (per_cu > 8) per_cu = 8;", "const int64_t cap = (int64_t)n_cu * per_cu;",
                 "const int64_t n_pairs = (args->n_frames + 1) / 2;", "int64_t blocks = (n_pairs + EF2_WPB - 1) / EF2_WPB;", "if (blocks > n_cu) blocks = n_cu;",
                 "const uint32_t s0 = (uint32_t)(((uint64_t)blockIdx.x * n_pairs) / gridDim.x);",
                 "const uint32_t cnt = (uint32_t)(((uint64_t)(blockIdx.x + 1) * n_pairs) / gridDim.x) - s0;",
                 "if (threadIdx.x == 0) *queue = 2 * EF2_WPB;", "uint32_t i_cur = wave, i_next = wave + EF2_WPB;"):
        assert line in text, "the launch code changed, restate it in tests/f32_sweep.py: " + line
    assert "mfcc->padded == 512 && ctx->d_tab[0] && !generic" in open(os.path.join(fs.CSRC, "edison_f32.hip")).read()
    assert [fs.generic_per_cu(p) for p in (128, 256, 512, 1024)] == [8, 8, 5, 3]


@pytest.mark.parametrize("n_cu", N_CUS)
def test_counts_reach_every_split_case(n_cu):
    for name, row in fs.ROWS.items():
        for env in (False, True):
            want = fs.FAST_CASES if fs.kernel(row, env) == "fast" else fs.GENERIC_CASES
            cs = fs.counts(row, n_cu, env)
            have = set().union(*(fs.cases(row, n, n_cu, env) for n in cs))
            assert sorted(set(want) - have) == [], (name, n_cu, env, "split cases no count reaches")
            assert any(n % 2 for n in cs)
    w = fs.ef2_wpb()
    fast = fs.counts(fs.ROWS["firmware"], n_cu)
    for n in (1, 2, 3, 2 * w - 1, 2 * w, 2 * w + 1, 2 * w * n_cu - 1, 2 * w * n_cu, 2 * w * n_cu + 1):
        assert n in fast
    # the split is a partition of the pairs, whatever the count
    for n in fast + [4 * w * n_cu + 5]:
        s = fs.fast_split(n, n_cu)
        assert s[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(s, s[1:])) and s[-1][0] + s[-1][1] == (n + 1) // 2 and len(s) <= n_cu
    cap = fs.generic_cap(1024, n_cu)
    assert fs.counts(fs.ROWS["g1024_sat"], n_cu) == sorted({1, 3, 4, 5, 4 * cap - 1, 4 * cap + 1, 8 * cap + 3})


def test_inputs():
    for name, row in fs.ROWS.items():
        base, where = fs.base_frames(row)
        assert base.shape == (64, row["frame_len"]) and base.dtype == np.int16
        assert len({b.tobytes() for b in base}) == 64, "the base frames are distinct"
        assert not base[where["zero"]].any() and (base[where["rail_pos"]] == 32767).all() and (base[where["rail_neg"]] == -32768).all()
        sq = base[where["square"]].astype(int)
        assert set(sq) == {32767, -32768} and (sq[1:] != sq[:-1]).all()
        assert np.count_nonzero(base[where["impulse"]]) == 1
        rms = np.sqrt((base.astype(float) ** 2).mean(axis=1))
        assert rms[rms > 0].min() < 1.0 and (base == 32767).any(axis=1).sum() > 3      # five decades, up to clipping
        idx = fs.tile_index(64 * 64 + 5)
        assert np.array_equal(idx[:64], np.arange(64)) and idx[64] == 1
        assert set(idx[0:4096:2]) == set(idx[1:4096:2]) == set(range(64)), "every base frame rides in both halves of a pair"
        for n in (1, 5, 131):
            x, ix = fs.audio(row, n, base)
            hop, N = row["hop"], row["frame_len"]
            assert x.size == ((n - 1) * hop + N if hop else N)
            if hop >= N:
                assert all(np.array_equal(x[i * hop:i * hop + N], base[ix[i]]) for i in range(n))


def _struct_tables(built_lib, row):
    _F32Tables = fs.F32Tables
    built_lib.ed_build_f32_tables.restype = ctypes.c_int
    built_lib.ed_build_f32_tables.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.POINTER(_F32Tables),
                                              ctypes.c_char_p, ctypes.c_size_t]
    t = _F32Tables()
    err = ctypes.create_string_buffer(200)
    assert built_lib.ed_build_f32_tables(row["n_features"], row["offset"], row["frame_len"], row["dec_bits"], row["preemph"], ctypes.byref(t), err, 200) == 0, err.value
    return t


@pytest.mark.parametrize("name", list(fs.ROWS))
def test_reference64_tables_are_the_products(built_lib, oracle_mod, name):
    """reference64 reads the oracle's tables; they are the float32 values ed_build_f32_tables hands the kernels, bit for bit"""
    row = fs.ROWS[name]
    t = _struct_tables(built_lib, row)
    win, W, D = fs.tables(row)
    N, P = row["frame_len"], fs.padded(row["frame_len"])
    assert t.padded == P and t.scale == float(1 << row["dec_bits"]) and t.preempha == np.float32(row["preemph"])
    assert np.array_equal(np.array(t.window, np.float32)[:N].astype(np.float64), win)
    first, last, off, w = np.array(t.mel_first), np.array(t.mel_last), np.array(t.mel_off), np.array(t.mel_w, np.float32)
    for b in range(26):
        want = np.zeros(P // 2 + 1)
        if first[b] >= 0:
            want[first[b]:last[b] + 1] = w[off[b]:off[b] + last[b] - first[b] + 1]
        assert np.array_equal(W[b], want), (name, b)
    assert W[:, P // 2].max() == 0 and last.max() < P // 4 + 1, "no band reaches past 4000 Hz, let alone the Nyquist bin"
    assert np.array_equal(np.array(t.dct, np.float32)[row["offset"] * 26:row["n_features"] * 26].astype(np.float64), D.ravel())


@pytest.mark.parametrize("i", [0, 1, 2])
def test_reference64_against_the_reference_made_fixture(oracle_mod, i):
    """tests/golden/mfccf32_golden.npz: what the reference's own mfcc_compute + CMSIS float transform answered. Log-mel and band
    energies within BARS; int8 equal outside the boundary band on frames of clear bands, never more than one apart there."""
    g = np.load(os.path.join(fs.ROOT, "tests", "golden", "mfccf32_golden.npz"))
    nf, off, flen, bits, pre, hop = g["cfg%d" % i]
    row = dict(name="fixture%d" % i, n_features=int(nf), offset=int(off), frame_len=int(flen), dec_bits=int(bits), preemph=float(pre), hop=int(hop))
    ri, rlm = g["mfcc%d" % i], g["logmel%d" % i]
    ref = fs.reference64(row, g["audio"], ri.shape[0], int(hop))
    lin, dlog, _, held = fs.errors(row, ref, rlm)
    print("fixture %d: lin %.3g log %.3g, %d of %d frames held" % (i, lin.max(), dlog.max(), held.sum(), held.size))
    assert lin.max() <= fs.BARS["lin"] and dlog.max() <= fs.BARS["log"], (lin.max(), dlog.max())
    assert held.mean() > 0.5
    want, near = fs.round_half_away(ref[0]), fs.boundary_band(row, ref[0])
    d = np.abs(want.astype(int) - ri.astype(int))
    assert d[held].max() <= 1
    assert not d[held][~near[held]].any(), np.argwhere(d * held[:, None] * ~near)[:4].tolist()
    assert near[held].mean() <= fs.INT8_CAP


def _measure_all(outputs):
    worst, shares, res = dict(lin=0.0, log=0.0, coef=0.0, dct=0.0), {}, {}
    for name, row in fs.ROWS.items():
        (lin, lg, co, dd), i8, ref, held = fs.measure(row, outputs)
        res[name] = (lin, lg, co, dd)
        for k, v in zip(("lin", "log", "coef", "dct"), (lin, lg, co, dd)):
            worst[k] = max(worst[k], v)
        want, near = fs.round_half_away(ref[0]), fs.boundary_band(row, ref[0])
        d = np.abs(want.astype(int) - i8.astype(int))
        assert held.sum() >= 48, (name, "too few base frames with every band clear", int(held.sum()))
        assert not d[held][~near[held]].any(), (name, "a reference's int8 differs outside the boundary band", np.argwhere(d * held[:, None] * ~near)[:4].tolist())
        assert d[held].max() <= 1, (name, int(d[held].max()))
        shares[name] = float(near[held].mean())
    return worst, shares, res


@pytest.fixture(scope="module")
def measured(oracle_mod):
    """{"ora": ..., "ref": ... or None}: (largest lin / log / coef, boundary share per row, figures per row) of each reference"""
    out = {"ora": _measure_all(fs.oracle_outputs), "ref": None}
    if os.path.exists(oracle_mod.F32_REF_SO):
        out["ref"] = _measure_all(fs.ref_outputs)
    for tag, m in out.items():
        if m:
            print(tag, {k: "%.3g" % v for k, v in m[0].items()}, {k: "%.1f %%" % (100 * v) for k, v in m[1].items()})
    return out


def test_both_references_pass_the_bars_with_the_margin_to_spare(measured):
    for tag, m in measured.items():
        if m is None:
            continue
        for k, v in m[0].items():
            assert v <= fs.BARS[k], (tag, k, v)
            assert v <= fs.BARS[k] / 2, (tag, k, v, "the margin is not there")


def test_the_bars_are_the_measured_maxima_times_the_margin(measured, f32ref):
    assert fs.MARGIN in (2, 4), "DESIGN.md section 4.6a: the margin goes no higher than 4"
    for k in ("lin", "log", "coef", "dct"):                          # dct: the compiled reference returns no floats, its figure is 0
        worst = max(measured["ora"][0][k], measured["ref"][0][k])
        assert fs.BARS[k] == fs.ceil1(fs.MARGIN * worst), (k, worst, fs.ceil1(fs.MARGIN * worst), "BARS drifted from what the references measure")
    # what the bars replace (tests/test_gpu_f32.py): 1e-4 of the largest bin, 1e-3 in the log domain, 0.32 scaled units at dec_bits 8
    assert fs.BARS["lin"] <= 1e-4 / 2 and fs.BARS["log"] <= 1e-3 / 5 and fs.BARS["coef"] * 256 <= 0.32 / 20


def test_the_int8_cap_holds_for_the_references(measured):
    """A condition on the rows: at most 10 % of the held values within the coefficient bar of a rounding boundary; in the rows with a
    large dec_bits every held value lies beyond both saturation bounds by more than the bar, so no value has two boundaries in reach."""
    for tag, m in measured.items():
        if m is None:
            continue
        for name, share in m[1].items():
            assert share <= fs.INT8_CAP, (tag, name, share)
    assert measured["ora"][1]["firmware"] <= fs.INT8_CAP and measured["ora"][1]["firmware_whole"] <= fs.INT8_CAP
    for name, row in fs.ROWS.items():
        tol = fs.BARS["coef"] * float(1 << row["dec_bits"])
        base, _ = fs.base_frames(row)
        C, LM, SM = fs.reference64(row, base.reshape(-1), 64, row["frame_len"])
        held = fs.clear_bands(LM, SM).all(axis=1)
        if name in fs.SATURATING:
            assert np.all((C[held] > 127.5 + tol) | (C[held] < -128.5 - tol)), name
        else:
            assert tol < 0.25, (name, "two rounding boundaries within one bar")


def test_reference64_against_oracle_on_overlapping_frames(oracle_mod):
    """hop < frame_len through reference64's own framing: the firmware row at hop 256 and the hop-1 rows against oracle.MfccF32"""
    for name in ("firmware", "f257_hop1", "g129_hop1", "g1000", "firmware_hop0"):
        row = fs.ROWS[name]
        x, _ = fs.audio(row, 131)
        ref = fs.reference64(row, x, 131, row["hop"])
        i8, f32, lm = fs.oracle_outputs(row, x, 131, row["hop"])
        lin, dlog, dco, held = fs.errors(row, ref, lm, f32)
        assert lin.max() <= fs.BARS["lin"] and dlog.max() <= fs.BARS["log"] and dco.max() <= fs.BARS["coef"], (name, lin.max(), dlog.max(), dco.max())
        near = fs.boundary_band(row, ref[0])
        assert not (fs.round_half_away(ref[0]) != i8)[held][~near[held]].any(), name


def test_the_nyquist_magnitude_cannot_be_observed():
    """ed_mfcc_f32_kernel computes |X[P / 2]| (k <= half) as mfcc.c:196-206 does, but create_mel_fbank runs over bins 0 .. P / 2 - 1 and
    stops at 4000 Hz = bin P / 4: no band reads it at any padded size, so no output can tell whether it is right."""
    for p in (128, 256, 512, 1024):
        row = dict(n_features=13, offset=1, frame_len=p, dec_bits=8, preemph=0.97)
        _, W, _ = fs.tables(row)
        assert np.nonzero(W.any(axis=0))[0].max() <= p // 4


def test_int8_of_frames_without_clear_bands_is_not_comparable(oracle_mod, f32ref):
    """Why the int8 checks hold frames of clear bands only: on the others (the square wave at fs / 2: every band 1e-8 of the largest bin)
    the two CPU references, both correct float32 code, answer int8 values far apart; on the held frames never more than one."""
    row = fs.ROWS["firmware"]
    x, _ = fs.audio(row, 5119)
    C, LM, SM = fs.reference64(row, x, 5119, row["hop"])
    held = fs.clear_bands(LM, SM).all(axis=1)
    d = np.abs(fs.oracle_outputs(row, x, 5119, row["hop"])[0].astype(int) - fs.ref_outputs(row, x, 5119, row["hop"])[0].astype(int))
    assert d[held].max() <= 1 and d[~held].max() > 10, (d[held].max(), d[~held].max())

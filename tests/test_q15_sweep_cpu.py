"""The sweep of MFCC variant C without a GPU (tests/q15_sweep.py): the rows cover the table of DESIGN.md section 4.6b, every note names
the kernel instance the restated dispatch gives its row, counts() reaches every case of the work split and of the deferred DCT batches,
the restated constants are the source's and the build's, the host library's tables have the shape, the Nyquist flag and the scale
every row claims and hold the oracle's compact matrix, and the inputs make a wrong Nyquist bin, a wrong division and a wrong sign
visible: the sensitivity conditions, computed from the oracle alone."""
import os
import re

import numpy as np
import pytest

import q15_sweep as qs

N_CUS = (8, 64, 256, 304)
FBS = sorted({r["fb"] for r in qs.ROWS.values()})


def test_the_rows_cover_the_table():
    have = set().union(*(qs.row_items(r) for r in qs.ROWS.values()))
    assert sorted(qs.full_items() - have, key=str) == [], "values of the table no row has"
    assert qs.ROWS["shipped"]["fb"] == (16000, 80.0, 7600.0, 128) and qs.ROWS["shipped"]["hop"] == 1024 and qs.ROWS["shipped"]["n_coef"] == 13
    # hop 333 and 1025 are the odd hops, and every entry of the module docstring has a row
    assert {333, 1025, 0, 1, 512, 1024} <= {r["hop"] for r in qs.ROWS.values()}
    assert {r["entry"] for r in qs.ROWS.values()} == set(qs.ENTRIES)
    # the largest count: once per shape x Nyquist, through a device entry, at a hop where frames do not overlap
    big = [r for r in qs.ROWS.values() if r["big"]]
    assert sorted(r["shape"] + (r["nyquist"],) for r in big) == sorted(qs.TABLE["shape_nyquist"])
    assert all(r["entry"] in qs.DEVICE_ENTRIES and qs.whole(r) for r in big)
    # ... and all four tile the 64 distinct base frames: a row written through a wrong or stale fid[] slot carries another frame's bits
    assert all(r["hop"] == 1024 for r in big)
    # the KWS entry: both strides odd (the unaligned instance through group_stride), one clear of the utterance, one overlapping
    a, b = qs.KWS_STRIDES
    assert a % 2 and a >= 31 * 1024 and b % 2 and b < 1024 and not qs.aligned(0, 1024, a) and not qs.aligned(0, 1024, b)


@pytest.mark.parametrize("name", list(qs.ROWS))
def test_note_names_the_instance(name):
    row = qs.ROWS[name]
    assert qs.note_instance(row["note"]) == qs.instance(row) + (row["nyquist"],), name
    s, a, nlo, nhi = qs.instance(row)
    assert s == (row["entry"] in qs.STAGE_ENTRIES)
    assert a == (not row["entry"].endswith("_odd") and row["hop"] % 2 == 0)


def test_restated_constants_are_the_source_ones():
    text = open(os.path.join(qs.CSRC, "mfcc_q15_kernels.hip")).read()
    assert (qs.eq_wpb(), qs.eq_nb(), qs.eq_buf()) == (16, 16, 1088)
    for line in ("#define EQ_TW_DWORDS ((2 * 4 + 1) * 6 * 64)",
                 "#define EQ_LDS_DWORDS(nlop, nhip) (((nlop) + (nhip)) * 64 + 1024 + EQ_TW_DWORDS + EQ_WPB * (EQ_BUF + EQ_NB * 32 + EQ_NB * 16 + EQ_NB) + 4)",
                 "const size_t lds = sizeof(u32) * EQ_LDS_DWORDS(ED_Q15_PAIRS(NLO), ED_Q15_PAIRS(NHI));",
                 "const bool aligned = ((reinterpret_cast<uintptr_t>(args->audio) & 3) == 0) && (args->frame_step % 2 == 0) && (args->group_stride % 2 == 0);",
                 "int64_t blocks = (args->n_frames + EQ_WPB - 1) / EQ_WPB;", "const int64_t cap = (int64_t)n_cu * bpc;", "if (blocks > cap) blocks = cap;",
                 "const uint32_t s0 = (uint32_t)(((uint64_t)blockIdx.x * n_frames) / gridDim.x);",
                 "const uint32_t cnt = (uint32_t)(((uint64_t)(blockIdx.x + 1) * n_frames) / gridDim.x) - s0;",
                 "if (threadIdx.x == 0) *queue = 2 * EQ_WPB;", "uint32_t i_cur = (uint32_t)w, i_next = (uint32_t)w + EQ_WPB;",
                 "if (slot == EQ_NB - 1 || last)", "const bool need_nyquist = STAGES || T->need_nyquist != 0;",
                 "if (mel_nlo == 6 && mel_nhi == 18) return ed_launch_q15_shape<6, 18>(args, dev_tab, stages, n_cu, stream);"):
        assert line in text, "the launch code changed, restate it in tests/q15_sweep.py: " + line
    assert "#define ED_Q15_PAIRS(n) (((n) + 2) / 2)" in open(os.path.join(qs.CSRC, "edison_internal.h")).read()
    # one workgroup per CU for both shapes: the kernel's LDS is most of a CU's 160 KB
    assert [qs.lds_bytes(s) for s in ((6, 18), (8, 24))] == [141328, 142352]
    assert [qs.blocks_per_cu(s) for s in ((6, 18), (8, 24))] == [1, 1]
    # what the source's #ifndef default says is what edison_amd/build.py compiles: EQ_WPB is a lab knob, which the source refuses
    # without ED_LAB and the product flags never carry (tests/test_host_cpu.py holds both ends); EQ_NB and EQ_BUF are plain defines
    from edison_amd import build as B
    guard = re.search(r"#if !defined\(ED_LAB\) && \(([^\n]*)\)\n#error", text).group(1)
    assert "defined(EQ_WPB)" in guard and "mfcc_q15_kernels.hip" in B.HIP_SOURCES
    assert not [f for f in B.product_flags() + B.PER_FILE_FLAGS.get("mfcc_q15_kernels.hip", []) if "EQ_" in f or "ED_LAB" in f]


@pytest.mark.parametrize("n_cu", N_CUS)
def test_counts_reach_every_case(n_cu):
    w, nb = qs.eq_wpb(), qs.eq_nb()
    for name, row in qs.ROWS.items():
        cs = qs.counts(row, n_cu)
        have = set().union(*(qs.cases(row, n, n_cu) for n in cs))
        want = set(qs.CASES) if row["big"] else set(qs.CASES) - {qs.BIG_CASE}
        assert have == want, (name, n_cu, "cases no count reaches, or the largest count in a row that is not marked", sorted(want ^ have))
        assert all(qs.cases(row, n, n_cu) for n in cs)
        for n in (1, 2, w - 1, w, w + 1, 2 * w + 1, w * n_cu - 1, w * n_cu + 1, 2 * w * n_cu + 1, 5 * w * n_cu + 7):
            assert n in cs
        assert ((w * nb + 1) * n_cu + 3 in cs) == row["big"] and cs[-1] == ((w * nb + 1) * n_cu + 3 if row["big"] else 5 * w * n_cu + 7)
    # the split is a partition of the frames into at most n_cu slices whose sizes differ by one at the most
    row = qs.ROWS["shipped_dev"]
    for n in qs.counts(row, n_cu) + [3 * w * n_cu + 5]:
        s = qs.split(n, n_cu)
        assert s[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(s, s[1:])) and s[-1][0] + s[-1][1] == n
        assert len(s) == qs.blocks(n, n_cu) == min(-(-n // w), n_cu) and max(c for _, c in s) - min(c for _, c in s) <= 1
        assert sum(c for _, c in s) == n
    # the largest count forces 17 frames onto some wave of every workgroup; the count before it forces it onto none
    big = (w * nb + 1) * n_cu + 3
    assert min(c for _, c in qs.split(big, n_cu)) == w * nb + 1 and max(c for _, c in qs.split(w * nb * n_cu, n_cu)) == w * nb
    # the KWS test: 31 n_utt frames fall into several cases
    tags = set().union(*(qs.cases(row, 31 * u, n_cu) for u in qs.kws_n_utt(n_cu)))
    assert {"several workgroups, uneven slices", "second frame by position", "first queue draws", "last batch partial"} <= tags


def test_inputs():
    for fb in FBS:
        row = dict(fb=fb, hop=1024)
        base, where = qs.base_frames(row)
        assert base.shape == (64, 1024) and base.dtype == np.int16
        assert len({b.tobytes() for b in base}) == 64, "the base frames are distinct"
        assert not base[where["zero"]].any() and (base[where["rail_pos"]] == 32767).all() and (base[where["rail_neg"]] == -32768).all()
        sq = base[where["square"]].astype(int)
        assert set(sq) == {32767, -32768} and (sq[1:] != sq[:-1]).all()
        assert np.count_nonzero(base[where["impulse"]]) == 1
        ch = base[where["chirp0"]].astype(int)
        assert set(ch) == {32767, -32768}, "the first chirp runs between the rails"
        rms = np.sqrt((base.astype(float) ** 2).mean(axis=1))
        assert rms[rms > 0].min() < 1.0 and (base == 32767).any(axis=1).sum() > 3      # five decades, up to clipping
        k0, k1 = qs.top_band_bins(fb)
        W = qs.oracle_weights(fb)[31]
        assert W[k0] > 0 and W[k1] > 0 and k0 < k1 <= 512, (fb, "the chirps run inside the top band")
    idx = qs.tile_index(64 * 64 + 5)
    assert np.array_equal(idx[:64], np.arange(64)) and idx[64] == 1
    for name in ("shipped", "hop1025_float", "stages_hop333", "hop0", "hop1"):
        row = qs.ROWS[name]
        base, where = qs.base_frames(row)
        for n in (1, 5, 131):
            x, ix = qs.audio(row, n, base)
            hop = row["hop"]
            assert x.size == ((n - 1) * hop + 1024 if hop else 1024)
            if hop >= 1024:
                assert all(np.array_equal(x[i * hop:i * hop + 1024], base[ix[i]]) for i in range(n))
            if hop == 0:
                assert np.array_equal(x, base[where["hop0"]])


@pytest.mark.parametrize("name", list(qs.ROWS))
def test_host_tables_are_what_the_row_claims(built_lib, oracle_mod, name):
    """ed_build_q15_tables gives the row's shape, Nyquist flag and scale, and its lanes hold the oracle's compact matrix, tap for tap --
    also where the upper edge lies above fs / 2 and the top band is cut off at bin 512"""
    row = qs.ROWS[name]
    r, t, msg = qs.host_tables(built_lib, row["fb"])
    assert r == 0, msg
    assert (t.mel_nlo, t.mel_nhi) == row["shape"] and t.need_nyquist == row["nyquist"] and t.mel_scale == row["fb"][3], (name, t.mel_nlo, t.mel_nhi, t.need_nyquist)
    Wh, Wo = qs.host_weights(t), qs.oracle_weights(row["fb"])
    assert np.array_equal(Wh, Wo), (name, "bands that differ", np.nonzero((Wh != Wo).any(axis=1))[0].tolist())
    # the packed pairs the kernel multiplies with: the same matrix, and nothing on the pad halfword behind bin 512
    Wp = qs.packed_weights(t)
    assert np.array_equal(Wp[:, :513], Wo) and not Wp[:, 513].any(), (name, "packed bands that differ", np.nonzero((Wp[:, :513] != Wo).any(axis=1))[0].tolist())
    assert bool(Wo[:, 512].any()) == bool(row["nyquist"]) and t.n_mel_coef == np.count_nonzero(Wo)
    if row["nyquist"]:
        assert Wo[31, 512] > 0 and not Wo[:30, 512].any(), "the taps on bin 512 belong to the top bands (9000 Hz: bands 30 and 31)"
    # every read of the spectrum stays inside its 513 bins (plus the pad halfword of the last pair)
    lo, hi = np.array(t.mel_lo_pair), np.array(t.mel_hi_pair)
    assert lo.min() >= 0 and hi.min() >= 0 and 2 * (lo.max() + qs.pairs(t.mel_nlo)) <= 514 and 2 * (hi.max() + qs.pairs(t.mel_nhi)) <= 514


def test_a_filterbank_beyond_the_wide_shape_is_refused(built_lib):
    r, t, msg = qs.host_tables(built_lib, (16000, 80.0, 12000.0, 128))
    assert r != 0 and "9+21" in msg, (r, msg)


# ---- the sensitivity conditions, from the oracle alone --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base_runs(oracle_mod):
    """fb -> (oracle output [64, 32], spectrogram, mel, exact band sums, wrapped band sums) of the 64 base frames"""
    out = {}
    for fb in FBS + [(16000, 80.0, 7600.0, 16384)]:
        row = dict(fb=fb, hop=1024)
        base, _ = qs.base_frames(row)
        mfcc, st = qs.oracle_outputs(row, base.reshape(-1), 64, stages=True)
        acc, wrapped = qs.band_sums(fb, st["spectrogram"])
        # the recomputation of the mel stage that the conditions below rest on is the oracle's
        assert np.array_equal(qs.trunc_div(wrapped, fb[3]), st["mel_spectrogram"]), fb
        out[fb] = (mfcc, st["spectrogram"], st["mel_spectrogram"], acc, wrapped)
    return out


@pytest.mark.parametrize("name", list(qs.ROWS))
def test_sensitivity(base_runs, name):
    row = qs.ROWS[name]
    fb, scale = row["fb"], row["fb"][3]
    mfcc, spec, mel, acc, wrapped = base_runs[fb]
    zero = int((~mfcc.any(axis=1)).sum())
    assert zero <= qs.ZERO_CAP * qs.N_BASE, (name, "base frames with an all-zero output", zero)
    if row["nyquist"]:
        s0 = spec.copy()
        s0[:, 512] = 0
        mel0 = qs.trunc_div(qs.band_sums(fb, s0)[1], scale)
        n = int((mel0[:, 31] != mel[:, 31]).sum())
        assert qs.oracle_weights(fb)[31, 512] != 0 and n >= qs.MIN_SENSITIVE, (name, "base frames whose band 31 needs the Nyquist bin", n)
        quiet = ~qs.oracle_weights(fb)[:, 512].astype(bool)
        assert np.array_equal(mel0[:, quiet], mel[:, quiet]) and quiet[:30].all()
    else:
        assert not qs.oracle_weights(fb)[:, 512].any()
    if not qs.pow2(scale):
        n = int(((wrapped % scale) != 0).any(axis=1).sum())
        assert n >= qs.MIN_SENSITIVE, (name, "base frames with a band sum that is no multiple of the scale", n)
    if scale == 32767:
        neg = np.argwhere(wrapped < 0)
        assert neg.size, (name, "no negative wrapped band sum")
        f, b = neg[0]
        floor = np.int16((int(wrapped[f, b]) // scale + 2 ** 15) % 2 ** 16 - 2 ** 15)
        assert wrapped[f, b] % scale != 0 and mel[f, b] == floor + 1, "the oracle truncates towards zero: one above the floor"


def test_no_negative_band_sum_at_a_power_of_two_scale(base_runs):
    """The sign fix of the kernel's shift division cannot be reached with these inputs: at 16384, the largest power of two the tables
    take, the chirp between the rails stays a factor of two below 2^31, and no row with a power-of-two scale wraps at all"""
    for fb, (mfcc, spec, mel, acc, wrapped) in base_runs.items():
        if qs.pow2(fb[3]):
            assert np.array_equal(acc, wrapped) and wrapped.min() >= 0, fb
    acc = base_runs[(16000, 80.0, 7600.0, 16384)][3]
    print("largest band sum at scale 16384: %d" % acc.max())
    assert 1.0e9 < acc.max() < 1.2e9 < 2 ** 31

"""The fast MFCC loop's sweep without a GPU: the rows of tests/mfcc_sweep.py launch every one of the 28 instances of ed_mfcc2_body
(by the restated launch code, mfcc_sweep.instance) but those in mfcc_sweep.EXCLUDED, each note names its row's instance, no row only
repeats others, the filterbanks have the table shapes and the non-zero last-quad weights they are there for (read from the tables
ed_build_mfcc_tables builds), and the frame counts hit every case of the restated work split (mfcc_sweep.split)."""
import ctypes

import numpy as np
import pytest

import lds_layout as L
import mfcc_sweep as ms

N_CUS = (1, 64, 256, 304)


def _missing(lib, names):
    have = set().union(*(ms.row_items(lib, ms.ROWS[n]) for n in names))
    return sorted(ms.full_items() - {("instance",) + i for i in ms.EXCLUDED} - have, key=str)


def test_there_are_28_instances():
    assert len(ms.all_instances()) == 28
    # the launch code still has the instantiations the restatement enumerates: every kernel with both flags and both shapes
    text = open(ms.CSRC + "/mfcc_kernels.hip").read()
    for k in ("ed_mfcc2_kernel", "ed_mfcc2_window_kernel", "ed_mfcc2_flag_kernel"):
        for flags in ("true, true", "true, false", "false, true", "false, false"):
            assert "%s<%s, NLO, NHI>" % (k, flags) in text, (k, flags)
    for flag in ("true", "false"):
        assert "ed_mfcc2_list_kernel<%s, NLO, NHI>" % flag in text
    assert text.count("_shape<2, 5>(") == 3 and text.count("_shape<ED_MEL_NLO_MAX, ED_MEL_NHI_MAX>(") == 3


def test_the_rows_launch_every_instance(built_lib):
    assert _missing(built_lib, ms.ROWS) == [], "items no row reaches"
    assert all(isinstance(v, str) and len(v) > 20 for v in ms.EXCLUDED.values())
    assert set(ms.EXCLUDED) <= ms.all_instances()
    reached = set().union(*(ms.row_items(built_lib, r) for r in ms.ROWS.values()))
    assert not {("instance",) + i for i in ms.EXCLUDED} & reached


@pytest.mark.parametrize("name", list(ms.ROWS))
def test_note_names_the_instance_and_the_row_stays_in_it(built_lib, name):
    """One row, one instance: at every frame count the row runs, on every device size, instance() gives what the note says; and every
    count is more than one workgroup's worth of frames somewhere (the queue hands out pairs), one-utterance rows at 31 frames."""
    row = ms.ROWS[name]
    shape = ms.bank_shape(built_lib, row["bank"], row["variant"])
    assert shape == ms.BANK_CLAIMS[row["bank"]]["shape"]
    for n_cu in N_CUS:
        counts = ms.row_counts(row, n_cu)
        assert counts and all(n % ms.unit(row) == 0 for n in counts)
        assert {ms.instance(ms.call(row, n, shape)) for n in counts} == {ms.note_instance(row["note"])}, name
        assert max(counts) > 2 * ms.ed2_wpb()
        if not row["n_utt_one"]:
            assert max(counts) >= 2 * ms.ed2_wpb() * n_cu, "every instance gets the counts up to one full grid and two frames"
    # frames never overlap and never leave their group: every frame of a launch is one whole frame of the base set
    assert row["hop"] >= ms.FRAME
    if ms.is_kws(row):
        assert row["group"][0] == ms.UTT_FRAMES and row["hop"] == ms.FRAME and row["n_coef"] == 13 and row["outs"] == "q" and row["variant"] == "B" and not row["log"]
    if row["variant"] == "TF":
        assert not row["log"] and row["entry"] != "mfcc_batches_t"


@pytest.mark.parametrize("name", list(ms.ROWS))
def test_every_row_is_needed(built_lib, name):
    assert _missing(built_lib, [n for n in ms.ROWS if n != name]) != [], "row %s reaches nothing the others do not" % name


def test_forms_reach_every_addressing_instance(built_lib):
    """The comparison across instances (FORMS) covers aligned / unaligned x plain / grouped and both list instances"""
    have = set()
    for f in ms.FORMS:
        row = ms.form_row(f, "B", False, "shipped")
        have.add(ms.instance(ms.call(row, 66, "2+5"))[:3])
    assert have == {(k, a, p) for k in ("mfcc2",) for a in (True, False) for p in (True, False)} | {("list", True, False), ("list", False, False)}


# ---- the filterbanks -----------------------------------------------------------------------------------------------------------------
def _tables(lib, bank, variant):
    fs, lo, hi, force = ms.FILTERBANKS[bank]
    return L.build_tables(lib, ms.VARIANT_CODE[variant], force, fs, lo, hi)


def _last_quads(t):
    """(lanes with a non-zero weight in quad index 2 of the narrow part, in quad index 5 of the wide part) of a 3+6 table, from the
    products the loop adds (lds_layout.mel_terms): the bins of narrow quad 2 are 4 (slo + 2) .. + 3, of wide quad 5 4 (shi + 5) .. + 3"""
    slo, shi, band, half, w4, nlo, nhi, _ = t
    assert (nlo, nhi) == (3, 6)
    terms = L.mel_terms(slo, shi, band, half, w4, nlo, nhi)
    lo_l, hi_l = 0, 0
    for lane in range(64):
        acc = terms["b%dr%d" % (int(band[lane]), lane >> 4)]
        lo_l += any(4 * (int(slo[lane]) + 2) <= k < 4 * (int(slo[lane]) + 3) for k, _ in acc["lo0"] + acc["lo1"])
        hi_l += any(4 * (int(shi[lane]) + 5) <= k < 4 * (int(shi[lane]) + 6) for k, _ in acc["hi0"] + acc["hi1"])
    return lo_l, hi_l


@pytest.mark.parametrize("variant", ["A", "B", "TF"])
def test_filterbanks_have_their_properties(built_lib, variant):
    for bank, claim in ms.BANK_CLAIMS.items():
        fs, lo, hi, force = ms.FILTERBANKS[bank]
        t = _tables(built_lib, bank, variant)
        assert "%d+%d" % (t[5], t[6]) == claim["shape"], bank
        native = L.build_tables(built_lib, ms.VARIANT_CODE[variant], False, fs, lo, hi)
        assert ("%d+%d" % (native[5], native[6]) == claim["shape"]) == claim["native"], bank
        if claim["shape"] == "3+6":
            lo_l, hi_l = _last_quads(t)
            assert (lo_l > 0) == bool(claim.get("last_narrow_quad")), (bank, lo_l)
            assert (hi_l > 0) == bool(claim.get("last_wide_quad")), (bank, hi_l)
    # the forced table holds the shipped weights: the same products in the same order (zero weights left out)
    a, b = _tables(built_lib, "shipped", variant), _tables(built_lib, "shipped_forced", variant)
    ta, tb = L.mel_terms(*a[:7]), L.mel_terms(*b[:7])
    assert {k: sorted(map(tuple, sum(v.values(), []))) for k, v in ta.items()} == {k: sorted(map(tuple, sum(v.values(), []))) for k, v in tb.items()}
    # between them the banks put a weight into the last quad of either budget
    claims = ms.BANK_CLAIMS.values()
    assert any(c.get("last_narrow_quad") for c in claims) and any(c.get("last_wide_quad") for c in claims)


def test_losing_the_last_quad_weights_is_noticed(built_lib):
    """The property check is not vacuous: with the weights of narrow quad 2 / wide quad 5 zeroed the count drops to zero"""
    t = list(_tables(built_lib, "narrow3", "B"))
    assert _last_quads(t)[0] > 0
    t[4] = t[4].copy()
    t[4][2] = 0
    assert _last_quads(t)[0] == 0
    t = list(_tables(built_lib, "wide6", "B"))
    assert _last_quads(t)[1] > 0
    t[4] = t[4].copy()
    t[4][3 + 5] = 0
    assert _last_quads(t)[1] == 0


def test_exact_mode_has_tables_for_every_bank(built_lib):
    """Exact KWS mode behind edison_mfcc_configure: the float64 kernel's table holds every bank of the sweep (ed_build_exact_tables;
    otherwise the flag rows of that bank would be refused with EDISON_E_NO_IMPL and belong into EXCLUDED)"""
    built_lib.ed_build_exact_tables.argtypes = [ctypes.c_double] * 4 + [ctypes.c_void_p]
    buf = (ctypes.c_char * (1 << 20))()
    for bank, (fs, lo, hi, _) in ms.FILTERBANKS.items():
        assert built_lib.ed_build_exact_tables(fs, lo, hi, 128.0, buf) == 0, bank


# ---- the work split ---------------------------------------------------------------------------------------------------------------------
def test_one_workgroup_per_cu():
    """The grid cap is n_cu * blocks_per_cu and the occupancy query answers 1: one workgroup's LDS is over half of a CU's, for both shapes"""
    for shape in ms.SHAPES:
        assert ms.CU_LDS_BYTES // 2 < ms.lds_bytes(shape) <= ms.CU_LDS_BYTES and ms.blocks_per_cu(shape) == 1, (shape, ms.lds_bytes(shape))
    assert ms.lds_bytes("2+5") < ms.lds_bytes("3+6")


@pytest.mark.parametrize("n_cu", N_CUS)
def test_split_tiles_the_pairs_and_the_counts_hit_every_case(n_cu):
    w, bpc = ms.ed2_wpb(), ms.blocks_per_cu("2+5")
    counts = ms.FRAME_COUNTS(n_cu, bpc)
    assert {1, 2, 3, 65535} <= set(counts)
    hit = {}
    for n in counts:
        s = ms.split(n, n_cu, bpc)
        assert len(s) == min(-(-((n + 1) // 2) // w), n_cu * bpc)
        at = 0
        for s0, cnt in s:
            assert s0 == at and cnt >= 1
            at += cnt
        assert at == (n + 1) // 2
        for c in ms.cases(n, n_cu, bpc):
            hit.setdefault(c, []).append(n)
    want = {"one workgroup, nothing drawn", "full grid, a short slice", "full grid, every slice exactly one pair per wave",
            "last pair drawn, no frame B", "last pair drawn, with frame B", "several passes", "odd"}
    if n_cu > 1:
        want |= {"waves start without a pair", "full grid, slices of one pair per wave and one more"}
    assert want <= set(hit), (sorted(want - set(hit)), "revisit FRAME_COUNTS: ED2_WPB = %d" % w)
    # the counts the issue names, by what they do
    full = 2 * w * n_cu * bpc
    assert "full grid, every slice exactly one pair per wave" in ms.cases(full, n_cu, bpc) and "full grid, every slice exactly one pair per wave" in ms.cases(full - 1, n_cu, bpc)
    assert "last pair drawn, no frame B" in ms.cases(full + 1, n_cu, bpc) and "last pair drawn, with frame B" in ms.cases(full + 2, n_cu, bpc)
    if n_cu > 1:
        assert ms.split(2 * w + 1, n_cu, bpc) == [(0, (w + 1) // 2), ((w + 1) // 2, w + 1 - (w + 1) // 2)]


@pytest.mark.parametrize("n_cu", N_CUS)
def test_rows_that_take_whole_groups_still_hit_the_cases(n_cu):
    """Rows of 3 frames and lists of 3 batches run multiples of 3: the full grid, the short slice and the drawn odd last pair are still among
    them. Utterances of 31 frames miss `every slice exactly one pair per wave` where 31 divides neither 24 n_cu nor 24 n_cu - 1: they
    run the nearest counts below and above."""
    bpc = ms.blocks_per_cu("2+5")
    for name in ("rows_B", "list_A", "exact_many"):
        hit = set().union(*(ms.cases(n, n_cu, bpc) for n in ms.row_counts(ms.ROWS[name], n_cu)))
        want = {"last pair drawn, no frame B", "odd"}
        if name != "exact_many" or n_cu > 1:          # two utterances are 31 pairs: more than one compute unit's grid takes short
            want |= {"full grid, a short slice"}
        if name != "exact_many":
            want |= {"full grid, every slice exactly one pair per wave"}
        if n_cu > 1:
            want |= {"waves start without a pair"}
        assert want <= hit, (name, sorted(want - hit))

"""The LDS layout of the fast MFCC loop (ed_mfcc2_body, edison_amd/csrc/mfcc_kernels.hip), checked from the tables and the layout
constants alone, without a GPU: every access stays where it may, every reader finds what its writer put there, the sums the mel
stage forms are the ones the earlier layout formed, term by term, and the bank-conflict account of the host-side model
(ed_mfcc2_lds_account, tables.c) is the one committed under profiles/."""
import contextlib
import importlib.util
import io
import json
import os

import pytest

import lds_layout as L

VARIANTS = {"A": 0, "B": 1}


def _account_tool():
    spec = importlib.util.spec_from_file_location("lds_account", os.path.join(L.ROOT, "tools", "lds_account.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_transpose2_slots_are_a_bijection_inside_the_buffer_and_free_of_bank_conflicts():
    """(lane 8p + c, register q) stores to slot STRIDE c + p + 8q; (lane p + 8q, register c) reads slot STRIDE c + lane: the read
    finds that very store, no two stores share a slot, all of it ends in front of the spectra's zero padding (which the loop never
    rewrites), and the eight lanes a ds_write_b128 serves together fall on eight different 16-byte slots mod 8 (32 banks)."""
    k = L.layout_constants()
    stride = k["ED2_T2_STRIDE"]
    written = {}
    for lane in range(64):
        c, p = lane & 7, lane >> 3
        for q in range(8):
            slot = stride * c + p + 8 * q
            assert slot not in written
            written[slot] = (p, q, c)
    for lane in range(64):
        p, q = lane & 7, lane >> 3
        for c in range(8):
            assert written[stride * c + lane] == (p, q, c)
    assert 4 * (max(written) + 1) <= k["ED2_S_OFF"] + 2 * 513          # floats: the pad S2[513..515] is written once, in the prologue
    assert k["ED2_S_OFF"] + 2 * 516 <= k["ED2_L_OFF"] and k["ED2_L_OFF"] + 64 <= k["ED2_XBUF_FLOATS"]
    assert k["ED2_S_OFF"] % 4 == 0 and k["ED2_L_OFF"] % 4 == 0 and k["ED2_XBUF_FLOATS"] % 4 == 0  # 16-byte reads
    for q in range(8):
        for p in range(8):                                             # one group of a ds_write_b128: lanes 8p .. 8p + 7
            assert len({(stride * c + p + 8 * q) % 8 for c in range(8)}) == 8
        for group in ((0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27), (4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31)):
            for half in (0, 32):                                       # the groups of a ds_read_b128: 16 slots mod 16
                assert len({(stride * q + lane + half) % 16 for lane in group}) == 16


@pytest.mark.parametrize("shape", sorted(L.SHAPES))
@pytest.mark.parametrize("vname", sorted(VARIANTS))
def test_mel_reads_stay_inside_the_spectrum_and_form_the_same_sums(built_lib, vname, shape):
    """Every spectrum read of the mel stage lies inside the padded spectrum float2[516], and each accumulator of each (band pair,
    quarter) adds the products the earlier tables made it add, in the same order (tests/golden/mel_terms_parent.json): only
    products with an exactly zero weight may have come or gone, so every sum is bit for bit the earlier one."""
    slo, shi, band, half, w4, nlo, nhi, _ = L.build_tables(built_lib, VARIANTS[vname], L.SHAPES[shape])
    assert (nlo, nhi) == ((3, 6) if L.SHAPES[shape] else (2, 5))
    assert slo.min() >= 0 and shi.min() >= 0 and 4 * (slo.max() + nlo) <= 516 and 4 * (shi.max() + nhi) <= 516
    assert set(half.tolist()) <= {0, 1}
    assert sorted(band[:16].tolist()) == list(range(16)) and all((band[16 * r:16 * r + 16] == band[:16]).all() for r in range(4))
    want = json.load(open(L.TERMS_FIXTURE))["%s %s" % (vname, shape)]
    got = L.mel_terms(slo, shi, band, half, w4, nlo, nhi)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


@pytest.mark.parametrize("shape", sorted(L.SHAPES))
def test_dct_inputs_are_read_where_they_are_written(built_lib, shape):
    """Lb2 = float2 u[16] | v[16] (frame A, frame B): the lane of row r, band b stores float 2 (16 (r & 1) + b) + (r >> 1); the
    64 stores fill the 64 floats once each, and the DCT reads (L4[0..3] from float2 16 (lane & 1) + 8 (lane >> 5)) stay inside."""
    _, _, band, _, _, _, _, _ = L.build_tables(built_lib, 1, L.SHAPES[shape])
    idx = sorted(2 * (16 * ((lane >> 4) & 1) + int(band[lane])) + (lane >> 5) for lane in range(64))
    assert idx == list(range(64))
    for lane in range(64):
        first = 2 * (16 * (lane & 1) + 8 * (lane >> 5))
        assert first % 4 == 0 and first + 16 <= 64


def test_lds_account_is_the_committed_one(built_lib):
    """The model's account of the loop's LDS passes, for both table shapes and for the transpose-2 stride before (66) and now, is
    the text committed as profiles/r06_mfcc_lds_account.txt; the kernel's stride is the one the account calls this kernel's."""
    tool = _account_tool()
    assert tool.T2_STRIDE == L.layout_constants()["ED2_T2_STRIDE"]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        tool.main()
    assert out.getvalue() == open(os.path.join(L.ROOT, "profiles", "r06_mfcc_lds_account.txt")).read()
    for wide in (False, True):
        before = sum(r[3] for r in tool.account(built_lib, wide, tool.T2_STRIDE_BEFORE))
        now = sum(r[3] for r in tool.account(built_lib, wide, tool.T2_STRIDE))
        assert 3 * now <= 2 * before, (wide, before, now)  # the modelled extra passes fell by at least a third

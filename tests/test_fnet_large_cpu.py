"""CPU tests of the rows of tests/fnet_large.py (float32 networks that exceed the LDS): the plain loader's
restatement refuses every one of them, the rows cover between them what the layer kernel's tiling can do, and the bit-exact host model
the GPU test compares with (fnet_pad.run) agrees with its float64 restatement within fnet_exact.bound."""
import numpy as np
import pytest

import fnet_exact as fe
import fnet_large as fl
import fnet_pad as fp


@pytest.mark.parametrize("name", list(fl.ROWS))
def test_plain_loader_refuses(name):
    """fnet_pad.plan is parse() without flags: E_NO_IMPL from one of the two LDS refusals; low_latency_conv's dense record has in_c above
    4096, which parse() meets first and answers E_SIZE ("layer field out of range")."""
    spec = fl.ROWS[name][0]
    assert fp.plan(fl.blob(name)) == dict(error=spec.get("plain", fe.E_NO_IMPL))
    if "plain" not in spec:
        assert fl.over_lds(fl.model(name)) in ("weights", "acts")
    else:
        assert max(L["inp"][2] for L in fe.conv_records(fl.model(name))) > fe.MAX_DIM


def test_named_shapes():
    """The shapes the rows are named for."""
    rec = {name: fl.records(fl.model(name))[0] for name in fl.ROWS}
    assert [(L["k_pad"], L["n_pad"]) for L in rec["dense_over"]] == [(2564, 16)]
    assert [(L["k_pad"], L["n_pad"], L["out_c"]) for L in rec["dense_wide"]] == [(700, 80, 72), (72, 16, 10)]
    assert [(L["K"], L["out_c"], L["P"], L["pad"]) for L in rec["conv_valid_pool2"]][0] == (432, 96, 2, False)
    assert [(L["K"], L["out_c"], L["P"], L["pad"], L["live"] < L["rows"]) for L in rec["conv_same_pool4"]][0] == (768, 64, 4, True, True)
    assert [L["k_pad"] * L["n_pad"] > fe.LDS_BYTES // 4 for L in rec["mixed"]] == [False, True, False]
    assert [(L["K"], L["out_c"]) for L in rec["conv_model"]][1] == (2560, 64)
    assert [(L["K"], L["out_c"]) for L in rec["low_latency_conv"]][1] == (11160, 128)
    assert fl.over_lds(fl.model("acts_over")) == "acts" and fl.over_lds(fl.model("dense_over")) == "weights"


def test_rows_cover_the_tiling():
    have = {name: fl.facts(name) for name in fl.ROWS}
    for fact in fl.REQUIRED:
        assert any(fact in f for f in have.values()), "no row covers %r" % (fact,)


@pytest.mark.parametrize("fact", [("k", "multiple_of_KC_plus_4"), ("over", "acts"), ("PAD", False, "P", 2), ("absent_rows", 4)])
def test_coverage_notices_a_missing_row(fact):
    """The coverage test is sensitive: with the rows that cover `fact` taken out, it is no longer covered."""
    have = {name: fl.facts(name) for name in fl.ROWS}
    sole = [name for name, f in have.items() if fact in f]
    assert sole
    assert not any(fact in f for name, f in have.items() if name not in sole)


def test_chunks_and_launches():
    for name in fl.ROWS:
        m = fl.model(name)
        cap = fl.cap_for(m, fl.CHUNK)
        assert fl.chunk_of(m, cap) == fl.CHUNK and fl.chunk_of(m, cap - 4 * 2) == fl.CHUNK - 1
        assert fl.launches(m, fl.N_CHUNKED, cap) == 3 * (len(fl.records(m)[0]) + 1)
        assert fl.chunk_of(m, fl.cap_for(m, 1) - 8) == 0
        assert fl.chunk_of(m) >= 128 and fl.chunk_of(m) % fl.MB == 0
    assert fl.LAYER_LDS_BYTES == 55808


@pytest.mark.parametrize("name", list(fl.ROWS))
def test_host_model_against_float64(name):
    m = fl.model(name)
    x = fl.inputs(name, 3)
    assert np.array_equal(x, fl.inputs(name, 5)[:3])
    got, prev = fp.run(m, x), x
    for i, (L, g) in enumerate(zip(fe.conv_records(m), got)):
        w64, S = fp.layer_from(m, i, prev)
        assert (np.abs(g - w64) <= fe.bound(L, S)).all(), (name, i)
        prev = g

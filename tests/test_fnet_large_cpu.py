"""CPU tests of the rows of tests/fnet_rows.py (float32 networks that exceed the LDS): the plain loader's
restatement refuses every one of them, the rows cover between them what the layer kernel's tiling can do, and the bit-exact host model
the GPU test compares with (fnet_host.run) agrees with its float64 restatement within fnet_host.bound."""
import numpy as np
import pytest

import fnet_host as fh
import fnet_plan as fpl
import fnet_rows as fr


@pytest.mark.parametrize("name", list(fr.LARGE))
def test_plain_loader_refuses(name):
    """fnet_plan.plan is parse() without flags: E_NO_IMPL from one of the two LDS refusals; low_latency_conv's dense record has in_c above
    4096, which parse() meets first and answers E_SIZE ("layer field out of range")."""
    spec = fr.LARGE[name][0]
    assert fpl.plan(fr.blob(name)) == dict(error=spec.get("plain", fpl.E_NO_IMPL))
    if "plain" not in spec:
        assert fr.plan_of(name, large=True)["lifted"] in ("weights", "acts")
    else:
        assert max(L["inp"][2] for L in fh.conv_records(fr.model(name))) > fpl.MAX_DIM


def test_named_shapes():
    """The shapes the rows are named for."""
    rec = {name: fr.plan_of(name, large=True)["layers"] for name in fr.LARGE}
    assert [(L["k_pad"], L["n_pad"]) for L in rec["dense_over"]] == [(2564, 16)]
    assert [(L["k_pad"], L["n_pad"], L["out_c"]) for L in rec["dense_wide"]] == [(700, 80, 72), (72, 16, 10)]
    assert [(L["K"], L["out_c"], L["P"], L["pad"]) for L in rec["conv_valid_pool2"]][0] == (432, 96, 2, False)
    assert [(L["K"], L["out_c"], L["P"], L["pad"], L["live"] < L["rows"]) for L in rec["conv_same_pool4"]][0] == (768, 64, 4, True, True)
    assert [L["k_pad"] * L["n_pad"] > fpl.LDS_BYTES // 4 for L in rec["mixed"]] == [False, True, False]
    assert [(L["K"], L["out_c"]) for L in rec["conv_model"]][1] == (2560, 64)
    assert [(L["K"], L["out_c"]) for L in rec["low_latency_conv"]][1] == (11160, 128)
    assert fr.plan_of("acts_over", large=True)["lifted"] == "acts" and fr.plan_of("dense_over", large=True)["lifted"] == "weights"


def test_rows_cover_the_tiling():
    have = {name: fr.large_facts(name) for name in fr.LARGE}
    for fact in fr.REQUIRED:
        assert any(fact in f for f in have.values()), "no row covers %r" % (fact,)


@pytest.mark.parametrize("fact", [("k", "multiple_of_KC_plus_4"), ("over", "acts"), ("PAD", False, "P", 2), ("absent_rows", 4)])
def test_coverage_notices_a_missing_row(fact):
    """The coverage test is sensitive: with the rows that cover `fact` taken out, it is no longer covered."""
    have = {name: fr.large_facts(name) for name in fr.LARGE}
    sole = [name for name, f in have.items() if fact in f]
    assert sole
    assert not any(fact in f for name, f in have.items() if name not in sole)


def test_chunks_and_launches():
    for name in fr.LARGE:
        p = fr.plan_of(name, large=True)
        assert p["layered"] and p["batch"] == 0 and p["n_layers"] == len(fh.conv_records(fr.model(name)))
        cap = fpl.cap_for(p, fr.CHUNK)
        assert fpl.chunk_of(p, cap) == fr.CHUNK and fpl.chunk_of(p, cap - 4 * 2) == fr.CHUNK - 1
        assert fpl.launches(p, fr.N_CHUNKED, cap) == 3 * (p["n_layers"] + 1)
        assert fpl.chunk_of(p, fpl.cap_for(p, 1) - 8) == 0
        assert fpl.chunk_of(p) >= 128 and fpl.chunk_of(p) % fpl.MB == 0
    assert fpl.LAYER_LDS_BYTES == 55808


@pytest.mark.parametrize("name", list(fr.LARGE))
def test_host_model_against_float64(name):
    m = fr.model(name)
    x = fr.inputs(name, 3)
    assert np.array_equal(x, fr.inputs(name, 5)[:3])
    got, prev = fh.run(m, x), x
    for i, (L, g) in enumerate(zip(fh.conv_records(m), got)):
        w64, S = fh.layer_from(m, i, prev)
        assert (np.abs(g - w64) <= fh.bound(L, S)).all(), (name, i)
        prev = g

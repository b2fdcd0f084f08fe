"""The branching sweep without a GPU: the rows of tests/branch_sweep.py reach every item of the restated dispatch of the fused
kernel's VALU, merge and Concat passes and of the planner's held areas (branch_sweep.paths) but those in branch_sweep.EXCLUDED, each
row is needed for at least one of them, every note agrees with the plan, the plan of every row walks (tests/plan_emulator.py) to
tests/res_ref.py bit for bit at every per-wave fill, every record reaches what the GPU tests compare, every mis-reading res_ref and
dscnn_ref know is told apart, the merge rows sit at both rails, and 60 random branching graphs walk to res_ref as well."""
import functools
import os
import sys

import numpy as np
import pytest

import branch_sweep as bs
import plan_emulator as pe
import res_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


@functools.lru_cache(maxsize=None)
def _plan(name):
    from edison_amd import _lib
    try:
        return pe.Plan(bs.blob(name))
    except _lib.EdisonError as e:
        return e.code


def _reached(name):
    plan = _plan(name)
    if isinstance(plan, int):
        return {("declined", bs.claims(bs.ROWS[name][1])["why"])}
    return bs.plan_items(plan)


def _missing(names):
    have = set().union(*(_reached(n) for n in names))
    return sorted(bs.full_set() - set(bs.EXCLUDED) - have, key=str)


def test_the_rows_cover_every_path(built_lib):
    assert _missing(bs.ROWS) == [], "items no row reaches"
    # an exclusion is a reason that names the planner's line, and no row reaches what it excludes
    assert all(isinstance(v, str) and "model_net" in v and ".c:" in v for v in bs.EXCLUDED.values())
    assert set(bs.EXCLUDED) <= bs.full_set()
    reached = set().union(*(_reached(n) for n in bs.ROWS))
    assert not set(bs.EXCLUDED) & reached, sorted(set(bs.EXCLUDED) & reached, key=str)


@pytest.mark.parametrize("name", list(bs.ROWS))
def test_every_row_is_needed(built_lib, name):
    assert _missing([n for n in bs.ROWS if n != name]) != [], "row %s reaches nothing the others do not" % name


def test_rows_stay_small():
    for name in bs.ROWS:
        shape, lay = bs.layers(name)
        assert shape[0] <= 12 and shape[1] <= 10 and len(lay) <= bs.MAX_LAYERS, name
        dense = False
        for L in lay:
            dense |= L["type"] == bs.T_DENSE
            assert dense or L.get("out_ch", 0) <= 66, name


def _fills(batch):
    """Per fill nb = 1 .. batch the smallest input count >= 5 (all five input sets) whose last pass of a wave holds nb inputs."""
    return [nb + batch * -(-(5 - nb) // batch) for nb in range(1, batch + 1)]


@pytest.mark.parametrize("name", list(bs.ROWS))
def test_note_agrees_with_the_plan_and_the_walk_with_the_restatement(built_lib, name):
    from edison_amd import _lib
    note = bs.claims(bs.ROWS[name][1])
    plan = _plan(name)
    if note.get("accelerated") == 0:
        assert plan == _lib.E_NO_IMPL, "%s: the fused planner accepts the graph" % name
        assert bs.decline_reasons(name) == {note["why"]}, name
        return
    assert not isinstance(plan, int), (name, plan)
    assert bs.decline_reasons(name) == set(), name
    have = dict(batch=plan.M.batch, frag_mode=plan.M.frag_mode, waves=plan.M.waves, accelerated=2)
    for k, v in note.items():
        assert have[k] == v, (name, k, have[k], v)
    blob = bs.blob(name)
    for n in _fills(plan.M.batch):
        x = bs.inputs(name, n)
        assert {i % 5 for i in range(n)} == set(range(5))
        got, ref = pe.run(plan, x), res_ref.run(blob, x)
        for k in ("logits", "argmax"):
            diff = np.argwhere(got[k] != ref[k])
            assert not diff.size, "%s, %d inputs: %s differs at %s" % (name, n, k, diff[0].tolist())
        if ref["softmax"] is not None:
            assert np.array_equal(got["softmax"], ref["softmax"]), (name, n)


@pytest.mark.parametrize("name", list(bs.ROWS))
def test_cut_plans_walk_to_the_restatement(built_lib, name):
    """Every cut that has a fused plan of its own walks to res_ref too (the others run layer by layer on the GPU)."""
    from edison_amd import _lib
    for li, blob in bs.cuts(name):
        try:
            plan = pe.Plan(blob)
        except _lib.EdisonError as e:
            assert e.code == _lib.E_NO_IMPL, (name, li, str(e))
            continue
        x = bs.inputs(name, plan.M.batch + 1)
        got, ref = pe.run(plan, x), res_ref.run(blob, x)
        assert np.array_equal(got["logits"], ref["logits"]), (name, li)
        assert np.array_equal(ref["logits"], res_ref.run(bs.blob(name), x)["acts"][li]), (name, li)


def _noise(k):
    return lambda a: np.random.default_rng(k).integers(-128, 128, a.shape)


def _shift(a):
    a = np.array(a, np.int64)
    a[:, 0::4] = np.clip(2 * a[:, 0::4], -128, 127)
    return a


@pytest.mark.parametrize("name", list(bs.ROWS))
def test_every_record_reaches_the_output(name):
    """What the GPU tests compare depends on every record: the logits differ from input to input, and a wrong result of any record --
    random bytes, or a one-bit shift on a quarter of its bytes -- changes the row's logits, or the record ends a cut of the row
    (branch_sweep.cuts), whose logits it is. A property of the graph and its inputs, not of a kernel."""
    blob = bs.blob(name)
    x = bs.inputs(name, 50)
    ref = res_ref.run(blob, x)
    assert len({r.tobytes() for r in ref["logits"]}) >= 15, "%s: the logits hardly depend on the input" % name
    cut = {li for li, _ in bs.cuts(name)}
    n_rec = len(ref["acts"]) - (ref["softmax"] is not None)
    for k in range(n_rec):
        noise = (res_ref.run(blob, x, corrupt=(k, _noise(k)))["logits"] != ref["logits"]).any(axis=1).sum()
        shift = (res_ref.run(blob, x, corrupt=(k, _shift))["logits"] != ref["logits"]).any(axis=1).sum()
        assert (noise >= 20 and shift >= 1) or k in cut, "%s: record %d hardly reaches the logits (noise changes %d of 50 inputs, a one-bit " \
            "shift %d) and ends no cut" % (name, k, noise, shift)


@pytest.mark.parametrize("name", list(bs.ROWS))
def test_the_rows_tell_the_misreadings_apart(name):
    blob = bs.blob(name)
    x = bs.inputs(name, 40)
    ref = res_ref.run(blob, x)
    for wrong in sorted(bs.variants(name)):
        assert wrong in bs.VARIANTS
        bad = res_ref.run(blob, x, wrong=wrong)
        assert not np.array_equal(bad["logits"], ref["logits"]), "%s: the reading `%s` gives the same logits" % (name, wrong)


def test_every_misreading_is_told_apart_by_some_row():
    seen = set().union(*(bs.variants(n) for n in bs.ROWS))
    assert seen == set(bs.VARIANTS), sorted(set(bs.VARIANTS) - seen)


def _merge_results(name):
    """Per Add / Sub / Mult record of a row: (record, op, shift, sat8 result before the ReLU tail), from res_ref's activations."""
    shape, lay = bs.layers(name)
    acts = res_ref.run(bs.blob(name), bs.inputs(name, 40))["acts"]
    out = []
    for i, L in enumerate(lay):
        if L["type"] not in (bs.T_ADD, bs.T_SUB, bs.T_MULT):
            continue
        ins = [acts[t] for t in L["src"]]
        r = res_ref.merge2(L["type"], L["out_shift"], ins[0], ins[1])
        for t in ins[2:]:
            r = res_ref.merge2(L["type"], L["out_shift"], t, r)
        assert np.array_equal(np.maximum(r, 0) if L["relu"] else r, acts[i])
        out.append((i, L["type"], L["out_shift"], r))
    return out


MERGE_ROWS = [n for n in bs.ROWS if any(L["op"] in ("add", "sub", "mult") for L in bs.ROWS[n][0]["layers"])]


@pytest.mark.parametrize("name", MERGE_ROWS)
def test_merge_rows_sit_at_both_rails(name):
    """A condition on the rows' inputs, not a tolerance: of the saturated results of every merge record of a row with a fused plan (of
    all merge records together in a declined row: `no_msrc` chains nine Adds) at least one byte is 127, one -128, and at least half
    lie strictly between, so both clamps of the merge pass and its plain arithmetic decide bytes the GPU tests compare. A rail no
    pair of int8 inputs reaches is not asked for: arm_mult_q7 gives at least -128 * 127 >> 7 = -127, a Sub at shift s >= 1 at least
    (-255 + (1 << (s - 1))) >> s > -128; the four corners of the operation say which."""
    res = _merge_results(name)
    assert res
    corner = np.array([-128, -128, 127, 127]), np.array([-128, 127, -128, 127])
    reach = {(op, shift): res_ref.merge2(op, shift, *corner) for _, op, shift, _ in res}
    for v in reach.values():
        assert v.max() == 127                             # every operation reaches the upper rail
    if bs.claims(bs.ROWS[name][1]).get("accelerated") == 0:
        res = [(-1, op, shift, np.concatenate([r.reshape(-1) for _, _, _, r in res])) for _, op, shift, _ in res[:1]]
    for i, op, shift, r in res:
        assert r.max() == 127, (name, i)
        assert r.min() == reach[(op, shift)].min(), (name, i, r.min())
        assert reach[(op, shift)].min() == -128 or (op, shift > 0) in ((bs.T_MULT, False), (bs.T_SUB, True)), (name, i)
        assert 2 * np.count_nonzero((r > -128) & (r < 127)) >= r.size, (name, i)


def test_a_dw_row_reaches_both_clamps_of_the_packing():
    """dw_border_half: without a ReLU, bytes at 127 and at -128 leave emm_pack4."""
    shape, lay = bs.layers("dw_border_half")
    assert lay[1]["type"] == bs.T_DW and not lay[1]["relu"]
    a = res_ref.run(bs.blob("dw_border_half"), bs.inputs("dw_border_half", 40))["acts"][1]
    assert a.max() == 127 and a.min() == -128 and 2 * np.count_nonzero((a > -128) & (a < 127)) >= a.size


def test_plan_walk_on_random_branching_graphs(built_lib):
    """Seeded random branching graphs (tools/fuzz_net.py random_branching_graph, which runs them on the GPU): every graph the fused
    planner accepts walks to res_ref's answer, the refused ones are refused with the documented codes, and the sample reaches held
    tensors, merge passes and DW passes."""
    import fuzz_net
    from edison_amd import _lib, nnom_import
    rng = np.random.default_rng(2025)
    walked = refused = held = merge = dwp = 0
    while walked < 60:
        shape, layers = fuzz_net.random_branching_graph(rng)
        try:
            blob = nnom_import.build_blob(shape, [dict(L) for L in layers])
            plan = pe.Plan(blob)
        except _lib.EdisonError as e:
            assert e.code in (_lib.E_SIZE, _lib.E_NO_IMPL), str(e)
            refused += 1
            continue
        x = rng.integers(-128, 128, (plan.M.batch + 1, shape[0] * shape[1] * shape[2])).astype(np.int8)
        x[0] = rng.integers(-10, 11, x.shape[1])
        got, ref = pe.run(plan, x), res_ref.run(blob, x)
        what = (shape, [(L["type"], {k: v for k, v in L.items() if k not in ("w", "b")}) for L in layers])
        assert np.array_equal(got["logits"], ref["logits"]) and np.array_equal(got["argmax"], ref["argmax"]), what
        walked += 1
        held += plan.M.hold_bytes > 0
        merge += any(R.kind in (pe.RUN_MERGE, pe.RUN_CAT) for R in plan.R)
        dwp += any(R.kind == pe.RUN_DW for R in plan.R)
    assert held >= 5 and merge >= 5 and dwp >= 5, (held, merge, dwp, refused)

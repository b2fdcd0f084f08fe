"""The int8 network sweep without a GPU: the rows of tests/net_sweep.py reach every path of the restated dispatch of the
matrix-core network kernel (net_sweep.paths = emm_layer_dispatch / emm_net_body, csrc/cnn_net_mfma_kernels.hip) but those in
net_sweep.EXCLUDED, each row is needed for at least one of them, every note agrees with the plan, and the plan of every row --
under the default planner and under each A/B knob that changes it -- walks (tests/plan_emulator.py) to oracle/net_ref.py bit for
bit."""
import functools

import numpy as np
import pytest

import net_sweep as ns
import plan_emulator as pe
from test_planner_cpu import KNOBS


@functools.lru_cache(maxsize=None)
def _plan(name, knobs=()):
    from edison_amd import _lib
    import os
    old = {k: os.environ.get(k) for k, _ in knobs}
    os.environ.update(dict(knobs))
    try:
        return pe.Plan(ns.blob(name))
    except _lib.EdisonError as e:
        return e.code
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _reached(name):
    from edison_amd import _lib
    plan = _plan(name)
    if plan == _lib.E_NO_IMPL:
        return {("accelerated", 0)}
    return ns.plan_items(plan)


def _missing(names):
    have = set().union(*(_reached(n) for n in names))
    return sorted(ns.full_set() - set(ns.EXCLUDED) - have, key=str)


def test_the_rows_cover_every_path(built_lib):
    assert _missing(ns.ROWS) == [], "items no row reaches"
    # an exclusion is a reason, and no row reaches what it excludes
    assert all(isinstance(v, str) and len(v) > 20 for v in ns.EXCLUDED.values())
    assert set(ns.EXCLUDED) <= ns.full_set()
    reached = set().union(*(_reached(n) for n in ns.ROWS))
    assert not set(ns.EXCLUDED) & reached, sorted(set(ns.EXCLUDED) & reached, key=str)


@pytest.mark.parametrize("name", list(ns.ROWS))
def test_every_row_is_needed(built_lib, name):
    """Without row `name` some item is unreached: the sweep has no row that only repeats others."""
    assert _missing([n for n in ns.ROWS if n != name]) != [], "row %s reaches nothing the others do not" % name


def test_layer_cuts_reach_every_resident_fragment_instance(built_lib):
    """The per-layer cuts of the rows (net_sweep.prefixes, run on the GPU by test_gpu_net_sweep.test_layer_cuts_bit_exact) end in
    every (tile group x epilogue) instance over LDS-resident fragments, in their own plans."""
    from edison_amd import _lib
    have = set()
    for name in ns.ROWS:
        for li, b in ns.prefixes(name):
            try:
                plan = pe.Plan(b)
            except _lib.EdisonError:
                continue
            for nb in range(1, plan.M.batch + 1):
                d = ns.paths(plan, nb)["runs"][li]
                have.add(d["tile"] + (plan.M.frag_mode == 2, d["epilogue"]))
    want = {i for i in ns.full_set() if i[0] in ("tiles", "small") and i[-2]}
    assert sorted(want - have, key=str) == []


def _corrupted(monkeypatch, blob, x, k, how):
    """oracle/net_ref.py with the k-th matrix-core layer's requantised output (its k-th call of _sat8) replaced: "noise" by uniform
    random bytes, "shift" by sat8(2 v) on every fourth channel (a one-bit shift error in one lane's register of a tile)."""
    from oracle import net_ref
    sat8, calls = net_ref._sat8, [0]

    def bad(a):
        i = calls[0]
        calls[0] += 1
        if i == k:
            if how == "noise":
                return np.random.default_rng(k).integers(-128, 128, np.shape(a)).astype(np.int8)
            a = np.array(a, copy=True)
            a[..., 0::4] *= 2
        return sat8(a)
    monkeypatch.setattr(net_ref, "_sat8", bad)
    try:
        return net_ref.run(blob, x)["logits"]
    finally:
        monkeypatch.setattr(net_ref, "_sat8", sat8)


@pytest.mark.parametrize("name", list(ns.ROWS))
def test_every_layer_reaches_the_logits(monkeypatch, name):
    """What the GPU tests compare depends on every matrix-core layer of every row: the logits differ from input to input, and a
    wrong output of any one layer -- random bytes, or a one-bit shift on a quarter of its channels -- changes the logits. This is a
    property of the graph and its inputs, not of a kernel: it holds for the general kernel under every plan (knobs, frag_mode 0)
    and for the graph's own kernel alike."""
    from oracle import net_ref
    blob = ns.blob(name)
    shape = ns.ROWS[name][0]["shape"]
    x = ns.inputs(name, 50, shape[0] * shape[1] * shape[2])
    ref = net_ref.run(blob, x)["logits"]
    assert len({r.tobytes() for r in ref}) >= 15, "%s: the logits hardly depend on the input" % name
    n_mm = sum(L["type"] in (ns.T_CONV, ns.T_DENSE) for L in ns.layers(name)[1])
    for k in range(n_mm):
        noise = (_corrupted(monkeypatch, blob, x, k, "noise") != ref).any(axis=1).sum()
        shift = (_corrupted(monkeypatch, blob, x, k, "shift") != ref).any(axis=1).sum()
        assert noise >= 20 and shift >= 1, "%s: matrix-core layer %d of %d hardly reaches the logits (noise changes %d of 50 inputs, a " \
            "one-bit shift %d)" % (name, k, n_mm, noise, shift)


def _walk(name, plan, what):
    from oracle import net_ref
    n = min(2 * plan.M.batch + 1, 5)                   # ragged against the per-wave batch
    x = ns.inputs(name, n, plan.P.in_n)
    got, ref = pe.run(plan, x), net_ref.run(ns.blob(name), x)
    for k in ("logits", "argmax"):
        diff = np.argwhere(got[k] != ref[k])
        assert not diff.size, "%s %s: %s differs at %s" % (name, what, k, diff[0].tolist())
    if ref["softmax"] is not None:
        assert np.array_equal(got["softmax"], ref["softmax"]), (name, what)


@pytest.mark.parametrize("name", list(ns.ROWS))
def test_note_agrees_with_the_plan_and_the_walk_with_the_restatement(built_lib, name):
    from edison_amd import _lib
    note = ns.claims(ns.ROWS[name][1])
    plan = _plan(name)
    if note.get("accelerated") == 0:
        assert plan == _lib.E_NO_IMPL, "%s: the matrix-core planner accepts the graph" % name
        return
    assert not isinstance(plan, int), (name, plan)
    have = dict(batch=plan.M.batch, frag_mode=plan.M.frag_mode, waves=plan.M.waves, accelerated=2)
    for k, v in note.items():
        assert have[k] == v, (name, k, have[k], v)
    _walk(name, plan, "default plan")


def _knob_cases():
    out = []
    for name in ns.ROWS:
        for k in KNOBS[1:]:
            out.append(pytest.param(name, tuple(sorted(k.items())), id="%s-%s" % (name, "+".join("%s=%s" % kv for kv in k.items()))))
    return out


def _same_plan(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("koff", "coltab", "xtab", "frag", "seeds")) and a.M == b.M and a.R == b.R and a.ML == b.ML


def knob_changes_plan(name, knobs):
    """Whether the A/B knobs `knobs` (tuple of (name, value)) change row `name`'s plan (False when the graph has none)."""
    a, b = _plan(name), _plan(name, knobs)
    if isinstance(a, int) or isinstance(b, int):
        return a != b
    return not _same_plan(a, b)


@pytest.mark.parametrize("name,knobs", _knob_cases())
def test_knob_plans_walk_to_the_restatement(built_lib, name, knobs):
    if not knob_changes_plan(name, knobs):
        return                                           # the same plan as the default: walked above
    plan = _plan(name, knobs)
    assert not isinstance(plan, int), (name, knobs, plan)
    _walk(name, plan, dict(knobs))


def test_knobs_change_most_plans(built_lib):
    """The knob reruns are not empty: every knob changes the plan of some row."""
    for k in KNOBS[1:]:
        assert any(knob_changes_plan(n, tuple(sorted(k.items()))) for n in ns.ROWS), k

"""The float-network sweep without a GPU: the rows of tests/fnet_rows.py cover every path of the restated plan
(tests/fnet_plan.py plan = parse() in csrc/edison_fnet.hip), fma32 is glibc's fmaf bit for bit, the host model of the kernel stays
within the GPU tests' bound of the float64 restatement (tests/fnet_host.py), and the bit-exact check sees wrong arithmetic that the
bound alone does not."""
import ctypes
import ctypes.util
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from edison_amd import cube_import

import fnet_host as fh
import fnet_plan as fpl
import fnet_rows as fr

VARIANTS = ("reversed", "rounded_product", "f64_sum", "drop_last")
bound = fh.bound


@pytest.fixture(scope="module")
def plans():
    return {name: fpl.plan(fr.blob(name)) for name in fr.SWEEP}


def _dense(L):
    return tuple(L["k"]) == tuple(L["inp"][:2]) and tuple(L["out"][:2]) == (1, 1)


@functools.lru_cache(maxsize=None)
def _facts(name):
    """What row `name` takes, read from its plan, its model and the host model's outputs: a set of hashable facts."""
    p, spec = fpl.plan(fr.blob(name)), fr.SWEEP[name][0]
    m = fh.load(fr.blob(name))
    recs = fh.conv_records(m)
    f = set()
    for k, v in fr.path(p).items():
        f |= {(k, x) for x in v}
    f |= {("NG>=3",) for x in fr.path(p)["NG"] if x >= 3} | {("n_out>=200",) for x in fr.path(p)["n_out"] if x >= 200}
    if 1 < p["batch"] < 16:
        f.add(("batch_mid",))
    if p["n_layers"] == fpl.MAX_LAYERS and max(L["rows"] for L in p["layers"]) > 1:
        f.add(("layers16_maps",))                 # the most records the plan holds, with maps of several rows per utterance
    if fr.w_floats(p) > fr.STEP_PASS * 256:
        f.add(("step_second_pass",))              # more packed weights than one pass of the optimiser's step kernel covers on 256 CUs
    K0 = recs[0]["k"][0] * recs[0]["k"][1] * recs[0]["inp"][2]
    if len(recs) == 1 and _dense(recs[0]) and not recs[0]["b"].any():
        f.add(("ladder", K0))
    f.add(("in_c>=3",)) if m["in_shape"][2] >= 3 else None
    if len(recs) >= 2 and all(_dense(L) for L in recs):
        f.add(("dense_only",))
    if not _dense(recs[-1]) and recs[-1]["out"][0] * recs[-1]["out"][1] > 1:
        f.add(("conv_last_map",))
    if "synth" in spec and any(t == ("relu",) for t in spec["synth"]):
        f.add(("imported_relu_folded",))
    for L in recs:
        ih, iw, ic = L["inp"]
        (kh, kw), (sh, sw), (ph, pw) = L["k"], L["s"], L["p"]
        oh, ow = (ih - kh) // sh + 1, (iw - kw) // sw + 1
        f |= {("pool", ph, pw), ("stride", sh, sw), (("dense" if _dense(L) else "conv"), "relu", L["relu"]), ("out_c", L["out"][2])}
        f |= {("out_c>=129",)} if L["out"][2] >= 129 else set()
        if oh % ph:
            f.add(("trunc", ph, pw, "h"))
        if ow % pw:
            f.add(("trunc", ph, pw, "w"))
        if not _dense(L):
            f |= {("1x1",)} if (kh, kw) == (1, 1) else set()
            f |= {("span_h",)} if kh == ih else set()
            f |= {("span_w",)} if kw == iw else set()
    for Lp in p["layers"]:
        if Lp["k_pad"] * Lp["n_pad"] == p["w_lds"] and p["batch"] == 1 and p["lds_bytes"] + 4 * (4 * Lp["n_pad"] + 4 + 4) > fpl.LDS_BYTES:
            f.add(("largest_weights_batch1",))    # 4 more k rows would not load
        if Lp["P"] == 4 and any(nu * Lp["rows"] % 16 for nu in range(1, p["batch"] + 1)):
            f.add(("m_tail_P4",))
    if 0 <= fpl.LDS_BYTES - p["lds_bytes"] <= 1024:
        f.add(("lds_within_1k",))
    if p["batch"] > 1 and 4 * p["batch"] * sum(p["buf_n"]) >= 0.75 * fpl.LDS_BYTES:
        f.add(("batch_mid_by_activations",))      # a tile of several utterances whose activations fill most of the LDS
    # from the host model's outputs: subnormals with zero bias; ReLU logits that are all 0 for some input
    sets = spec.get("sets", fr.SETS)
    x = fr.inputs(name, len(sets), p["in_n"])
    outs = fh.run(m, x)
    if all(not L["b"].any() for L in recs):
        o = np.concatenate([a.ravel() for a in outs])
        if ((o != 0) & (np.abs(o) < np.finfo(np.float32).tiny)).sum() > 100:
            f.add(("subnormal_outputs",))
    if recs[-1]["relu"] and any(not z.any() for z in outs[-1]):
        f.add(("relu_logits_all_zero",))
    return frozenset(f)


# every item the sweep must cover; each row is there for at least one item no other row gives
REQUIRED = (
    [("ladder", 4), ("ladder", 5), ("ladder", 8), ("n_out", 1), ("n_out", 2), ("n_out>=200",)]
    + [("P", v) for v in (1, 2, 4)] + [("K4", v) for v in range(4)] + [("nt", v) for v in range(1, 5)] + [("NG", 1), ("NG", 2), ("NG>=3",)]
    + [("pool", 1, 1), ("pool", 2, 1), ("pool", 1, 2), ("pool", 2, 2), ("pool", 4, 1), ("pool", 1, 4)]
    + [("trunc", 2, 1, "h"), ("trunc", 1, 2, "w"), ("trunc", 2, 2, "h"), ("trunc", 2, 2, "w"), ("trunc", 4, 1, "h"), ("trunc", 1, 4, "w")]
    + [("stride", 1, 1), ("stride", 2, 1), ("stride", 1, 2), ("stride", 3, 2), ("1x1",), ("span_h",), ("span_w",)]
    + [(k, "relu", r) for k in ("conv", "dense") for r in (0, 1)] + [("relu_logits_all_zero",)]
    + [("out_c", v) for v in (1, 15, 16, 17, 64, 65)] + [("out_c>=129",)]
    + [("in_c>=3",), ("dense_only",), ("conv_last_map",), ("layers", 16), ("imported_relu_folded",)]
    + [("batch", 1), ("batch", 16), ("batch_mid",), ("batch_mid_by_activations",), ("lds_within_1k",), ("largest_weights_batch1",)]
    + [("m_tail_P4",), ("subnormal_outputs",), ("layers16_maps",), ("step_second_pass",)]
)


def _missing(names):
    have = set().union(*(_facts(n) for n in names))
    return [r for r in REQUIRED if r not in have]


def test_the_rows_cover_every_path():
    assert all("error" not in fpl.plan(fr.blob(n)) for n in fr.SWEEP)
    assert _missing(fr.SWEEP) == []
    # the arithmetic ladder comes first, in order K = 4, 5, 8
    assert [next(iter(k for k in _facts(n) if k[0] == "ladder"), None) for n in list(fr.SWEEP)[:3]] == [("ladder", 4), ("ladder", 5), ("ladder", 8)]
    # the loader's refusals, each with its code (test_refusal_code)
    assert set(fr.SWEEP_REFUSALS) == {"pool31", "layers17", "weights_over_lds", "lds_batch1", "k_pad", "n_pad"}


@pytest.mark.parametrize("name", list(fr.SWEEP))
def test_every_row_is_needed(name):
    """Without this row some required item is no longer covered."""
    assert _missing([n for n in fr.SWEEP if n != name]), "%s adds nothing the other rows do not cover" % name


@pytest.mark.parametrize("name", list(fr.SWEEP))
def test_note_agrees_with_the_plan(plans, name):
    have = fr.path(plans[name])
    for k, v in fr.claims(fr.SWEEP[name][1]).items():
        assert have[k] == v, (name, k, v, have[k])


@pytest.mark.parametrize("name", list(fr.SWEEP_REFUSALS))
def test_refusal_code(name):
    build, code, _ = fr.SWEEP_REFUSALS[name]
    assert fpl.plan(build()) == dict(error=code)


def test_shipped_plan():
    with open(os.path.join(GOLDEN, "cube_kws.ednf"), "rb") as f:
        p = fpl.plan(f.read())
    assert (p["batch"], p["lds_bytes"], p["n_layers"], p["n_out"]) == (7, 159808, 5, 10)
    assert p["acts_floats"] == 13 * 9 * 16 + 5 * 7 * 32 + 3 * 5 * 64 + 3 * 32 + 10


def test_importer_blob_n_out_is_the_whole_output():
    """The header's n_out is out_h x out_w x out_c of the last conv (what the loader checks), not its channel count."""
    p = fpl.plan(fr.blob("conv_last_map"))
    assert p["n_out"] == 16 and cube_import.read_blob(fr.blob("conv_last_map"))["n_out"] == 16


# ---- fma32 ------------------------------------------------------------------------------------------------------------------------
def _fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    f = libm.fmaf
    f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    return lambda a, b, c: np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)


def _same_bits(x, y):
    return np.array_equal(np.asarray(x, np.float32).view(np.int32), np.asarray(y, np.float32).view(np.int32))


def _f32_bits(rng, n, lo, hi):
    """n float32 with random sign and mantissa and exponent field in [lo, hi] (0 = subnormal)."""
    bits = (rng.integers(0, 2, n) << 31) | (rng.integers(lo, hi + 1, n) << 23) | rng.integers(0, 1 << 23, n)
    return bits.astype(np.uint32).view(np.float32)


def test_fma32_is_glibc_fmaf():
    fmaf, rng = _fmaf(), np.random.default_rng(7)
    n = 40000
    cases = []
    # random operands over the whole normal range (products and sums that overflow are left out below)
    a, b, c = (_f32_bits(rng, n, 1, 254) for _ in range(3))
    cases.append((a, b, c))
    # near-unit operands with close exponents: long carries and rounding in every position
    a, b, c = (_f32_bits(rng, n, 120, 134) for _ in range(3))
    cases.append((a, b, c))
    # exact and near cancellations: c = -(a b) rounded, perturbed by a few ulps
    a, b = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    c = -(a * b)
    c = (c.view(np.int32) + rng.integers(-2, 3, n).astype(np.int32)).view(np.float32)
    cases.append((a, b, c))
    # subnormal results: products and addends around 2^-126 .. 2^-149, subnormal operands
    a, b = _f32_bits(rng, n, 50, 75), _f32_bits(rng, n, 50, 75)
    c = _f32_bits(rng, n, 0, 3)
    cases.append((a, b, c))
    a, b, c = _f32_bits(rng, n, 0, 2), _f32_bits(rng, n, 120, 140), _f32_bits(rng, n, 0, 2)
    cases.append((a, b, c))
    # signed zeros
    z = np.array([0.0, -0.0], np.float32)
    g = np.array(np.meshgrid(z, z, z, [1.0, -1.0])).reshape(4, -1).astype(np.float32)
    cases.append((g[0], g[1], g[2]))
    cases.append((g[3], g[0], g[1]))
    cases.append((g[0], g[3], g[2]))
    total = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for a, b, c in cases:
            keep = np.isfinite(a.astype(np.float64) * b + c) & (np.abs(a.astype(np.float64) * b + c) < 3.0e38)
            a, b, c = a[keep], b[keep], c[keep]
            assert _same_bits(fh.fma32(a, b, c), fmaf(a, b, c))
            total += a.size
    assert total >= 100000


def test_fma32_where_the_float64_sum_rounds_wrong():
    """(1 + j 2^-23)(2 - j 2^-22) = 2 - j^2 2^-45 exactly: added to c = 2^25 + 4 m its float64 sum is a float32 tie, the exact sum
    is not. Rounding float64(a b + c) to float32 goes the wrong way whenever ties-to-even picks the far side; fma32 does not."""
    fmaf = _fmaf()
    j = np.arange(1, 200, dtype=np.float64)
    m = np.arange(1, 200, 2, dtype=np.float64)
    J, M = np.meshgrid(j, m)
    a = (1 + J * 2.0 ** -23).astype(np.float32).ravel()
    b = (2 - J * 2.0 ** -22).astype(np.float32).ravel()
    c = (2.0 ** 25 + 4 * M).astype(np.float32).ravel()
    cases = [(a, b, c), (-a, b, -c), (a * np.float32(2.0 ** -40), b, c * np.float32(2.0 ** -40)), (a, -b * np.float32(2.0 ** 60), -c * np.float32(2.0 ** 60))]
    for a, b, c in cases:
        want = fmaf(a, b, c)
        naive = (a.astype(np.float64) * b + c).astype(np.float32)
        assert not (naive == want).any()          # every case: the naive route is wrong ...
        assert _same_bits(fh.fma32(a, b, c), want)  # ... and fma32 is right


# ---- the host model against the float64 restatement, and what the bit check sees ----------------------------------------------
def _row_inputs(name, p, n=None):
    return fr.inputs(name, n or min(3 * p["batch"] + 2, 12), p["in_n"])


@pytest.mark.parametrize("name", list(fr.SWEEP))
def test_model_within_the_bound(plans, name):
    m = fh.load(fr.blob(name))
    x = _row_inputs(name, plans[name])
    prev = x
    for i, (L, got) in enumerate(zip(fh.conv_records(m), fh.run(m, x))):
        want, S = fh.layer_from(m, i, prev)
        assert (np.abs(got - want) <= bound(L, S)).all(), (name, i)
        prev = got
    if ("relu_logits_all_zero",) in _facts(name):
        logits = fh.run(m, x)[-1]
        zero = ~logits.any(axis=1)               # every logit 0: probs tie, the first maximum is class 0
        assert (np.argmax(fh.softmax(logits[zero]), axis=1) == 0).all()


SENSITIVE_ROWS = [n for n in fr.SWEEP if max(L["K"] for L in fpl.plan(fr.blob(n))["layers"]) >= 8]


@functools.lru_cache(maxsize=None)
def _variants(name):
    """variant -> (changes at least one output bit, stays within 8e-7 S at every layer), each layer fed the exact previous one."""
    m = fh.load(fr.blob(name))
    sets = fr.SWEEP[name][0].get("sets", fr.SETS)
    x = fr.inputs(name, 2 * len(sets), fpl.plan(fr.blob(name))["in_n"])
    x = x[[i for i in range(len(x)) if sets[i % len(sets)] in ("n1", "n60", "i16")]]
    exact = fh.run(m, x)
    out = {}
    for v in VARIANTS:
        prev, changed, within = x, False, True
        for i, L in enumerate(fh.conv_records(m)):
            got = fh.layer(L, prev, v)
            changed |= not np.array_equal(got, exact[i])
            want, S = fh.layer_from(m, i, prev)
            within &= bool((np.abs(got - want) <= bound(L, S)).all())
            prev = exact[i]
        out[v] = (changed, within)
    return out


@pytest.mark.parametrize("name", SENSITIVE_ROWS)
def test_wrong_arithmetic_changes_bits(name):
    """On every row whose largest K is >= 8, each wrong variant changes at least one output bit."""
    for v, (changed, _) in _variants(name).items():
        assert changed, (name, v)


def test_the_bound_alone_misses_wrong_arithmetic():
    """What the bit check adds: reversed k order, a rounded product then an add and the float64 sum rounded
    once all stay within the 8e-7 S bound on every row with K >= 8; only the bit check sees them. Dropping the last k term the bound
    sees too."""
    within = {v: [n for n in SENSITIVE_ROWS if _variants(n)[v][1]] for v in VARIANTS}
    print("rows where the variant stays within 8e-7 S (seen only by the bit check):", {v: len(r) for v, r in within.items()})
    for v in ("reversed", "rounded_product", "f64_sum"):
        assert within[v] == SENSITIVE_ROWS, v
    assert within["drop_last"] == []

"""CPU tests of DW_Conv2D and AvgPool support: the importer, the host planners and the numpy restatement (tests/dscnn_ref.py)
against tests/golden/dscnn_golden.npz -- layer outputs of the REFERENCE's NNoM 0.3.0 + CMSIS-NN compiled around the three
dscnn_*.h headers (tests/golden/gen_fixtures_dscnn.py). No GPU.

About the two AvgPool routines. The issue expected them to round differently. In the build the fixtures come from
(no ARM_MATH_DSP) they do not: arm_avepool_q7_HWC's portable branch computes `sum / count` over the taps inside the image
(arm_pool_q7_HWC.c:424-446), local_avepool_q7_HWC `sum / (count >> 0)` (nnom_local.c:45-67) -- the same C division. What
does differ is the WINDOW: the square routine is handed kernel.w / pad.w / stride.w only and uses them on both axes
(nnom_avgpool.c:76-86). That is the "CMSIS rule" the wrong-variant tests below apply on the wrong branch.
"""
import hashlib
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
NAMES = ["kws", "edges", "square"]

# sha256 of the blob the importer made from each committed header BEFORE the two layers were added, and of the shipped blob
# (edison_amd/data/kws_nnom.ednn; the header it was made from belongs to the reference and is not in this repository)
OLD_BLOBS = {
    "even_same": "d06ce1549ad64631b1bfea4214bba1d83f07feff29ae5acd70af4d8f4c3a4c0f",
    "kws_small": "38b2ae12ba781b4341a5e06046bab6148c725f5722e070b5d6dc2a7b68581766",
    "low_latency_small": "aa51c75c06505674acb3157a5fbe095ee3cf23e96143a38e0ef548f556dcc407",
    "odd_no_softmax": "6b5922d3ad7f6d2ba0a055d522db7899a68641a1f86784ff8c80838700f91142",
    "same_stride": "62d3d1f623787b98160ab2091744e766f22cab34f947cfcaaef521c07fd4f05e",
    "square": "f2587d71353204ded1d971a4f026aafe849e6d64b602f62ce39ff9eac211511b",
    "tiny_conv": "6e026b3c3b1a05a973804d28e711a250167a439c59f87ea6bbc137b07542aec0",
}
SHIPPED = "b4fe789c79f4aa3329a4b93effe106b82146cea8be6c4e95c0f5d17cf3d870d5"


def _text(name):
    with open(os.path.join(GOLDEN, "alt_models", name + ".h")) as f:
        return f.read()


def _blob_of(text):
    from edison_amd import nnom_import
    shape, layers = nnom_import.parse_weights_h(text)
    return nnom_import.build_blob(shape, layers)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "dscnn_golden.npz"))


@pytest.fixture(scope="module")
def blobs():
    return {n: _blob_of(_text("dscnn_" + n)) for n in NAMES}


# ---------------------------------------------------------------------------------------------------------------- importer
@pytest.mark.parametrize("name", NAMES)
def test_importer_round_trips_the_header(name, blobs):
    """Every number of the header is found again in the blob: graph, geometry, shifts, flags and the tensors, in [ky][kx][ch] order."""
    from edison_amd import nnom_import as imp
    from oracle import net_ref
    text = _text("dscnn_" + name)
    shape, layers = imp.parse_weights_h(text)
    (h, w, c), recs, payload = net_ref.parse_blob(blobs[name])
    assert (h, w, c) == shape and len(recs) == len(layers)
    stmts = [s for s in re.findall(r"layer\[\d+\]\s*=\s*model\.hook\((.*), layer\[\d+\]\);", text) if not s.startswith(("Output", "Flatten"))]
    assert len(stmts) == len(recs)
    arrays = {m.group(1): np.array([int(t) for t in m.group(2).split(",")]) for m in re.finditer(r"#define\s+(\w+)\s+\{([^}]*)\}", text)}
    shifts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(\w+SHIFT)\s+\((\d+)\)", text)}
    n_dw = 0
    for i, (s, v) in enumerate(zip(stmts, recs)):
        if s.startswith("DW_Conv2D"):
            n_dw += 1
            kh, kw, sh, sw = (int(t) for t in re.search(r"kernel\((\d+), (\d+)\), stride\((\d+), (\d+)\)", s).groups())
            up = "DEPTHWISE_CONV2D_%d" % n_dw
            assert v[0] == imp.T_DWCONV == 5 and tuple(v[2:6]) == (kh, kw, sh, sw) and v[1] == v[11] == c
            assert v[6] == shifts[up + "_BIAS_LSHIFT"] and v[7] == shifts[up + "_OUTPUT_RSHIFT"]
            assert (v[8] >> 1) & 1 == int("PADDING_SAME" in s)
            assert np.array_equal(payload[v[9]:v[9] + kh * kw * c], arrays[up + "_KERNEL_0"]) and v[9] % 16 == 0
            assert np.array_equal(payload[v[10]:v[10] + c], arrays[up + "_BIAS_0"])
            same = (v[8] >> 1) & 1
            h, w = imp.out_dim(h, kh, sh, same), imp.out_dim(w, kw, sw, same)
        elif s.startswith("AvgPool"):
            kh, kw, sh, sw = (int(t) for t in re.search(r"kernel\((\d+), (\d+)\), stride\((\d+), (\d+)\)", s).groups())
            assert v[0] == imp.T_AVGPOOL == 6 and tuple(v[2:6]) == (kh, kw, sh, sw) and v[7] == 0 and v[8] == 2 * int("PADDING_SAME" in s)
            assert v[1] == v[6] == v[9] == v[10] == v[11] == 0
            same = (v[8] >> 1) & 1
            h, w = imp.out_dim(h, kh, sh, same), imp.out_dim(w, kw, sw, same)
        elif v[0] == imp.T_CONV:
            same = (v[8] >> 1) & 1
            h, w, c = imp.out_dim(h, v[2], v[4], same), imp.out_dim(w, v[3], v[5], same), v[1]
        elif v[0] == imp.T_DENSE:
            h, w, c = 1, 1, v[1]
    # the ReLU tail of a DW_Conv2D is folded into its record like a Conv2D's
    want_relu = []
    for line in re.findall(r"layer\[\d+\]\s*=\s*(.*);", text):
        if "act_relu()" in line:
            want_relu[-1] = 1
        elif "model.hook(" in line and not re.search(r"hook\((Output|Flatten)", line):
            want_relu.append(0)
    assert [v[8] & 1 for v in recs] == want_relu


def test_blobs_without_the_new_layers_are_byte_identical():
    for name, sha in OLD_BLOBS.items():
        assert hashlib.sha256(_blob_of(_text(name))).hexdigest() == sha, name
    with open(os.path.join(ROOT, "edison_amd", "data", "kws_nnom.ednn"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == SHIPPED


def _edit(name, old, new, count=1):
    text = _text("dscnn_" + name)
    assert text.count(old) >= 1, old
    return text.replace(old, new, count)


@pytest.mark.parametrize("what, text_of, word", [
    ("multiplier 2", lambda: _edit("edges", "DW_Conv2D(1, kernel(2, 2)", "DW_Conv2D(2, kernel(2, 2)"), "DW_Conv2D"),
    ("odd channels", lambda: _edit("edges", "Conv2D(6, kernel(1, 1)", "Conv2D(5, kernel(1, 1)"), "DW_Conv2D"),
    ("PADDING_FOO on DW_Conv2D", lambda: _edit("edges", "stride(2, 2), PADDING_SAME", "stride(2, 2), PADDING_FOO"), "DW_Conv2D"),
    ("PADDING_FOO on AvgPool", lambda: _edit("edges", "AvgPool(kernel(3, 2), stride(1, 1), PADDING_SAME)", "AvgPool(kernel(3, 2), stride(1, 1), PADDING_FOO)"), "AvgPool"),
    ("GlobalAvgPool", lambda: _edit("edges", "AvgPool(kernel(3, 2), stride(1, 1), PADDING_SAME)", "GlobalAvgPool()"), "GlobalAvgPool"),
    ("GlobalMaxPool", lambda: _edit("edges", "AvgPool(kernel(3, 2), stride(1, 1), PADDING_SAME)", "GlobalMaxPool()"), "GlobalMaxPool"),
    ("SumPool", lambda: _edit("edges", "AvgPool(kernel(3, 2)", "SumPool(kernel(3, 2)"), "SumPool"),
    ("ZeroPadding", lambda: _edit("edges", "AvgPool(kernel(3, 2), stride(1, 1), PADDING_SAME)", "ZeroPadding(border(1, 1, 1, 1))"), "ZeroPadding"),
    ("DW weights of the wrong size", lambda: _edit("edges", "DW_Conv2D(1, kernel(2, 2)", "DW_Conv2D(1, kernel(3, 2)"), "DW_Conv2D"),
])
def test_importer_refusals_name_the_layer(what, text_of, word):
    from edison_amd import nnom_import as imp
    with pytest.raises(ValueError) as e:
        imp.parse_weights_h(text_of())
    assert word in str(e.value), (what, str(e.value))


# ---------------------------------------------------------------------------------------------------------------- planners
@pytest.mark.parametrize("name", NAMES)
def test_host_plans_cover_the_new_layers(name, blobs):
    """ed_plan_net / ed_plan_net_mm: shapes as the restatement's, a plan for the fused kernel with an ED_RUN_DW (5) / ED_RUN_AVG (6)
    pass per new layer, inputs and outputs of those passes inside the wave's activation region."""
    import dscnn_ref
    import plan_emulator
    from oracle import net_ref
    P = plan_emulator.Plan(blobs[name])
    _, recs, _ = net_ref.parse_blob(blobs[name])
    r = dscnn_ref.run(blobs[name], np.zeros((1, P.P.in_n), np.int8))
    assert [L.out_n for L in P.PL] == [a.shape[1] for a in r["acts"]]
    assert [L.type for L in P.PL] == [v[0] for v in recs]
    region = 2 * P.M.buf_bytes
    for L, R in zip(P.PL, P.R):
        if L.type in (5, 6):
            assert R.kind == L.type
            assert R.in_img >= L.in_n and 0 <= R.in_off and R.in_off + P.M.batch * R.in_img <= region
            last = R.o_origin + (L.out_h - 1) * R.o_row + (L.out_w - 1) * R.oc_pitch + L.out_c
            assert last <= R.o_img and 0 <= R.o_off and R.o_off + P.M.batch * R.o_img <= region
            assert R.oc_pitch % 2 == 0 and (L.in_c % 4 or R.oc_pitch % 4 == 0)
        if L.type == 5:
            c4n = (L.in_c + 3) // 4
            assert R.seed_off % 4 == 0 and R.seed_off + 4 * c4n <= P.seeds.size
            assert R.frag_off % 16 == 0 and R.frag_off + 4 * c4n * L.kh * L.kw <= P.frag.size


def test_square_avgpool_plans_the_window_the_reference_uses(blobs):
    import plan_emulator
    P = plan_emulator.Plan(blobs["square"])
    L = P.PL[1]
    assert L.type == 6 and (L.in_h, L.in_w, L.out_h, L.out_w) == (8, 8, 8, 8)
    assert (L.kh, L.kw, L.sh, L.sw, L.pad_h, L.pad_w) == (3, 3, 1, 1, 1, 1)       # the header says kernel(2, 3)
    L = plan_emulator.Plan(blobs["edges"]).PL[3]
    assert L.type == 6 and (L.kh, L.kw, L.pad_h, L.pad_w) == (3, 2, 1, 0)         # a non-square map keeps its own window


def test_spec_source_is_declined_for_these_graphs(blobs):
    """A graph with a new layer is not specialised: the generated-constants entry point declines with EDISON_E_NO_IMPL."""
    import ctypes
    from edison_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        buf = ctypes.create_string_buffer(blobs[name], len(blobs[name]))
        need = ctypes.c_size_t()
        assert L.edison_net_spec_source(ctypes.cast(buf, ctypes.c_void_p), len(blobs[name]), None, 0, ctypes.byref(need)) == _lib.E_NO_IMPL


# ---------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference_at_every_layer(name, blobs, golden):
    import dscnn_ref
    r = dscnn_ref.run(blobs[name], golden["in_" + name])
    off = 0
    for i, a in enumerate(r["acts"]):
        assert np.array_equal(a, golden["acts_" + name][:, off:off + a.shape[1]]), "layer %d" % i
        off += a.shape[1]
    assert off == golden["acts_" + name].shape[1]
    assert np.array_equal(r["argmax"], golden["argmax_" + name])


def test_fixture_holds_the_cases_it_is_meant_to(blobs, golden):
    """DW_Conv2D saturates at both ends, an AvgPool sees negative sums that do not divide evenly, on both routines."""
    import dscnn_ref
    from oracle import net_ref
    for name in ("edges", "square"):
        r = dscnn_ref.run(blobs[name], golden["in_" + name])
        first = r["acts"][0]                                                        # a DW_Conv2D on the raw input
        assert net_ref.parse_blob(blobs[name])[1][0][0] == 5 and first.max() == 127 and first.min() == -128, name
    for name, layer in (("kws", 6), ("edges", 2), ("square", 0)):                   # the tensor in front of an AvgPool
        r = dscnn_ref.run(blobs[name], golden["in_" + name])
        assert net_ref.parse_blob(blobs[name])[1][layer + 1][0] == 6 and (r["acts"][layer] < 0).mean() > 0.2, name


# which graphs tell each mis-reading from the reference (first layer that differs is a layer of the named kind); worked out from the
# graphs, not from a run: floor / truncation differ where an AvgPool meets negative sums (all three); the tap count matters where
# SAME cuts windows (edges, square; kws pools VALID over the whole map); the rounding term and the weight order touch every
# DW_Conv2D with more than one tap and channel (edges starts with a 1x1 kernel over 2 channels, still caught by its later layers);
# the square routine's window differs from the stated one where kh != kw: on a square map (square) or, applied wrongly, on a
# non-square one (edges: 3x2 on 4x3; kws: 2x3 on a 2x3 map, where kernel.w on both axes still covers exactly the map: not caught)
CATCHES = {
    "floor_div": {"kws": True, "edges": True, "square": True},
    "count_area": {"kws": False, "edges": True, "square": True},
    "no_round": {"kws": True, "edges": True, "square": True},
    "chw_weights": {"kws": True, "edges": True, "square": True},
    "cmsis_always": {"kws": False, "edges": True, "square": False},
    "local_always": {"kws": False, "edges": False, "square": True},
}


@pytest.mark.parametrize("wrong", sorted(CATCHES))
def test_wrong_variants_are_caught(wrong, blobs, golden):
    import dscnn_ref
    caught = {}
    for name in NAMES:
        r = dscnn_ref.run(blobs[name], golden["in_" + name], wrong=wrong)
        caught[name] = not np.array_equal(np.concatenate(r["acts"], axis=1), golden["acts_" + name])
    assert caught == CATCHES[wrong]
    assert any(caught.values())


@pytest.mark.parametrize("name", NAMES)
def test_packed_depthwise_operands_reproduce_the_layer(name, blobs, golden):
    """What the fused kernel's ED_RUN_DW pass is handed -- [tap][group of four channels] weight dwords in the fragment buffer, four
    seeds per group -- walked here as the kernel walks it, on the reference's own input of each DW_Conv2D layer: equals its output."""
    import plan_emulator
    P = plan_emulator.Plan(blobs[name])
    acts, x = golden["acts_" + name].astype(np.int64), golden["in_" + name].astype(np.int64)
    seen = 0
    for i, (L, R) in enumerate(zip(P.PL, P.R)):
        if L.type != 5:
            continue
        seen += 1
        src = x if i == 0 else acts[:, P.PL[i - 1].acts_off:P.PL[i - 1].acts_off + P.PL[i - 1].out_n]
        img = src.reshape(-1, L.in_h, L.in_w, L.in_c)
        c4n = (L.in_c + 3) // 4
        wq = P.frag[R.frag_off:R.frag_off + 4 * c4n * L.kh * L.kw].astype(np.int64).reshape(L.kh, L.kw, 4 * c4n)
        seeds = P.seeds[R.seed_off:R.seed_off + 4 * c4n].astype(np.int64)
        assert not wq[:, :, L.in_c:].any() and not seeds[L.in_c:].any()
        out = np.zeros((img.shape[0], L.out_h, L.out_w, L.in_c), np.int64)
        for y in range(L.out_h):
            for q in range(L.out_w):
                acc = np.broadcast_to(seeds[:L.in_c], (img.shape[0], L.in_c)).copy()
                for ky in range(L.kh):
                    for kx in range(L.kw):
                        iy, ix = y * L.sh - L.pad_h + ky, q * L.sw - L.pad_w + kx
                        if 0 <= iy < L.in_h and 0 <= ix < L.in_w:
                            acc += img[:, iy, ix, :] * wq[ky, kx, :L.in_c]
                out[:, y, q, :] = np.clip(acc >> (R.rs & 0xff), R.lo_clamp, 127)
        assert np.array_equal(out.reshape(img.shape[0], -1), acts[:, L.acts_off:L.acts_off + L.out_n]), "layer %d" % i
    assert seen >= 2

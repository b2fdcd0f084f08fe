"""Padded float networks without a GPU (tests/fnet_rows.py's PAD table): the float64 restatement with pads equals torch's
float64 conv2d over F.pad and max_pool2d over a -inf pad; the bit-exact host model stays within the project's bound of it; every sweep
row takes a path no other row takes; same_pads on the reference training script's shapes; blobs without pads are version 1, byte for
byte; the importer's refusals; which padded records quantise to NNoM's PADDING_SAME."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from edison_amd import cube_import
from edison_amd import quantize as qz

import cube_synth
import fnet_host as fh
import fnet_plan as fpl
import fnet_rows as fr

torch = pytest.importorskip("torch")
F = torch.nn.functional


def _n(name):
    return 2 * fpl.plan(fr.blob(name))["batch"] + 1


def _torch_layer(L, x):
    """Record L on x [n][h][w][c] float64 by torch: conv2d over a zero F.pad, bias, ReLU, max_pool2d over a -inf F.pad."""
    (pt, pl, pb, pr), (qt, ql, qb, qr) = fh.pads(L)
    t = torch.from_numpy(np.ascontiguousarray(x, np.float64)).permute(0, 3, 1, 2)
    w = torch.from_numpy(L["w"].astype(np.float64)).permute(0, 3, 1, 2).contiguous()
    y = F.conv2d(F.pad(t, (pl, pr, pt, pb)), w, torch.from_numpy(L["b"].astype(np.float64)), stride=tuple(L["s"]))
    if L["relu"]:
        y = torch.relu(y)
    if tuple(L["p"]) != (1, 1):
        y = F.max_pool2d(F.pad(y, (ql, qr, qt, qb), value=float("-inf")), tuple(L["p"]))
    return y.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("name", list(fr.PAD))
def test_restatement_is_torch_float64(name):
    m = fr.model(name)
    x = fr.inputs(name, _n(name), int(np.prod(m["in_shape"]))).astype(np.float64)
    a = x
    for i, L in enumerate(fh.conv_records(m)):
        got, _ = fh.layer_from(m, i, a)
        want = _torch_layer(L, a.reshape((-1,) + tuple(L["inp"]))).reshape(got.shape[0], -1)
        assert got.shape == want.shape and np.isfinite(want).all(), (name, i)
        assert (np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), 1e-300) + 1e-12 * np.abs(want).max()).all(), (name, i)
        a = got


@pytest.mark.parametrize("name", list(fr.PAD))
def test_model_within_the_bound(name):
    """K_BOUND 1e-7 S as for unpadded networks: a zero tap adds nothing to S and its fmaf changes nothing."""
    m = fr.model(name)
    x = fr.inputs(name, _n(name), int(np.prod(m["in_shape"])))
    prev = x
    for i, (L, got) in enumerate(zip(fh.conv_records(m), fh.run(m, x))):
        want, S = fh.layer_from(m, i, prev)
        assert np.isfinite(got).all() and (np.abs(got - want) <= fh.bound(L, S)).all(), (name, i)
        prev = got


# The plan of nine unpadded sweep rows, as the version-1 restatement gave it before there was one restatement: (n_layers, in_n, n_out,
# batch, buf_n, w_lds, k_lds, acts_floats, lds_bytes), then per layer (P, rows, K, k_pad, n_pad, NT, NG, nt_last, src, dst, relu, out_c,
# out_n, in_c, k, s, p)
V1_TOP = ("n_layers", "in_n", "n_out", "batch", "buf_n", "w_lds", "k_lds", "acts_floats", "lds_bytes")
V1_LAYER = ("P", "rows", "K", "k_pad", "n_pad", "NT", "NG", "nt_last", "src", "dst", "relu", "out_c", "out_n", "in_c", "k", "s", "p")
V1_PLANS = {
    "ladder_k4": ((1, 4, 1, 16, [4, 4], 64, 4, 1, 784),
                  [(1, 1, 4, 4, 16, 1, 1, 1, 0, 1, 0, 1, 1, 1, (1, 4), (1, 1), (1, 1))]),
    "ladder_k5": ((1, 5, 1, 16, [8, 4], 128, 8, 1, 1312),
                  [(1, 1, 5, 8, 16, 1, 1, 1, 0, 1, 0, 1, 1, 1, (1, 5), (1, 1), (1, 1))]),
    "ladder_k8": ((1, 8, 2, 16, [8, 4], 128, 8, 2, 1312),
                  [(1, 1, 8, 8, 16, 1, 1, 1, 0, 1, 0, 2, 2, 1, (2, 4), (1, 1), (1, 1))]),
    "pool21_trunc_h": ((2, 66, 3, 16, [68, 64], 1024, 64, 67, 12800),
                       [(2, 32, 9, 12, 16, 1, 1, 1, 0, 1, 1, 4, 64, 1, (3, 3), (1, 1), (2, 1)),
                        (1, 1, 64, 64, 16, 1, 1, 1, 1, 0, 0, 3, 3, 4, (4, 4), (1, 1), (1, 1))]),
    "pool12_trunc_w": ((2, 66, 3, 16, [68, 80], 1280, 80, 83, 14912),
                       [(2, 32, 9, 12, 16, 1, 1, 1, 0, 1, 0, 5, 80, 1, (3, 3), (1, 1), (1, 2)),
                        (1, 1, 80, 80, 16, 1, 1, 1, 1, 0, 0, 3, 3, 5, (4, 4), (1, 1), (1, 1))]),
    "pool22_trunc_hw": ((2, 200, 4, 16, [200, 272], 4352, 272, 276, 48704),
                        [(4, 64, 8, 8, 32, 2, 1, 2, 0, 1, 1, 17, 272, 2, (2, 2), (1, 1), (2, 2)),
                         (1, 1, 272, 272, 16, 1, 1, 1, 1, 0, 0, 4, 4, 17, (4, 4), (1, 1), (1, 1))]),
    "pool41_tail": ((2, 52, 5, 16, [52, 48], 768, 48, 53, 9664),
                    [(4, 24, 6, 8, 16, 1, 1, 1, 0, 1, 1, 8, 48, 1, (3, 2), (1, 1), (4, 1)),
                     (1, 1, 48, 48, 16, 1, 1, 1, 1, 0, 0, 5, 5, 8, (2, 3), (1, 1), (1, 1))]),
    "pool14_tail": ((2, 45, 6, 16, [48, 92], 1472, 92, 96, 15216),
                    [(4, 24, 6, 8, 16, 1, 1, 1, 0, 1, 1, 15, 90, 1, (2, 3), (1, 1), (1, 4)),
                     (1, 1, 90, 92, 16, 1, 1, 1, 1, 0, 0, 6, 6, 15, (2, 3), (1, 1), (1, 1))]),
    "batch1_lds_max": ((1, 2272, 16, 1, [2272, 16], 36352, 2272, 16, 163648),
                       [(1, 1, 2272, 2272, 16, 1, 1, 1, 0, 1, 0, 16, 16, 1, (8, 284), (1, 1), (1, 1))]),
}


@pytest.mark.parametrize("name", [n for n in fr.SWEEP if n not in ("batch1_lds_max", "layers16")][:8] + ["batch1_lds_max"])
def test_unpadded_networks_are_fnet_exact(name):
    """On a network without pads the plan and the layer model are what they were before they knew of pads: the plan's version-1 keys
    have the values pinned above and its padded keys say "no pads"; a model dict that never heard of pads and the same model with
    explicit zero pads give the same bits."""
    blob = fr.blob(name)
    assert blob[4:8] == b"\x01\0\0\0"
    q = fpl.plan(blob)
    top, layers = V1_PLANS[name]
    assert tuple(q[k] for k in V1_TOP) == top and not q["layered"] and q["lifted"] is None
    assert [tuple(b[k] for k in V1_LAYER) for b in q["layers"]] == layers
    for b in q["layers"]:
        assert not b["pad"] and b["live"] == b["rows"] and b["kn"] == b["k_pad"] and b["cpad"] == b["ppad"] == fh.Z4
    m = fh.load(blob)
    bare = dict(m, layers=[{k: v for k, v in L.items() if k not in ("cpad", "ppad")} for L in m["layers"]])
    zeros = dict(m, layers=[dict(L, cpad=fh.Z4, ppad=fh.Z4) if L["type"] == cube_import.T_CONV else L for L in m["layers"]])
    assert not any("cpad" in L or "ppad" in L for L in bare["layers"]) and all("cpad" in L for L in fh.conv_records(zeros))
    x = fr.inputs(name, 2, q["in_n"])
    for a, b in zip(fh.run(bare, x), fh.run(zeros, x)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for i in range(len(fh.conv_records(m))):
        (ya, sa), (yb, sb) = fh.layer_from(bare, i, x if i == 0 else ya), fh.layer_from(zeros, i, x if i == 0 else ya)
        assert (ya == yb).all() and (sa == sb).all()


def test_the_rows_take_different_paths():
    assert all("error" not in fpl.plan(fr.blob(n)) for n in fr.PAD)
    have = set().union(*(fr.pad_facts(n) for n in fr.PAD))
    need = [("k>in", 1), ("pad_layer", 1), ("pad_layer", 2), ("pad_NG", 2), ("pad_nt", 2), ("pad_no_relu",), ("m_tail_P4_absent",), ("batch_mid",),
            ("ppad", (2, 2), (0, 0, 1, 1)), ("ppad", (2, 1), (0, 0, 1, 0)), ("ppad", (4, 1), (1, 0, 2, 0)), ("ppad", (1, 4), (0, 1, 0, 2)),
            ("cpad", (2, 0, 0, 0), (1, 1), False), ("cpad", (0, 2, 0, 0), (1, 1), False), ("cpad", (1, 0, 1, 1), (2, 2), False)]
    assert [r for r in need if r not in have] == []
    p = fpl.plan(fr.blob("mid_pads_batch"))
    assert p["batch"] == 7 and [L["pad"] for L in p["layers"]] == [False, True, True, False]
    assert fpl.plan(fr.blob("pool22_odd"))["layers"][0]["live"] == 15 and fpl.plan(fr.blob("pool22_odd"))["layers"][0]["rows"] == 24
    # the second k table counts: a padded layer's 2 k_pad ints are the plan's k_lds where no unpadded layer has more
    q = fpl.plan(fr.blob("oc65_pad"))
    assert q["k_lds"] == max(L["kn"] for L in q["layers"]) and q["layers"][0]["kn"] == 2 * q["layers"][0]["k_pad"]


@pytest.mark.parametrize("name", list(fr.PAD))
def test_every_row_is_needed(name):
    others = set().union(*(fr.pad_facts(n) for n in fr.PAD if n != name))
    assert fr.pad_facts(name) - others, "%s takes no path the other rows do not take" % name


def test_zoo_shapes():
    """The four padded architectures at 31x13x1: the shapes Keras gives them."""
    outs = {n: [tuple(L["out"]) for L in fh.conv_records(fr.model(n))] for n in fr.ZOO}
    assert outs == dict(tiny_conv=[(16, 7, 8), (1, 1, 10)], medium_embedding_conv=[(8, 4, 16), (8, 4, 12), (1, 1, 10)],
                        tiny_embedding_conv=[(8, 4, 8), (1, 1, 8), (1, 1, 10)], simple_conv=[(15, 6, 8), (1, 1, 10)])
    m = fr.model("tiny_embedding_conv")
    second = fh.conv_records(m)[1]
    assert second["k"] == (8, 10) and second["inp"] == (8, 4, 8) and second["cpad"] == (0, 3, 0, 3)      # wider than its input
    assert fh.conv_records(fr.model("medium_embedding_conv"))[0]["ppad"] == (0, 0, 0, 1)


SAME = [((31, 8, 2), 16, (3, 4)), ((13, 10, 2), 7, (4, 5)), ((13, 8, 2), 7, (3, 4)), ((16, 2, 2), 8, (0, 0)), ((7, 2, 2), 4, (0, 1)),
        ((8, 4, 1), 8, (1, 2)), ((4, 4, 1), 4, (1, 2)), ((8, 8, 8), 1, (0, 0)), ((4, 10, 8), 1, (3, 3)), ((31, 8, 1), 31, (3, 4)),
        ((13, 8, 1), 13, (3, 4)), ((13, 20, 1), 13, (9, 10)), ((10, 3, 2), 5, (0, 1))]


def test_same_pads():
    """Keras's rule on the thirteen (in, k, stride) triples of the reference training script's architectures at 31x13 (and the 3-wide
    stride-2 kernel over 10 columns): out = ceil(in / s), total = max((out - 1) s + k - in, 0), before = total // 2."""
    assert len(SAME) == 13
    for (n, k, s), out, want in SAME:
        b, a = cube_import.same_pads(n, k, s)
        assert (b, a) == want, (n, k, s)
        assert (n + b + a - k) // s + 1 == out == -(-n // s)
    assert cube_import.same_pads(5, 1, 1) == (0, 0) and cube_import.same_pads(6, 1, 4) == (0, 0)       # never negative


def test_blobs_without_pads_are_version_1_byte_for_byte():
    with open(os.path.join(GOLDEN, "cube_kws.ednf"), "rb") as f:
        shipped = f.read()
    m = cube_import.read_blob(shipped)
    assert all(L["cpad"] == L["ppad"] == (0, 0, 0, 0) for L in fh.conv_records(m))
    assert cube_import.build_blob(m, m["keywords"]) == shipped                       # records read with zero pads: still version 1
    for L in m["layers"]:
        L.pop("cpad", None), L.pop("ppad", None)
    assert cube_import.build_blob(m, m["keywords"]) == shipped                       # and model dicts that never heard of pads
    for name in ("pool22_trunc_hw", "synth_pool12_relu"):
        b = fr.blob(name)
        assert b[4:8] == b"\x01\0\0\0" and cube_import.build_blob(cube_import.read_blob(b)) == b
    # a padded model: version 2, 24-int records, and it reads back to the same bytes
    b = fr.blob("pool22_odd")
    assert b[4:8] == b"\x02\0\0\0" and cube_import.build_blob(cube_import.read_blob(b)) == b
    v1 = cube_import.build_blob(fr.unpadded(fr.model("sym3x3")))
    assert v1[4:8] == b"\x01\0\0\0" and len(fr.blob("sym3x3")) - len(v1) > 0


def test_importer_takes_padded_sources_and_refuses_the_rest():
    """Importing a padded network raised CubeImportError before pads were supported; now only these do."""
    for name in fr.ZOO:
        m = cube_import.read_blob(fr.blob(name))
        assert any(any(L["cpad"]) for L in fh.conv_records(m))
    in_shape, conv = (6, 5, 1), ("conv", 3, (3, 3), (1, 1), (2, 2), 1)
    tail = [("dense", 4), ("softmax",)]

    def refuse(spec, match, **kw):
        with pytest.raises(cube_import.CubeImportError, match=match):
            cube_synth.import_sources(*cube_synth.cube_sources(in_shape, [spec] + tail, **kw))

    refuse(conv + ((3, 1, 0, 1), fh.Z4), "layer_0: conv pad .* must be smaller than the 3x3 kernel")
    refuse(conv + ((1, 3, 1, 0), fh.Z4), "layer_0: conv pad")
    refuse(conv + ((1, 1, 1, 1), (2, 0, 0, 0)), "layer_0: pool pad .* must be smaller than the 2x2 pool")
    refuse(conv + ((1, 1, 1, 1), (0, 0, 1, 1)), "layer_0: declared output \\(4, 4, 3\\) does not match the computed \\(3, 3, 3\\)", declared={0: (4, 4)})
    # swapped axes: pads (2, 0, 0, 0) read as (0, 2, 0, 0) give another shape, which the declared tensor catches
    net_c, data_c = cube_synth.cube_sources(in_shape, [conv + ((2, 0, 0, 0), fh.Z4)] + tail)
    swapped = net_c.replace(".filter_pad = AI_SHAPE_INIT(4, 0, 2, 0, 0)", ".filter_pad = AI_SHAPE_INIT(4, 2, 0, 0, 0)")
    assert swapped != net_c
    with pytest.raises(cube_import.CubeImportError, match="layer_0: declared output"):
        cube_synth.import_sources(swapped, data_c)
    # dilation stays refused
    with pytest.raises(cube_import.CubeImportError, match="layer_0: dilation"):
        cube_synth.import_sources(net_c.replace(".dilation = AI_SHAPE_2D_INIT(1, 1)", ".dilation = AI_SHAPE_2D_INIT(2, 1)"), data_c)


@pytest.mark.parametrize("name", list(fr.PAD_REFUSALS))
def test_refusal_code(name):
    build, code, _ = fr.PAD_REFUSALS[name]
    assert fpl.plan(build()) == dict(error=code)


def test_read_blob_refuses_version_3():
    with pytest.raises(cube_import.CubeImportError, match="version 3"):
        cube_import.read_blob(fr.PAD_REFUSALS["version3"][0]())


def test_an_absent_element_as_zero_changes_neg_no_relu():
    """What the row is for: with 0 in place of -inf every window that holds an absent element becomes 0."""
    m = fr.model("neg_no_relu")
    L = fh.conv_records(m)[0]
    x = fr.inputs("neg_no_relu", 3, 25)
    right, wrong = fh.layer(L, x), fh.layer(L, x, absent=0.0)
    assert (right < -30).all() and (wrong == 0).reshape(3, 3, 3, 4)[:, 0].all() and (wrong == 0).reshape(3, 3, 3, 4)[:, :, 0].all()
    assert np.array_equal(right.reshape(3, 3, 3, 4)[:, 1:, 1:], wrong.reshape(3, 3, 3, 4)[:, 1:, 1:])


def test_statistic_counts_present_rows_only():
    for name in ("pool22_odd", "pool41_lead", "neg_no_relu", "mid_pads_batch"):
        m, p = fr.model(name), fpl.plan(fr.blob(name))
        s = fh.stats(m, fr.inputs(name, 2, p["in_n"]))
        assert s["count"].tolist() == [2 * p["in_n"]] + [2 * L["live"] * L["out_c"] for L in p["layers"]]
        assert (s["hist"].sum(axis=1) == s["count"]).all()
    # a truncating pool: the rows it drops are not computed, so not counted (9 conv columns, pool (1, 2): 8 of them), with and without pad keys
    m = fh.load(fr.blob("pool12_trunc_w"))
    bare = dict(m, layers=[{k: v for k, v in L.items() if k not in ("cpad", "ppad")} for L in m["layers"]])
    x = fr.inputs("pool12_trunc_w", 3, 66)
    a, b = fh.stats(bare, x), fh.stats(m, x)
    assert all(np.array_equal(a[k], b[k]) for k in a) and a["count"].tolist() == [3 * 66, 3 * 4 * 8 * 5, 3 * 3]


# ---- NNoM's PADDING_SAME ----------------------------------------------------------------------------------------------------------------
def _quantize(name):
    m = fr.model(name)
    x = fr.inputs(name, 4, int(np.prod(m["in_shape"])))
    return qz.quantize(m, fh.stats(m, x))


def test_nnom_rule_accepts():
    from edison_amd import nnom_import
    _, rep = _quantize("sym3x3")
    assert [L["same"] for L in rep["graph"] if L["type"] == nnom_import.T_CONV] == [1]
    blob, rep = _quantize("medium_embedding_conv")
    assert [(L["type"], L["same"]) for L in rep["graph"] if "same" in L] == [(nnom_import.T_CONV, 1), (nnom_import.T_POOL, 1), (nnom_import.T_CONV, 1)]
    text = qz.write_weights_h(rep["graph"], rep["in_shape"], rep["input"]["dec"])
    assert text.count("PADDING_SAME") == 3 and "PADDING_VALID" not in text
    assert nnom_import.build_blob(*nnom_import.parse_weights_h(text)) == blob
    _, rep = _quantize("simple_conv")                                                  # 'same' conv, 'valid' pool
    assert [L["same"] for L in rep["graph"] if "same" in L] == [1, 0]


@pytest.mark.parametrize("name,layer", [("stride2_same", "conv2d_1"), ("top_only", "conv2d_1"), ("tiny_embedding_conv", "conv2d_2"),
                                        ("k_wider_than_input", "conv2d_1")])
def test_nnom_rule_refuses_by_layer_name(name, layer):
    with pytest.raises(qz.QuantizeError, match="^%s: its (conv|pool) pads .*NNoM" % layer) as e:
        _quantize(name)
    m = fr.model(name)
    rec = fh.conv_records(m)[int(layer[-1]) - 1]
    assert str(rec["cpad"]) in str(e.value) or str(rec["ppad"]) in str(e.value)

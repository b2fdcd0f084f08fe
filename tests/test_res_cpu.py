"""CPU tests of the branching graphs: the importer's wiring and refusals, the blob's source table, the numpy restatement
(tests/res_ref.py) against tests/golden/res_golden.npz bit for bit, and that nothing sequential changed its bytes."""
import hashlib
import os
import struct

import numpy as np
import pytest

import res_ref
from edison_amd import nnom_import as imp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
NAMES = ["kws", "edges", "cat", "pool", "cat2"]

# sha256 of the blobs of the three DS-CNN headers and of the shipped blob on the commit before branching graphs were added
OLD_BLOBS = {
    "dscnn_kws": "4f741e33b530413bb73e612e24fa53d153aa8116505f290bea13d97b6e1566e9",
    "dscnn_edges": "3eae59b2065150c912e9be71086910dce608970fef5d99ba737150764becb97c",
    "dscnn_square": "be4fe752ea5e479b636f6600b075943b5026640c71d21fe1a76aadcd8d7cfb12",
}
SHIPPED = "b4fe789c79f4aa3329a4b93effe106b82146cea8be6c4e95c0f5d17cf3d870d5"


def _text(name):
    with open(os.path.join(GOLDEN, "alt_models", name + ".h")) as f:
        return f.read()


def _blob_of(text):
    shape, layers = imp.parse_weights_h(text)
    return imp.build_blob(shape, layers)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "res_golden.npz"))


@pytest.fixture(scope="module")
def blobs():
    return {n: _blob_of(_text("res_" + n)) for n in NAMES}


def test_sequential_blobs_keep_their_bytes():
    for name, sha in OLD_BLOBS.items():
        blob = _blob_of(_text(name))
        assert hashlib.sha256(blob).hexdigest() == sha, name
        assert struct.unpack_from("<8i", blob, 8)[6] == 0          # no source table
    with open(os.path.join(ROOT, "edison_amd", "data", "kws_nnom.ednn"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == SHIPPED


def test_source_table_states_the_wiring(blobs):
    assert imp.blob_sources(blobs["kws"]) == [[-1], [0], [1], [2, 0], [3], [4], [5], [6, 4], [7], [8], [9]]
    assert imp.blob_sources(blobs["edges"]) == [[-1], [0], [1], [2, 0], [3, 0, 2], [4, 4], [5], [6], [7, 6], [8, 6], [9], [10]]
    assert imp.blob_sources(blobs["cat"]) == [[-1], [0], [0], [0], [1, 2, 3], [4], [4, 5], [6], [7], [8]]
    assert imp.blob_sources(blobs["pool"]) == [[-1], [0], [0], [2], [1], [3, 4], [5]]
    assert imp.blob_sources(blobs["cat2"]) == [[-1], [0], [0], [1, 2], [3], [3, 4], [5], [6, 5], [7], [8]]
    for name in NAMES:
        assert res_ref.sources(blobs[name]) == imp.blob_sources(blobs[name])
        _, recs, _ = res_ref.net_ref.parse_blob(blobs[name])
        for v, s in zip(recs, imp.blob_sources(blobs[name])):
            if v[0] in (7, 8, 9, 10):
                assert v[11] == len(s)
    _, recs, _ = res_ref.net_ref.parse_blob(blobs["edges"])
    assert [(v[0], v[7], v[8] & 1) for v in recs if v[0] in (7, 8, 9)] == [(8, 1, 0), (7, 2, 1), (9, 5, 0), (9, 0, 0), (8, 0, 0)]
    _, recs, _ = res_ref.net_ref.parse_blob(blobs["cat"])
    assert [(v[0], v[1], v[8] & 1) for v in recs if v[0] == 10] == [(10, 15, 0), (10, 30, 1)]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_golden_vectors_at_every_layer(name, blobs, golden):
    r = res_ref.run(blobs[name], golden["in_" + name])
    off = 0
    for i, a in enumerate(r["acts"]):
        assert np.array_equal(a, golden["acts_" + name][:, off:off + a.shape[1]]), "record %d" % i
        off += a.shape[1]
    assert off == golden["acts_" + name].shape[1]
    assert np.array_equal(r["argmax"], golden["argmax_" + name])
    assert golden["in_" + name].shape[0] >= 24


@pytest.mark.parametrize("wrong,name", [("truncate", "edges"), ("mult_no_q7", "edges"), ("add_wide", "edges"), ("sub_swapped", "edges"),
                                        ("concat_planar", "cat")])
def test_wrong_variants_are_caught(wrong, name, blobs, golden):
    r = res_ref.run(blobs[name], golden["in_" + name], wrong=wrong)
    assert not np.array_equal(np.concatenate(r["acts"], axis=1), golden["acts_" + name]), wrong


def _swap(text, old, new):
    assert old in text
    return text.replace(old, new, 1)


REFUSALS = [
    ("third input to Sub", lambda: _swap(_text("res_edges"), "model.merge(Sub(SUB_1_OUTPUT_SHIFT), layer[3], layer[1])",
                                         "model.mergex(Sub(SUB_1_OUTPUT_SHIFT), 3, layer[3], layer[1], layer[2])"), "Sub"),
    ("third input to Mult", lambda: _swap(_text("res_edges"), "model.merge(Mult(MULT_1_OUTPUT_SHIFT), layer[6], layer[6])",
                                          "model.mergex(Mult(MULT_1_OUTPUT_SHIFT), 3, layer[6], layer[6], layer[1])"), "Mult"),
    ("Concat on another axis", lambda: _swap(_text("res_cat"), "Concat(-1)", "Concat(1)"), "Concat"),
    ("unequal shapes", lambda: _swap(_text("res_edges"), "model.merge(Sub(SUB_1_OUTPUT_SHIFT), layer[3], layer[1])",
                                     "model.merge(Sub(SUB_1_OUTPUT_SHIFT), layer[3], layer[0])"), "Sub"),
    ("unequal Concat channels", lambda: _swap(_text("res_cat"), "model.mergex(Concat(-1), 3, layer[3], layer[4], layer[5])",
                                              "model.mergex(Concat(-1), 3, layer[3], layer[4], layer[0])"), "Concat"),
    ("forward source", lambda: _swap(_text("res_edges"), "model.merge(Sub(SUB_1_OUTPUT_SHIFT), layer[3], layer[1])",
                                     "model.merge(Sub(SUB_1_OUTPUT_SHIFT), layer[3], layer[9])"), "Sub"),
    ("unread layer", lambda: _swap(_text("res_kws"), "model.merge(Add(ADD_1_OUTPUT_SHIFT), layer[4], layer[1])",
                                   "model.merge(Add(ADD_1_OUTPUT_SHIFT), layer[1], layer[1])"), "nothing reads"),
    # the Output hooks the Dense, not the Softmax behind it: the last record would be answered in the Dense's name
    ("unread last layer", lambda: _swap(_text("res_kws"), "nnom_output_data), layer[15])", "nnom_output_data), layer[14])"), "nothing reads"),
]


@pytest.mark.parametrize("what,text_of,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_importer_refusals_name_the_layer(what, text_of, word):
    with pytest.raises(ValueError) as e:
        _blob_of(text_of())
    assert word in str(e.value), what


@pytest.mark.parametrize("layer", ["GlobalAvgPool()", "GlobalMaxPool()", "SumPool(kernel(2, 2), stride(2, 2), PADDING_VALID)",
                                   "ZeroPadding(border(1, 1, 1, 1))"])
def test_layers_refused_before_stay_refused(layer):
    text = _swap(_text("res_kws"), "MaxPool(kernel(2, 2), stride(2, 2), PADDING_VALID)", layer)
    with pytest.raises(ValueError) as e:
        imp.parse_weights_h(text)
    assert layer.split("(")[0] in str(e.value)


def test_build_blob_refuses_a_source_that_does_not_point_backwards(blobs):
    shape, layers = imp.parse_weights_h(_text("res_kws"))
    layers[3]["src"] = [2, 5]
    with pytest.raises(ValueError) as e:
        imp.build_blob(shape, layers)
    assert "backwards" in str(e.value)


def _check_slice(blob):
    """A fused plan's passes against the wave's LDS slice: every image inside it, nothing stored into the expansion buffer, and no pass
    storing over a tensor that this pass or a later one still reads. A tensor lies where the pass that stored it (li_out) put it."""
    import plan_emulator
    P = plan_emulator.Plan(blob)
    M = P.M
    hold = M.hold_bytes
    assert M.ok and hold > 0 and hold % 16 == 0
    assert M.lds_bytes == M.tbl_bytes + M.frag_lds + M.waves * (2 * M.buf_bytes + M.x_bytes + hold) <= 160 * 1024
    slice_bytes = 2 * M.buf_bytes + M.x_bytes + hold
    src = res_ref.sources(blob)
    where = {}                                                  # tensor -> (first byte, end) in the slice, once stored
    for i, R in enumerate(P.R):
        if R.kind == 0:                                         # a MaxPool fused into the convolution in front: no pass of its own
            continue
        assert 0 <= R.in_off and R.in_off + M.batch * R.in_img <= slice_bytes
        assert 0 <= R.o_off and R.o_off + M.batch * R.o_img <= slice_bytes
        assert not (2 * M.buf_bytes <= R.o_off < 2 * M.buf_bytes + M.x_bytes)
        lo, hi = R.o_off, R.o_off + M.batch * R.o_img
        for t, (a, b) in where.items():
            if any(t in src[j] for j in range(i, len(src))):    # read by this pass or behind it
                assert b <= lo or hi <= a, "pass %d stores at %d..%d over tensor %d at %d..%d" % (i, lo, hi, t, a, b)
        for t in src[i]:
            assert t < 0 or t in where, "pass %d reads tensor %d, which no pass stored" % (i, t)
        where[R.li_out] = (lo, hi)
    return P


def test_fused_planner_holds_the_skips_and_declines_the_inception_stem(blobs):
    """ed_plan_net_mm through edison_net_plan_dump: the two residual graphs get a fused plan with merge passes (ED_RUN_MERGE = 7), held
    areas counted in lds_bytes, and every pass's images inside the wave's slice; `cat` has none -- its stem is read by a 1x1 convolution,
    a zero-padded 3x3 convolution and a pool, which want different LDS layouts of one tensor -- and stays layer by layer."""
    import plan_emulator
    from edison_amd import _lib
    for name in ("kws", "edges"):
        P = _check_slice(blobs[name])
        recs = res_ref.net_ref.parse_blob(blobs[name])[1]
        kinds = [R.kind for R in P.R]
        assert [k == 7 for k in kinds] == [v[0] in (7, 8, 9) for v in recs], kinds
    with pytest.raises(_lib.EdisonError):
        plan_emulator.Plan(blobs["cat"])


def test_a_fused_pool_output_does_not_share_with_what_its_convolution_reads(blobs):
    """`pool`: record 2's convolution fuses the MaxPool behind it (kind 0: no pass for record 3) and stores the pooled record 3 while it
    reads record 0, whose last reader it is. Both are held: their areas must be disjoint, like those of everything else alive."""
    P = _check_slice(blobs["pool"])
    assert [R.kind for R in P.R] == [1, 1, 1, 0, 2, 7, 1]
    assert P.R[2].li_out == 3 and P.R[2].in_off == P.R[1].in_off      # both convolutions read the held stem
    a, b = P.R[2].in_off, P.R[2].in_off + P.M.batch * P.R[2].in_img
    assert P.R[2].o_off >= b or P.R[2].o_off + P.M.batch * P.R[2].o_img <= a
    assert P.M.batch >= 2                                              # the merge pass runs over several images of a wave


def test_concat_of_agreeing_branches_takes_the_fused_kernel(blobs):
    """`cat2`: two 1x1 convolutions read the stem in one layout, so the graph has a fused plan: both Concats are ED_RUN_CAT passes (8),
    the Mult an ED_RUN_MERGE pass, with more than one input per wave."""
    P = _check_slice(blobs["cat2"])
    assert [R.kind for R in P.R] == [1, 1, 1, 8, 1, 8, 1, 7, 1, 4]
    assert P.M.batch >= 2

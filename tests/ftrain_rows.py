"""The data of the float32 trainer's suites, one section per suite: the rows, their models, blobs and inputs, the
shared float64 references, the synthetic sets of the fit tests. Test infrastructure, not a test. The mathematics is
tests/ftrain_ref.py's, the dropout mask tests/fdrop_ref.py's."""
import os

import numpy as np

from edison_amd import cube_import, train

import fdrop_ref
import fnet_rows
import ftrain_ref
from fnet_host import conv_records

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_ROWS = 17                      # rows of a gradient check: two tiles at a batch of 16, the second of one row


def _labels(model, n):
    return (np.arange(n) % int(np.prod(conv_records(model)[-1]["out"]))).astype(np.int32)


# ---- the fit tests (test_gpu_ftrain, _pad, _dropout, _bn, _data and their CPU suites) ---------------------------------------------------
FIT_ROW, PAD_FIT_ROW, FIT_CLASSES, FIT_ROWS = "pool21_trunc_h", "stride2_same", 3, 96
FIT_STEPS, FIT_BATCH, FIT_LR = 40, 32, 0.01


def fit_set():
    """Three classes on pool21_trunc_h's input shape: a fixed N(0, 1) pattern per class + N(0, 0.3), 96 rows, labels i % 3."""
    return ftrain_ref.class_set(int(np.prod(fnet_rows.model(FIT_ROW)["in_shape"])), FIT_CLASSES, FIT_ROWS, 2024)


def pad_fit_set():
    """fit_set on stride2_same's input shape (its dense layer has 3 outputs)."""
    return ftrain_ref.class_set(int(np.prod(fnet_rows.PAD[PAD_FIT_ROW][0]["in_shape"])), FIT_CLASSES, FIT_ROWS, 2025)


# the from-scratch fit tests (test_ftrain_zoo_cpu in float64, test_gpu_ftrain_data on the GPU): the architecture and the steps at which
# the float64 host trainer meets test_fit_learns_the_synthetic_set's conditions on fit_set()
SCRATCH_ARCH, SCRATCH_STEPS = "single_fc", FIT_STEPS


def scratch_model():
    return train.get_model(SCRATCH_ARCH, fnet_rows.model(FIT_ROW)["in_shape"], FIT_CLASSES)


def kws_set(in_n=403, classes=10, rows=96):
    """The same for `kws train` on a zoo network at 31 x 13 x 1: ten classes, 96 rows."""
    return ftrain_ref.class_set(in_n, classes, rows, 2026)


# ---- padded networks (test_fgrad_pad_cpu, test_gpu_ftrain_pad) ------------------------------------------------------------------------
NEG_T = "neg_no_relu_t"          # fnet_rows.PAD's neg_no_relu with a bias that does not saturate the softmax
PAD_ROWS = [NEG_T if name == "neg_no_relu" else name for name in fnet_rows.PAD]
ALL_N = ("sym3x3", "pool41_lead", "mid_pads_batch")      # rows the GPU test also runs at n = 1, b - 1, b, b + 1 and 3 b + 2 for the trainer's batch b
_MODELS = {}


def n_max(name):
    """The most rows of row `name` a gradient check draws: 3 x 16 + 2 on the ALL_N rows (mid_pads_batch trains at batch 5: 17)."""
    return 3 * 16 + 2 if name in ALL_N else N_ROWS


def pad_model(name):
    """fnet_rows.model; neg_no_relu_t: neg_no_relu's layers and pads with bias -3 and positive weights in every record."""
    if name not in _MODELS:
        if name == NEG_T:
            spec = fnet_rows.PAD["neg_no_relu"][0]
            _MODELS[name] = fnet_rows.seeded(fnet_rows.network(spec["in_shape"], spec["layers"]), 2000 + fnet_rows._seed(name), positive=True, bias=-3.0)
        else:
            _MODELS[name] = fnet_rows.model(name)
    return _MODELS[name]


def pad_blob(name):
    return cube_import.build_blob(pad_model(name)) if name == NEG_T else fnet_rows.blob(name)


def pad_data(name, n=N_ROWS):
    """(x [n][in_n] float32, labels i % n_out) of row `name`: N(0, 1); neg_no_relu_t: -|N(0, 1)| - 0.1, every input negative."""
    m = pad_model(name)
    in_n = int(np.prod(m["in_shape"]))
    x = np.random.default_rng(5000 + fnet_rows._seed(name)).normal(0, 1, (n, in_n)).astype(np.float32)
    if name == NEG_T:
        x = (-np.abs(x) - np.float32(0.1)).astype(np.float32)
    return x, _labels(m, n)


# ---- dropout (test_fdrop_cpu, test_gpu_ftrain_dropout) --------------------------------------------------------------------------------
SHIPPED = "cube_kws"
# name -> (source: "sweep" (fnet_rows), "pad" (PAD_ROWS) or "shipped", the row there, dropout, seed of the masks)
DROP_ROWS = {
    "p1_inc3": ("sweep", "inc3_oc64_oc65_s21", None, 11),                       # P = 1 everywhere: the two positions coincide
    "p2_pool12_no_relu_before": ("sweep", "pool12_trunc_w", [(0.25, 1), 0], 12),   # P = 2 without ReLU: the dropped-winner bit decides
    "p4_pool22_before": ("sweep", "pool22_trunc_hw", [(0.5, 1), 0], 13),          # P = 4, 17 channels: two channel tiles
    "p4_pool22_after": ("sweep", "pool22_trunc_hw", [(0.25, 0), 0], 14),
    "pool21_before": ("sweep", "pool21_trunc_h", [(0.25, 1), 0], 15),
    "pool21_after": ("sweep", "pool21_trunc_h", [(0.5, 0), 0], 16),
    "neg_no_relu_before": ("pad", NEG_T, [(0.25, 1), 0], 17),
    "mid_pads_batch": ("pad", "mid_pads_batch", [0.25, 0.5, (0.25, 1), 0], 18),
    "simple_conv": ("pad", "simple_conv", train.KERAS_DROPOUT["simple_conv"], 19),
    "medium_embedding_conv": ("pad", "medium_embedding_conv", train.KERAS_DROPOUT["medium_embedding_conv"], 20),
    "batch5": ("sweep", "batch5", [0.25, (0.5, 1), 0], 21),
    "shipped_kws_conv": ("shipped", SHIPPED, train.KERAS_DROPOUT["kws_conv"], 116),   # a trained network is sure of itself: most seeds leave a probability below 1e-4
}
_DROP_CASES, _DROP_REFS = {}, {}


def drop_case(name):
    """Row `name` -> dict(model, blob, dropout, seed, x [17][in_n], y [17]), built once. The padded rows' inputs are pad_data's, the others' N(0, 1)."""
    if name in _DROP_CASES:
        return _DROP_CASES[name]
    kind, row, dropout, seed = DROP_ROWS[name]
    if kind == "pad":
        model, blob = pad_model(row), pad_blob(row)
        x, y = pad_data(row, N_ROWS)
    else:
        if kind == "shipped":
            with open(os.path.join(GOLDEN, "cube_kws.ednf"), "rb") as f:
                blob = f.read()
        else:
            blob = fnet_rows.blob(row)
        model = cube_import.read_blob(blob)
        # N(0, 1), as pad_data draws: fnet_rows' own input sets and the shipped network's features saturate the softmax
        x = np.random.default_rng(6000 + seed).normal(0, 1, (N_ROWS, int(np.prod(model["in_shape"])))).astype(np.float32)
        y = _labels(model, N_ROWS)
    if dropout is None:                                                        # every record but the last, rates 0.25 and 0.5 in turn
        nl = len(conv_records(model))
        dropout = [(0.25, 0.5)[i % 2] for i in range(nl - 1)] + [0]
    _DROP_CASES[name] = dict(model=model, blob=blob, dropout=dropout, seed=seed, x=x, y=y, sp=fdrop_ref.spec(model, dropout))
    return _DROP_CASES[name]


def drop_reference(name, call=0):
    """ftrain_ref.loss_grad (float64, detail) of row `name` at counter `call`, computed once and shared."""
    if (name, call) not in _DROP_REFS:
        c = drop_case(name)
        _DROP_REFS[name, call] = ftrain_ref.loss_grad(c["model"], c["x"], c["y"], dropout=(c["sp"], c["seed"], call), detail=True)
    return _DROP_REFS[name, call]


# ---- BatchNorm (test_fbn_cpu, test_gpu_ftrain_bn) -------------------------------------------------------------------------------------
# name -> dict(in_shape, layers (fnet_rows._records' form), bn, dropout, n, seed: of the inputs, chosen so that test_fbn_cpu's bound
# precondition holds, bias0: added to record 0's bias, neg: gamma and beta set through set_bn_state)
BN_ROWS = {
    "bn_p1": dict(in_shape=(6, 5, 2), layers=[("conv", 5, (2, 2), (1, 1), (1, 1), 1), ("dense", 4, 0)], bn=[1, 0], seed=1),
    "bn_pool21_neg": dict(in_shape=(7, 5, 2), layers=[("conv", 17, (2, 2), (1, 1), (2, 1), 1), ("dense", 3, 0)], bn=[1, 0], neg=True, seed=1),
    "bn_trunc": dict(in_shape=(6, 5, 1), layers=[("conv", 6, (2, 2), (1, 1), (2, 2), 1), ("dense", 3, 0)], bn=[1, 0], seed=1),
    "bn_mixed": dict(in_shape=(12, 8, 1), layers=[("conv", 6, (3, 3), (1, 1), (2, 1), 1), ("conv", 8, (2, 2), (1, 1), (1, 1), 0),
                                                  ("conv", 5, (2, 2), (1, 1), (1, 1), 1), ("dense", 4, 0)], bn=[1, 0, 1, 0],
                     dropout=[(0.25, 1), 0, (0.25, 0), 0], seed=1),
    "bn_dense": dict(in_shape=(3, 4, 1), layers=[("dense", 6, 1), ("dense", 3, 0)], bn=[1, 0], n=2, seed=1),
    "bn_offset": dict(in_shape=(6, 5, 2), layers=[("conv", 5, (2, 2), (1, 1), (1, 1), 1), ("dense", 4, 0)], bn=[1, 0], bias0=30.0, seed=1, weights_of="bn_p1"),
    "shipped": dict(shipped=True, bn=train.KERAS_BATCHNORM["kws_conv"], dropout=train.KERAS_DROPOUT["kws_conv"], n=9, seed=1),
}
_BN_CASES, _BN_REFS = {}, {}


def bn_fresh_model(name):
    """The row's model dict with fresh weights: N(0, 1) / sqrt(K) and N(0, 0.1) biases, float32."""
    row = BN_ROWS[name]
    if row.get("shipped"):
        with open(os.path.join(GOLDEN, "cube_kws.ednf"), "rb") as f:
            shipped = cube_import.read_blob(f.read())
        in_shape = tuple(shipped["in_shape"])
        recs = [dict(L) for L in shipped["layers"]]
    else:
        in_shape = row["in_shape"]
        recs = fnet_rows.network(in_shape, row["layers"], pad_keys=False)["layers"]
    m = fnet_rows.seeded(dict(in_shape=in_shape, layers=recs), 4000 + sum(map(ord, row.get("weights_of", name))))
    first = conv_records(m)[0]
    first["b"] = (first["b"] + np.float32(row.get("bias0", 0.0))).astype(np.float32)
    return m


def bn_case(name):
    """Row `name` -> dict(model, blob, bn, dropout, sp, seed, x [n][in_n] N(0, 1), y, state0: the state the test starts from), built once."""
    if name in _BN_CASES:
        return _BN_CASES[name]
    row = BN_ROWS[name]
    model = bn_fresh_model(name)
    n = row.get("n", N_ROWS)
    rng = np.random.default_rng(7000 + 100 * row["seed"] + sum(map(ord, name)))
    x = rng.normal(0, 1, (n, int(np.prod(model["in_shape"])))).astype(np.float32)
    state0 = ftrain_ref.initial_state(model, row["bn"], np.float32)
    if row.get("neg"):                         # half the channels with a negative gamma: the pool's winner behind BatchNorm is not the one before it
        for st in state0:
            if st is not None:
                oc = len(st["gamma"])
                st["gamma"] = (np.where(np.arange(oc) % 2, -1.0, 1.0) * rng.uniform(0.5, 1.5, oc)).astype(np.float32)
                st["beta"] = rng.normal(0, 0.3, oc).astype(np.float32)
    dropout = row.get("dropout")
    _BN_CASES[name] = dict(model=model, blob=cube_import.build_blob(model), bn=list(row["bn"]), dropout=dropout,
                           sp=None if dropout is None else fdrop_ref.spec(model, dropout), seed=40 + row["seed"], x=x, y=_labels(model, n), state0=state0, n=n)
    return _BN_CASES[name]


def bn_state(name, call):
    """The state training call `call` of row `name` starts from: state0, or the one after the call before."""
    return bn_case(name)["state0"] if call == 0 else bn_reference(name, call - 1)[1]


def bn_reference(name, call=0):
    """(ftrain_ref.loss_grad in float64 of row `name` at training call `call` (0 or 1: two consecutive calls on unchanged weights), the
    state after it), computed once and shared."""
    if (name, call) not in _BN_REFS:
        c = bn_case(name)
        state = bn_state(name, call)
        r = ftrain_ref.loss_grad(c["model"], c["x"], c["y"], dropout=(c["sp"], c["seed"], call), bn=dict(state=state), detail=True)
        _BN_REFS[name, call] = (r, ftrain_ref.moved(state, r["bn"]))
    return _BN_REFS[name, call]


def bn_bounds(name, call):
    """ftrain_ref.bounds of row `name` at call `call`, computed once."""
    if ("bounds", name, call) not in _BN_REFS:
        c = bn_case(name)
        _BN_REFS["bounds", name, call] = ftrain_ref.bounds(c["model"], c["x"], c["y"], bn_reference(name, call)[0], dropout=(c["sp"], c["seed"], call),
                                                           bn=dict(state=bn_state(name, call)))
    return _BN_REFS["bounds", name, call]

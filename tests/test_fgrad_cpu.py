"""The float64 restatement of training (tests/ftrain_ref.py) held to torch's float64 autograd and to central differences, the packed
layout of edison_amd/train.py held to the plan's (fnet_plan.plan), the Adam restatement held to torch.optim.Adam, the host side
of fit: the shuffle and the two callbacks; and what tests/test_gpu_ftrain_tiles.py rests on: the order of a multi-tile call's sums
(ftrain_ref.fold_tiles), what that order is sensitive to, what the float64 bound sees at these sizes, and the trainer's batch
(ftrain_ref.train_batch). No GPU."""
import os

import numpy as np
import pytest

from edison_amd import cube_import, train

import fnet_host
import fnet_plan
import fnet_rows
import ftrain_ref
import ftrain_rows

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = ["ladder_k5", "pool21_trunc_h", "pool12_trunc_w", "pool22_trunc_hw", "pool41_tail", "inc3_oc64_oc65_s21", "oc40_s32_span_h", "n_out_210",
        "relu_logits", "conv_last_map", "layers16", "batch5", "dense16_wide", "synth_pool12_relu"]


def _case(name, n=5):
    if name == "cube_kws":
        model = fnet_host.load(os.path.join(HERE, "golden", "cube_kws.ednf"))
        g = np.load(os.path.join(HERE, "golden", "cube_golden.npz"))
        rows = np.stack([g[k] for k in sorted(g.files) if k.startswith("net_in_")]).astype(np.float32)
        x = rows[np.arange(n) % rows.shape[0]]
    else:
        model = fnet_rows.model(name)
        x = ftrain_ref.inputs(name, n, int(np.prod(model["in_shape"])))
    n_out = int(np.prod(fnet_host.conv_records(model)[-1]["out"]))
    return model, x, (np.arange(n) % n_out).astype(np.int32)


@pytest.mark.parametrize("name", ROWS + ["cube_kws"])
def test_agrees_with_torch_float64_autograd(name):
    import torch
    model, x, y = _case(name)
    ref = ftrain_ref.loss_grad(model, x, y)
    tor = ftrain_ref.torch_grads(model, x, y, torch.float64)
    assert np.allclose(ref["logits"], tor["logits"], rtol=1e-10, atol=1e-12)
    assert np.allclose(ref["loss"], tor["loss"], rtol=1e-10, atol=1e-12)
    for i, (a, b) in enumerate(zip(ref["grads"], tor["grads"])):
        for k in ("w", "b"):
            scale = max(np.abs(b[k]).max(), 1e-300)
            assert np.abs(a[k] - b[k]).max() <= 1e-10 * scale, (name, i, k, np.abs(a[k] - b[k]).max() / scale)


def test_inputs_leave_the_saturating_sets_out():
    x = ftrain_ref.inputs("pool21_trunc_h", 9, 66)
    assert x.shape == (9, 66) and np.abs(x).max() < 200          # n1, zero and neg (30 |g|) rows only
    assert (x[1] == 0).all() and (x[2] <= 0).all() and (x[4] == 0).all()


@pytest.mark.parametrize("name", ["ladder_k5", "pool21_trunc_h"])
def test_agrees_with_central_differences(name):
    model, x, y = _case(name, n=4)
    ref = ftrain_ref.loss_grad(model, x, y)
    base = [dict(w=np.asarray(L["w"], np.float64), b=np.asarray(L["b"], np.float64)) for L in fnet_host.conv_records(model)]
    h = 1e-6
    for i, t in enumerate(base):
        for k in ("w", "b"):
            num = np.zeros(t[k].size)
            for j in range(t[k].size):
                vals = []
                for sgn in (1.0, -1.0):
                    w = [dict(w=u["w"].copy(), b=u["b"].copy()) for u in base]
                    w[i][k].reshape(-1)[j] += sgn * h
                    vals.append(ftrain_ref.loss_grad(model, x, y, weights=w)["loss"].mean())
                num[j] = (vals[0] - vals[1]) / (2 * h)
            g = ref["grads"][i][k].reshape(-1)
            # the loss is smooth between the kinks of ReLU and max: a central difference errs by O(h^2) |f'''| + rounding / h
            assert np.abs(num - g).max() <= 1e-7 * max(np.abs(g).max(), 1.0), (name, i, k, np.abs(num - g).max())


def test_first_maximum_and_relu_at_zero():
    """One 1 x 2 pool window with a tie, under ReLU and without: the gradient goes to element 0, and a 0 / 0 tie under ReLU passes none."""
    def net(relu, bias):
        conv = dict(type=cube_import.T_CONV, inp=(1, 2, 1), out=(1, 1, 1), k=(1, 1), s=(1, 1), p=(1, 2), relu=relu,
                    w=np.ones((1, 1, 1, 1), np.float32), b=np.full(1, bias, np.float32))
        dense = dict(type=cube_import.T_CONV, inp=(1, 1, 1), out=(1, 1, 2), k=(1, 1), s=(1, 1), p=(1, 1), relu=0,
                     w=np.array([1.0, -1.0], np.float32).reshape(2, 1, 1, 1), b=np.zeros(2, np.float32))
        return dict(in_shape=(1, 2, 1), layers=[conv, dense, dict(type=cube_import.T_SOFTMAX, inp=(1, 1, 2), out=(1, 1, 2))])
    tie = ftrain_ref.loss_grad(net(0, 0.5), np.array([[2.0, 2.0]]), [0])["grads"][0]
    assert tie["w"].reshape(-1)[0] != 0                                    # x[0] = 2 reaches dW through element 0 ...
    one = ftrain_ref.loss_grad(net(0, 0.5), np.array([[2.0, 1.0]]), [0])["grads"][0]
    assert tie["w"].reshape(-1)[0] == one["w"].reshape(-1)[0]              # ... and element 1 adds nothing
    dead = ftrain_ref.loss_grad(net(1, 0.0), np.array([[0.0, 0.0]]), [0])["grads"][0]
    assert dead["w"].reshape(-1)[0] == 0 and dead["b"][0] == 0             # ReLU'(0) = 0


def _routed_dw(model, x, y, pick):
    """Record 0's dW of a tie_case network, restated with loops: each pool window's gradient to the element `pick` chooses among
    those equal to the window's maximum. Returns (dW, how often the first of several maxima was element e)."""
    conv, dense = fnet_host.conv_records(model)
    w, b = conv["w"].astype(np.float64), conv["b"].astype(np.float64)
    img = x.astype(np.float64).reshape(-1, 6, 6)
    n = len(img)
    ph, pw = conv["p"]
    Ph, Pw, oc = conv["out"]
    pre = np.array([[[[(img[u, r:r + 2, c:c + 2] * w[o, :, :, 0]).sum() + b[o] for o in range(oc)] for c in range(5)] for r in range(5)]
                    for u in range(n)])
    win = lambda u, py, px, o: [pre[u, py * ph + e // pw, px * pw + e % pw, o] for e in range(ph * pw)]
    pooled = np.array([[[[max(win(u, py, px, o)) for o in range(oc)] for px in range(Pw)] for py in range(Ph)] for u in range(n)])
    z = pooled.reshape(n, -1) @ dense["w"].astype(np.float64).reshape(3, -1).T + dense["b"]
    pz = np.exp(z - z.max(axis=1, keepdims=True))
    dz = (pz / pz.sum(axis=1, keepdims=True) - np.eye(3)[y]) / n
    dpooled = (dz @ dense["w"].astype(np.float64).reshape(3, -1)).reshape(pooled.shape)
    dw, tied_first = np.zeros_like(w), np.zeros(ph * pw, int)
    for u in range(n):
        for py in range(Ph):
            for px in range(Pw):
                for o in range(oc):
                    v = win(u, py, px, o)
                    at = [e for e in range(ph * pw) if v[e] == pooled[u, py, px, o]]
                    tied_first[at[0]] += len(at) > 1
                    e = pick(at)
                    r, c = py * ph + e // pw, px * pw + e % pw
                    dw[o, :, :, 0] += dpooled[u, py, px, o] * img[u, r:r + 2, c:c + 2]
    return dw, tied_first


@pytest.mark.parametrize("pool", ftrain_ref.TIE_POOLS, ids=lambda p: "pool%d%d" % p)
def test_tied_windows_send_the_gradient_to_their_first_element(pool):
    """The rows tests/test_gpu_ftrain.py holds the trainer's first-maximum choice to: windows tie exactly with their first maximum at
    every element that can tie, the restatement sends a tied window's gradient to its first maximum only, and the last maximum
    instead would move dW far beyond any rounding bound."""
    import torch
    model, x, y = ftrain_ref.tie_case(pool)
    assert fnet_host.conv_records(model)[0]["relu"] == 0
    ref = ftrain_ref.loss_grad(model, x, y)
    first, tied_first = _routed_dw(model, x, y, lambda at: at[0])
    assert (tied_first[:-1] > 0).all(), tied_first                          # a window's last element is never the first of several
    assert ftrain_ref.tensor_error(ref["grads"][0]["w"], first) <= 1e-12
    last, _ = _routed_dw(model, x, y, lambda at: at[-1])
    assert ftrain_ref.tensor_error(last, first) > 1e-2
    tor = ftrain_ref.torch_grads(model, x, y, torch.float64)
    for a, b in zip(ref["grads"], tor["grads"]):
        assert ftrain_ref.tensor_error(a["w"], b["w"]) <= 1e-10 and ftrain_ref.tensor_error(a["b"], b["b"]) <= 1e-10


@pytest.mark.parametrize("name", ["pool22_trunc_hw", "inc3_oc64_oc65_s21", "n_out_210", "ladder_k5"])
def test_pack_round_trip_against_the_plan(name):
    blob = fnet_rows.blob(name)
    model, plan = cube_import.read_blob(blob), fnet_plan.plan(blob)
    lay, n = train.layout(model)
    at = 0
    for r, L in zip(lay, plan["layers"]):
        assert (r["w_at"], r["K"], r["k_pad"], r["out_c"], r["n_pad"]) == (at, L["K"], L["k_pad"], L["out_c"], L["n_pad"])
        at += L["k_pad"] * L["n_pad"] + L["n_pad"]
    assert n == at
    payload = np.frombuffer(blob, "<f4", n, len(blob) - 4 * n)            # the blob's weights are the packed array
    tensors = train.unpack(payload, lay)
    for t, L in zip(tensors, fnet_host.conv_records(model)):
        assert np.array_equal(t["w"], L["w"]) and np.array_equal(t["b"], L["b"])
    assert np.array_equal(train.pack(tensors, lay), payload)
    marked = np.where(payload == 0, np.float32(1e6), payload)             # the padding is kept from `base`, the real entries replaced
    again = train.pack(tensors, lay, base=marked)
    real = train.pack([dict(w=np.ones_like(t["w"]), b=np.ones_like(t["b"])) for t in tensors], lay) != 0
    assert np.array_equal(again[real], payload[real]) and np.array_equal(again[~real], marked[~real])
    with pytest.raises(ValueError):
        train.pack(tensors[:-1] + [dict(w=tensors[-1]["w"][..., None], b=tensors[-1]["b"])], lay)


# ---- the order of a multi-tile call's sums, and the trainer's batch ---------------------------------------------------------------
FOLD_ROW, FOLD_TILES, FOLD_ROWS, FOLD_GRID = "pool21_trunc_h", 40, 16, 16


@pytest.fixture(scope="module")
def fold_case():
    """(model, layout, x, y, the whole batch's float64 gradient, T [40][w_floats]: each tile's float64 gradient of the batch loss, cast)."""
    n = FOLD_TILES * FOLD_ROWS
    model, x, y = _case(FOLD_ROW, n)
    lay, w = train.layout(model)
    whole = ftrain_ref.loss_grad(model, x, y)
    T = np.stack([train.pack(ftrain_ref.loss_grad(model, x[j:j + FOLD_ROWS], y[j:j + FOLD_ROWS], n_total=n)["grads"], lay)
                  for j in range(0, n, FOLD_ROWS)])
    assert T.shape == (FOLD_TILES, w) and T.dtype == np.float32
    return model, lay, x, y, whole, T


def test_fold_tiles_sums_a_batch_within_the_bound(fold_case):
    """Per-tile float64 gradients rounded to float32 and folded in the kernels' order: the whole batch's gradient within the GPU
    tests' bound (ftrain_ref.bounds)."""
    model, lay, x, y, whole, T = fold_case
    got = train.unpack(ftrain_ref.fold_tiles(T, FOLD_GRID, 1.0), lay)
    per = ftrain_ref.bounds(model, x, y, whole)[0]
    for g, g64, allowed in zip(got, whole["grads"], per):
        for k in ("w", "b"):
            bound = allowed[k][0]
            err = ftrain_ref.tensor_error(g[k], g64[k])
            print("%s: %.3g (bound %.3g)" % (k, err, bound))
            assert err <= bound
    one = ftrain_ref.fold_tiles(T[:3], FOLD_GRID, 1.0)                       # fewer tiles than workgroups: three slabs of one tile
    assert np.array_equal(one, (T[0] + T[1]) + T[2])
    with pytest.raises(AssertionError):
        ftrain_ref.fold_tiles(T, FOLD_GRID, 3.0)
    with pytest.raises(AssertionError):
        ftrain_ref.fold_tiles(T.astype(np.float64), FOLD_GRID, 1.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fold_tiles_sees_a_swapped_tile_and_a_flat_chain(fold_case):
    """What the exact GPU check (tests/test_gpu_ftrain_tiles.py) relies on: the folded bits change when two tiles of different
    workgroups change places, when a workgroup's tiles are taken in another order than its slab adds them, and when all tiles are
    summed in one chain; a power-of-two scale changes nothing."""
    T = fold_case[5]
    want = ftrain_ref.fold_tiles(T, FOLD_GRID, 1.0)
    swapped = T.copy()
    swapped[[3, FOLD_GRID + 4]] = T[[FOLD_GRID + 4, 3]]                      # workgroup 3's first tile and workgroup 4's second
    assert not np.array_equal(_bits(ftrain_ref.fold_tiles(swapped, FOLD_GRID, 1.0)), _bits(want))
    flat = T[0].copy()
    for j in range(1, len(T)):
        flat += T[j]
    assert not np.array_equal(_bits(flat), _bits(want))
    assert not np.array_equal(_bits(ftrain_ref.fold_tiles(T, len(T), 1.0)), _bits(want))     # one tile per workgroup: the flat chain again
    assert np.array_equal(_bits(ftrain_ref.fold_tiles(T, len(T), 1.0)), _bits(flat))
    assert not np.array_equal(_bits(ftrain_ref.fold_tiles(T, FOLD_GRID // 2, 1.0)), _bits(want))   # another grid: another order
    # the power-of-two argument on the host
    assert np.array_equal(_bits(ftrain_ref.fold_tiles(T * np.float32(2.0 ** 9), FOLD_GRID, 2.0 ** -9)), _bits(want))


def test_a_lost_tile_moves_every_tensor_by_more_than_the_bound():
    """pool21_trunc_h at n = 8 229 on a grid of 256 workgroups of 16 rows: without workgroup 0's second tile (rows 4 096 .. 4 111)
    every tensor of the float64 gradient moves by more than the GPU tests' bound (the inputs were chosen so: the lowest ratio is
    record 0's bias, 9). A wrong row inside a tile or another order of the sum is far below it: the exact check is for those."""
    n, b, grid = 8229, 16, 256
    model, x, y = _case(FOLD_ROW, n)
    whole = ftrain_ref.loss_grad(model, x, y)
    rows = slice(grid * b, grid * b + b)
    lost = ftrain_ref.loss_grad(model, x[rows], y[rows], n_total=n)["grads"]
    per = ftrain_ref.bounds(model, x, y, whole)[0]
    ratios = []
    for i, (g64, t, allowed) in enumerate(zip(whole["grads"], lost, per)):
        for k in ("w", "b"):
            bound = allowed[k][0]
            moved = ftrain_ref.tensor_error(g64[k] - t[k], g64[k])
            print("record %d %s: moved %.3g, bound %.3g, ratio %.1f" % (i, k, moved, bound, moved / bound))
            ratios.append(moved / bound)
    assert min(ratios) > 1.0, ratios


def _plans():
    out = {name: fnet_plan.plan(fnet_rows.blob(name)) for name in fnet_rows.SWEEP}
    with open(os.path.join(HERE, "golden", "cube_kws.ednf"), "rb") as f:
        out["cube_kws"] = fnet_plan.plan(f.read())
    return out


def test_train_batch_is_the_networks_except_where_dy_does_not_fit():
    """ftrain_ref.train_batch (ftrain_size_lds and edison_ftrain_create's lowering loop restated) on every sweep row and the shipped
    network: only batch5 trains below its forward batch, at 2 of 5 -- dY of its first record, 1 064 rows x 16 padded channels an
    utterance, is 144 704 bytes with its row bases at 2 utterances and over the limit at 3."""
    plans = _plans()
    for name, p in plans.items():
        tb = ftrain_ref.train_batch(p)
        assert 1 <= tb <= p["batch"] and ftrain_ref.train_lds_bytes(p, tb) <= fnet_plan.LDS_BYTES, name
        assert tb == (2 if name == "batch5" else p["batch"]), (name, tb, p["batch"])
    assert plans["batch5"]["batch"] == 5 and ftrain_ref.train_batch(plans["cube_kws"]) == 7
    p = plans["batch5"]
    assert p["layers"][0]["rows"] == 1064 and p["layers"][0]["n_pad"] == 16
    assert ftrain_ref.train_lds_bytes(p, 2) == 4 * 2128 * 16 + 4 * 2128 == 144704
    assert ftrain_ref.train_lds_bytes(p, 3) > fnet_plan.LDS_BYTES
    # where the forward half is the larger one the bytes are the forward plan's: the shipped network's 159 808
    assert ftrain_ref.train_lds_bytes(plans["cube_kws"], 7) == plans["cube_kws"]["lds_bytes"] == 159808
    # a plan whose one utterance does not fit is refused (0), and a limit between two batches lowers by one
    assert ftrain_ref.train_batch(p, limit=ftrain_ref.train_lds_bytes(p, 1) - 1) == 0
    assert ftrain_ref.train_batch(p, limit=ftrain_ref.train_lds_bytes(p, 1)) == 1
    # the new sweep row: forward batch 10, more packed floats than one pass of the step kernel covers on 256 CUs
    wide = plans["dense16_wide"]
    assert (wide["batch"], wide["n_layers"], fnet_rows.w_floats(wide)) == (10, 16, 558928) and 558928 > fnet_rows.STEP_PASS * 256


def test_adam_restatement_against_torch():
    import torch
    rng = np.random.default_rng(5)
    w0 = [rng.normal(0, 1, (4, 3)), rng.normal(0, 1, 7)]
    ws = [w.copy() for w in w0]
    tw = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in w0]
    opt = torch.optim.Adam(tw, lr=0.0005, betas=(0.9, 0.999), eps=1e-7)
    adam = ftrain_ref.Adam()
    for step in range(5):
        gs = [rng.choice([-1.0, 1.0], w.shape) * rng.uniform(0.5, 2.0, w.shape) for w in w0]
        for t, g in zip(tw, gs):
            t.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        adam.step(ws, gs, 0.0005)
        for a, t in zip(ws, tw):
            # torch puts eps beside sqrt(v) / sqrt(1 - b2^t), Keras beside sqrt(v): the denominators differ by less than eps. With
            # |g| >= 0.5, sqrt(v) >= sqrt(0.001) 0.5 = 0.0158, so an update differs by at most 1e-7 / 0.0158 of itself, and an
            # update is at most lr (1 - b1) / sqrt(1 - b2) = 3.2 lr: 5 steps x 3.2 lr x 6.4e-6
            assert np.abs(a - t.detach().numpy()).max() <= 5 * 3.2 * 0.0005 * 6.4e-6, step
    assert adam.t == 5


def test_adam_first_step_is_lr_sized():
    adam = ftrain_ref.Adam()
    w = [np.array([1.0, -2.0, 3.0])]
    adam.step(w, [np.array([0.5, -4.0, 0.0])], 0.01)
    assert np.allclose(w[0], [1.0 - 0.01, -2.0 + 0.01, 3.0], atol=1e-7)  # m / sqrt(v) = sign(g) after bias correction


def test_shuffle_is_reproducible_from_the_seed():
    a, b = train.epoch_order(96, 0, 3), train.epoch_order(96, 0, 3)
    assert np.array_equal(a, b) and np.array_equal(np.sort(a), np.arange(96))
    assert not np.array_equal(a, train.epoch_order(96, 0, 4)) and not np.array_equal(a, train.epoch_order(96, 1, 3))


class _Scripted:
    """A trainer whose losses follow a script: fit's bookkeeping without a network."""

    def __init__(self, val_losses, n_train):
        self.val, self.n_train, self.lrs, self.batches, self.epoch = list(val_losses), n_train, [], [], 0

    def grad(self, x, y):
        if x.shape[1] == 2:                                               # the validation set is marked by its width
            loss = np.full(len(y), self.val[self.epoch], np.float32)
            self.epoch += 1
        else:
            self.batches.append(x[:, 0].astype(int).tolist())
            loss = np.full(len(y), 1.0, np.float32)
        return dict(loss=loss, argmax=np.zeros(len(y), np.int32))

    def step(self, lr):
        self.lrs.append(lr)


def test_fit_batches_history_and_callbacks():
    n = 7
    x = np.arange(n, dtype=np.float32).reshape(n, 1)
    y = np.zeros(n, np.int32)
    val = (np.zeros((3, 2), np.float32), np.array([0, 1, 0]))
    # improves, stalls (lr halves after one epoch without a gain above 1e-4), improves, then never again: stopped after 10 such epochs
    script = [1.0, 1.0, 0.5, 0.49995] + [0.6] * 20
    tr = _Scripted(script, n)
    hist = train.fit(tr, x, y, epochs=50, batch_size=3, val=val, seed=4, lr=0.01)
    assert [len(b) for b in tr.batches[:3]] == [3, 3, 1]                  # the last batch is short
    assert sorted(sum(tr.batches[:3], [])) == list(range(n)) and sum(tr.batches[:3], []) == train.epoch_order(n, 4, 0).tolist()
    assert hist["val_loss"][:4] == pytest.approx(script[:4]) and hist["loss"][0] == pytest.approx(1.0)
    assert hist["acc"][0] == 1.0 and hist["val_acc"][0] == pytest.approx(2 / 3)
    # epoch 1 stalls -> epoch 2 runs at 0.005; epoch 2 improves; epoch 3 gains under min_delta -> 0.0025; then a halving per epoch
    assert hist["lr"][:6] == pytest.approx([0.01, 0.01, 0.005, 0.005, 0.0025, 0.00125])
    assert hist["stopped_early"] and len(hist["val_loss"]) == 4 + 10     # best 0.49995 at epoch 3, ten epochs without a better one
    assert hist["steps"] == 3 * 14 and len(tr.lrs) == 42
    # without a validation set the callbacks have nothing to watch; max_steps ends inside an epoch
    tr = _Scripted([], n)
    hist = train.fit(tr, x, y, epochs=5, batch_size=3, seed=4, lr=0.01, max_steps=4)
    assert hist["steps"] == 4 and len(hist["loss"]) == 2 and hist["val_loss"] == [] and not hist["stopped_early"]
    assert set(tr.lrs) == {0.01}


def test_reduce_lr_floor_and_early_stopping_reset():
    p = train.ReduceLROnPlateau()
    lr = 3e-9
    for _ in range(4):
        lr = p.update(1.0, lr)
    assert lr == 1e-9                                                     # never below min_lr
    s = train.EarlyStopping(patience=2)
    assert [s.update(v) for v in (1.0, 1.0, 0.9, 0.9, 0.9)] == [False, False, False, False, True]


def test_fit_replay_in_float64_meets_the_gpu_tests_thresholds():
    """The condition tests/test_gpu_ftrain.py puts on the GPU's fit, met with room by the float64 replay: 40 Adam steps at batch 32,
    lr 0.01, seed 0 on the synthetic set halve the train loss and reach 0.9 accuracy."""
    x, y = ftrain_rows.fit_set()
    host = ftrain_ref.HostTrainer(fnet_rows.model(ftrain_rows.FIT_ROW))
    hist = train.fit(host, x, y, epochs=100, batch_size=ftrain_rows.FIT_BATCH, seed=0, lr=ftrain_rows.FIT_LR, max_steps=ftrain_rows.FIT_STEPS)
    assert hist["steps"] == 40
    r = host.grad(x, y)
    print("first epoch loss %.4f, last %.4f; final loss on the set %.4f, accuracy %.3f" % (hist["loss"][0], hist["loss"][-1], r["loss"].mean(),
                                                                                           (r["argmax"] == y).mean()))
    assert hist["loss"][-1] < 0.25 * hist["loss"][0] and (r["argmax"] == y).mean() >= 0.97

"""GPU tests (-m gpu) of the float32 trainer's gradient call beyond one tile per workgroup (ed_ftrain_grad_kernel, csrc/fnet_grad_kernels.hip;
DESIGN.md section 19): a workgroup's later tiles add into the slab its first tile stored, take over the LDS the backward half of the
tile before used, and write over that tile's activation, gradient and mask stores.

The exact check. Everything after dz = (p - onehot) / n is linear in dz (the MFMA chains, the slab store and adds, the reduce), and a
row labelled -1 in the device form counts in n but has dz = +0.0f. So tile j of a call of N rows, run alone among fillers labelled -1
in a call of n' rows, gives tile j's term of the big call times N / n', exactly where N and n' are powers of two and nothing leaves
the normal range; the small calls have one tile per workgroup, the path tests/test_gpu_ftrain.py holds to float64. The big call's
gradient must then be ftrain_ref.fold_tiles of those terms, element for element: the kernels' order restated in numpy. A tile dropped,
stored instead of added, added twice, taken in another order or read from a stale store changes floats (tests/test_fgrad_cpu.py holds
the fold's sensitivity). The float64 bound at these sizes only sees a whole tile lost (there too).

Every size comes from the trainer's own batch and grid (Trainer.info); nothing here skips on what the device is."""
import hashlib

import numpy as np
import pytest

import ftrain_ref
import fnet_host
import fnet_plan
import test_gpu_ftrain as gt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built_lib):
    from edison_amd.context import Context
    c = Context(0)
    yield c
    c.close()


_ROWS = {}


def rows(name, model, n, exact=False):
    """The first n rows and labels of a row's draw, made once for the largest n asked so far (a prefix of a longer draw is the
    shorter draw). exact=False: gt.data's, the sets n1, zero and neg. exact=True, for the scaling argument: N(0, 1) rows only -- the
    neg set saturates the softmax, its dz reaches down to 1e-37 and dz / N leaves the normal range --, and for the shipped network
    the fixture rows, which repeat, each with N(0, 1 % of its own sigma) noise, so that no two tiles are equal. Fixed seeds."""
    key = (name, exact)
    if key not in _ROWS or len(_ROWS[key][1]) < n:
        rng = np.random.default_rng(586 + sum(map(ord, name)))
        if exact and name != "cube_kws":
            n_out = int(np.prod(fnet_host.conv_records(model)[-1]["out"]))
            x, y = rng.normal(0, 1, (n, int(np.prod(model["in_shape"])))).astype(np.float32), (np.arange(n) % n_out).astype(np.int32)
        else:
            x, y = gt.data(name, model, n)
            if exact:
                x = (x + rng.normal(0, 1, x.shape) * 0.01 * x.std(axis=1, keepdims=True)).astype(np.float32)
        _ROWS[key] = (x, y)
    x, y = _ROWS[key]
    return x[:n], y[:n]


def pow2_at_least(v):
    return 1 << max(int(v) - 1, 0).bit_length()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_call(ctx, tr, name, model, real, x, y, w0):
    """One host-form gradient call of rows (x, y) held the way tests/test_gpu_ftrain.py holds its calls: logits and argmax
    edison_fnet_batch's bits, loss and every tensor by the float64 bounds, padding +0.0f, a repeat the same bits, nothing else moved.
    Returns the packed gradient."""
    n = len(y)
    ref = ftrain_ref.loss_grad(model, x, y)
    before = ctx.fnet(x)
    r = tr.grad(x, y)
    assert same_bits(tr.logits(n), before["logits"]), (name, n)
    assert np.array_equal(r["argmax"], before["argmax"])
    lb, le = ftrain_ref.bounds(model, x, y, ref)[1]
    lerr = ftrain_ref.tensor_error(r["loss"], ref["loss"])
    print("%s n=%d loss: gpu %.3g  e32 %.3g  bound %.3g" % (name, n, lerr, le, lb))
    assert lerr <= lb, (name, n, lerr, lb)
    gt.check_gradient(name, tr, model, real, x, y, ref)
    g = tr.gradient()
    r2 = tr.grad(x, y)
    assert same_bits(tr.gradient(), g), (name, n)
    assert same_bits(r2["loss"], r["loss"]) and same_bits(tr.logits(n), before["logits"])
    assert same_bits(tr.packed_weights(), w0)
    after = ctx.fnet(x)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    return g


# (row, tiles per workgroup at least): N is the smallest power of two >= that x grid x batch
EXACT = [("pool21_trunc_h", 2), ("pool21_trunc_h", 4), ("batch5", 2), ("cube_kws", 2)]


@pytest.mark.parametrize("name,per_wg", EXACT, ids=["%s-x%d" % c for c in EXACT])
def test_a_multi_tile_gradient_is_the_fold_of_its_tiles_exactly(ctx, name, per_wg):
    """On 256 CUs: pool21_trunc_h at N = 8 192 (512 tiles of 16, two per workgroup) and 16 384 (four per workgroup: a store and three
    adds), batch5 at its lowered batch 2 and N = 1 024 (two per workgroup), the shipped network at batch 7 and N = 4 096 (586 tiles,
    two or three per workgroup, the last one of one row)."""
    import torch
    model, blob, real = gt.case(name)
    ctx.fnet_load(blob)
    with ctx.trainer() as tr:
        info = tr.info()
        b, G, w = info["batch"], info["grid"], info["w_floats"]
        N = pow2_at_least(per_wg * G * b)
        n1 = pow2_at_least(b)                                               # rows of a small call: tile j's, then fillers
        n_tiles = (N + b - 1) // b
        assert n_tiles >= per_wg * G and n1 <= G * b and N >= 2 * n1
        x, y = rows(name, model, N + n1, exact=True)                        # n1 more finite rows behind the last tile: its fillers
        assert np.isfinite(x).all()
        w0 = tr.packed_weights()
        # the big call, held as every call is; then each of its tiles alone on the same trainer
        big = check_call(ctx, tr, name, model, real, x[:N], y[:N], w0)
        labels = np.full((n_tiles, n1), -1, np.int32)
        for j in range(n_tiles):
            own = y[j * b:min((j + 1) * b, N)]
            labels[j, :len(own)] = own
        fillers = int((labels < 0).sum())
        dev = torch.device("cuda", 0)
        xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev)
        torch.cuda.synchronize()                                            # the context's own stream takes them from here
        ignored0 = tr.info()["ignored"]
        T = np.empty((n_tiles, w), np.float32)
        smallest, digests = np.inf, set()
        for j in range(n_tiles):
            tr.grad_t(xt[j * b:j * b + n1], yt[j], n1)
            T[j] = tr.gradient()
            nz = np.abs(T[j][T[j] != 0])
            smallest = min(smallest, float(nz.min()) if nz.size else np.inf)
            digests.add(hashlib.blake2b(T[j].tobytes(), digest_size=16).digest())
            if j == 0:
                assert tr.info()["ignored"] - ignored0 == n1 - b
        assert tr.info()["ignored"] - ignored0 == fillers == n_tiles * n1 - N
        scale = n1 / N
        print("%s: batch %d, grid %d, N %d, %d tiles, small calls of %d rows, smallest term %.3g x %g" % (name, b, G, N, n_tiles, n1, smallest, scale))
        assert len(digests) == n_tiles, "two tiles give the same gradient: a swapped order would not show"
        assert np.isfinite(T).all() and smallest * scale > 2.0 ** -100
        assert not T[:, ~real].view(np.uint32).any()
        want = ftrain_ref.fold_tiles(T, G, scale)
        diff = np.flatnonzero(~(want == big))
        assert diff.size == 0, "%s: %d of %d gradient entries are not the fold of the tiles' (first at %d: call %r, fold %r)" % (
            name, diff.size, w, diff[0], big[diff[0]], want[diff[0]])
        assert not big[~real].view(np.uint32).any()
        assert same_bits(tr.packed_weights(), w0)


RAGGED = [("pool21_trunc_h", "1"), ("pool21_trunc_h", "b-1"), ("inc3_oc64_oc65_s21", "1"), ("inc3_oc64_oc65_s21", "b-1"), ("batch5", "1")]


@pytest.mark.parametrize("name,tail", RAGGED, ids=["%s-r=%s" % c for c in RAGGED])
def test_ragged_tile_counts_against_float64(ctx, name, tail):
    """n = 2 grid batch + 2 batch + r: workgroups 0, 1 and 2 take a third tile, and workgroup 2's is r rows short of full on stores
    that hold two full tiles' already. r = 1 and batch - 1 (batch5 trains at batch 2, where they are one case)."""
    model, blob, real = gt.case(name)
    ctx.fnet_load(blob)
    with ctx.trainer() as tr:
        info = tr.info()
        b, G = info["batch"], info["grid"]
        assert b == ftrain_ref.train_batch(fnet_plan.plan(blob)) and b >= 2
        assert b == 2 if name == "batch5" else b > 2                        # r = b - 1 is another case than r = 1
        r = 1 if tail == "1" else b - 1
        n = 2 * G * b + 2 * b + r
        assert (n + b - 1) // b == 2 * G + 3 and n % b == r
        x, y = rows(name, model, n)
        check_call(ctx, tr, name, model, real, x, y, tr.packed_weights())

"""GPU tests (-m gpu) of the float32 trainer's gradient call beyond one tile per workgroup (ed_ftrain_grad_kernel, csrc/fnet_grad_kernels.hip;
DESIGN.md section 19): a workgroup's later tiles add into the slab its first tile stored, take over the LDS the backward half of the
tile before used, and write over that tile's activation, gradient and mask stores.

The exact check. Everything after dz = (p - onehot) / n is linear in dz (the MFMA chains, the slab store and adds, the reduce), and a
row labelled -1 in the device form counts in n but has dz = +0.0f. So tile j of a call of N rows, run alone among fillers labelled -1
in a call of n' rows, gives tile j's term of the big call times N / n', exactly where N and n' are powers of two and nothing leaves
the normal range; the small calls have one tile per workgroup, the path tests/test_gpu_ftrain.py holds to float64. The big call's
gradient must then be ftrain_ref.fold_tiles of those terms, element for element: the kernels' order restated in numpy. A tile dropped,
stored instead of added, added twice, taken in another order or read from a stale store changes floats (tests/test_fgrad_cpu.py holds
the fold's sensitivity). The float64 bound at these sizes only sees a whole tile lost (there too). The body is
ftrain_drive.check_fold, which the padded trainer's test shares; the rows are ftrain_drive.rows'.

Every size comes from the trainer's own batch and grid (Trainer.info); nothing here skips on what the device is."""
import pytest

import ftrain_ref
import fnet_plan
from ftrain_drive import case, check_call, check_fold, own_context, rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built_lib):
    yield from own_context()


# (row, tiles per workgroup at least): N is the smallest power of two >= that x grid x batch
EXACT = [("pool21_trunc_h", 2), ("pool21_trunc_h", 4), ("batch5", 2), ("cube_kws", 2)]


@pytest.mark.parametrize("name,per_wg", EXACT, ids=["%s-x%d" % c for c in EXACT])
def test_a_multi_tile_gradient_is_the_fold_of_its_tiles_exactly(ctx, name, per_wg):
    """On 256 CUs: pool21_trunc_h at N = 8 192 (512 tiles of 16, two per workgroup) and 16 384 (four per workgroup: a store and three
    adds), batch5 at its lowered batch 2 and N = 1 024 (two per workgroup), the shipped network at batch 7 and N = 4 096 (586 tiles,
    two or three per workgroup, the last one of one row)."""
    model, blob, real = case(name)
    ctx.fnet_load(blob)
    with ctx.trainer() as tr:
        check_fold(ctx, tr, name, model, real, per_wg)


RAGGED = [("pool21_trunc_h", "1"), ("pool21_trunc_h", "b-1"), ("inc3_oc64_oc65_s21", "1"), ("inc3_oc64_oc65_s21", "b-1"), ("batch5", "1")]


@pytest.mark.parametrize("name,tail", RAGGED, ids=["%s-r=%s" % c for c in RAGGED])
def test_ragged_tile_counts_against_float64(ctx, name, tail):
    """n = 2 grid batch + 2 batch + r: workgroups 0, 1 and 2 take a third tile, and workgroup 2's is r rows short of full on stores
    that hold two full tiles' already. r = 1 and batch - 1 (batch5 trains at batch 2, where they are one case)."""
    model, blob, real = case(name)
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

"""The store of the fast MFCC loop (ed_mfcc2_body, csrc/mfcc_kernels.hip, step 7) at the smallest sizes where it can go wrong.

The store writes frame A's and frame B's rows with one instruction: a scalar row address from the pair's frame A, a per-lane offset
computed once in front of the loop, a lane mask (coefficient < n_coef, and frame B only where the pair has one), and one wave-uniform
branch per output wanted (float32, int8). Cases:
  frame counts 1, 2, 3, 25 (odd: the last pair has no frame B) in one plain batch, and 2 groups of 31 frames (the grouped instance;
  the pair of frames 30 | 31 straddles the groups);  n_coef 1, 13, 32;  float32 only, int8 only, both, int8 at scales 1 and 0.3.
Every output is a view with guard rows on both sides, which must not change. Every row is compared bit for bit with the row the
same frame got in ONE 64-frame, 32-coefficient, float32-only launch of the fast kernel (the one-frame kernel is another text of the
same sums and differs from the fast one in the last places: tests/test_gpu_mfcc_sweep.py compares the same way), and the int8 row with
round_half_even(clip(float32(coefficient) * float32(scale), -128, 127)) of that reference."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAME, N_BASE, GUARD_ROWS, GUARD_F, GUARD_Q = 1024, 64, 2, 4321.0, 99
N_COEFS = (1, 13, 32)
OUTS = (("f", 1.0), ("q", 1.0), ("q", 0.3), ("fq", 1.0), ("fq", 0.3))
FPG = 31
GROUP_STRIDE = FPG * FRAME + 64       # samples between the groups' first frames: even, so the aligned instance runs


class _Ref:
    """The base frames (speech-level noise, quiet noise, silence, the rails) and their 32 coefficients from one 64-frame launch"""

    def __init__(self, ctx):
        import torch
        from edison_amd import _lib
        self.torch, self.variant = torch, _lib.MFCC_B
        self.dev = torch.device("cuda", ctx.device)
        rng = np.random.default_rng(77)
        f = rng.normal(0, 3000, (N_BASE, FRAME))
        f[0] = 0
        f[1], f[2] = 32767, -32768
        f[3:11] = rng.normal(0, 0.01 * 32767, (8, FRAME))
        self.base = torch.from_numpy(np.clip(np.rint(f), -32768, 32767).astype(np.int16)).to(self.dev)
        self.coef = torch.empty((N_BASE, 32), dtype=torch.float32, device=self.dev)
        ctx.mfcc_t(self.base.reshape(-1), N_BASE, FRAME, self.variant, 32, out=self.coef)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(self.coef).all()) and float(self.coef.abs().max()) > 1.0

    def quantised(self, rows, scale):
        torch = self.torch
        s = torch.tensor(np.float32(scale), device=self.dev)
        return torch.round(torch.clamp(rows * s, -128.0, 127.0)).to(torch.int8)

    def guarded(self, n, nc, dtype):
        torch = self.torch
        buf = torch.full((n + 2 * GUARD_ROWS, nc), GUARD_F if dtype == torch.float32 else GUARD_Q, dtype=dtype, device=self.dev)
        return buf, buf[GUARD_ROWS:GUARD_ROWS + n]

    def guards_intact(self, buf, n):
        g = GUARD_F if buf.dtype == self.torch.float32 else GUARD_Q
        return bool((buf[:GUARD_ROWS] == g).all()) and bool((buf[GUARD_ROWS + n:] == g).all())


@pytest.fixture(scope="module")
def ref(ctx):
    ctx.use_torch_stream()
    try:
        yield _Ref(ctx)
    finally:
        ctx.use_own_stream()


@pytest.mark.parametrize("form,n", [("plain", 1), ("plain", 2), ("plain", 3), ("plain", 25), ("grouped", 2 * FPG)])
def test_store_paths(ctx, ref, form, n):
    torch = ref.torch
    idx = (torch.arange(n, device=ref.dev) * 5 + 3) % N_BASE            # which base frame sits in frame slot f
    if form == "plain":
        audio = ref.base[idx].reshape(-1).clone()
    else:
        audio = torch.randint(-3000, 3000, (2 * GROUP_STRIDE,), device=ref.dev, dtype=torch.int16)
        for g in range(2):
            audio[g * GROUP_STRIDE:g * GROUP_STRIDE + FPG * FRAME] = ref.base[idx[g * FPG:(g + 1) * FPG]].reshape(-1)
    for nc in N_COEFS:
        want_f = ref.coef[idx, :nc]
        for outs, scale in OUTS:
            fbuf, fo = ref.guarded(n, nc, torch.float32) if "f" in outs else (None, None)
            qbuf, qo = ref.guarded(n, nc, torch.int8) if "q" in outs else (None, None)
            if form == "plain":
                ctx.mfcc_t(audio, n, FRAME, ref.variant, nc, out=fo, feat=qo, feat_scale=scale)
            else:
                ctx.mfcc_rows_t(audio, 2, GROUP_STRIDE, FPG, FRAME, ref.variant, nc, out=fo, feat=qo, feat_scale=scale)
            torch.cuda.synchronize()
            case = (form, n, nc, outs, scale)
            if fo is not None:
                assert ref.guards_intact(fbuf, n), (case, "a guard row of the float32 output changed")
                bad = (fo != want_f).any(dim=1).nonzero()
                assert bad.numel() == 0, (case, "float32 rows differ from the 64-frame launch", bad[:6, 0].tolist())
            if qo is not None:
                assert ref.guards_intact(qbuf, n), (case, "a guard row of the int8 output changed")
                bad = (qo != ref.quantised(want_f, scale)).any(dim=1).nonzero()
                assert bad.numel() == 0, (case, "int8 rows are not the rounded float32 of the 64-frame launch", bad[:6, 0].tolist())

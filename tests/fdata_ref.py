"""Host restatements for training from scratch on a device-resident data set (edison_amd/train.py, csrc/fnet_data_kernels.hip; DESIGN.md
section 19d): Adadelta as Keras and torch.optim.Adadelta state it, in float64 and in the kernel's float32 arithmetic. Test
infrastructure, not a test: tests/test_ftrain_zoo_cpu.py holds the float64 one to torch and the float32 one to the float64 one,
tests/test_gpu_ftrain_data.py holds the kernel to the float64 one.

The step: a = rho a + (1 - rho) g g, u = g sqrt(d + eps) / sqrt(a + eps), w -= lr u, d = rho d + (1 - rho) u u, from a = d = 0."""
import numpy as np

EPS32 = 2.0 ** -24


class Adadelta:
    """float64, over any list of arrays (fgrad_ref.Adam's interface)."""

    def __init__(self, rho=0.95, eps=1e-7):
        self.rho, self.eps, self.a, self.d = rho, eps, None, None

    def step(self, ws, gs, lr):
        """ws, gs: lists of float64 arrays; ws is updated in place."""
        if self.a is None:
            self.a, self.d = [np.zeros_like(w) for w in ws], [np.zeros_like(w) for w in ws]
        for w, g, a, d in zip(ws, gs, self.a, self.d):
            a *= self.rho
            a += (1.0 - self.rho) * g * g
            u = g * np.sqrt(d + self.eps) / np.sqrt(a + self.eps)
            w -= lr * u
            d *= self.rho
            d += (1.0 - self.rho) * u * u


class Adadelta32:
    """ed_ftrain_adadelta_kernel's arithmetic in numpy float32: every product, sum, square root and quotient rounded to float32, the
    constants rho, 1 - rho (taken in double first, as the library does), eps and lr as floats. The kernel may fuse a product into the sum
    behind it, which this does not: one rounding fewer, inside the bound."""

    def __init__(self, rho=0.95, eps=1e-7):
        self.rho, self.omr, self.eps, self.a, self.d = np.float32(rho), np.float32(1.0 - rho), np.float32(eps), None, None

    def step(self, ws, gs, lr):
        """ws, gs: lists of float32 arrays; ws is updated in place."""
        lr = np.float32(lr)
        if self.a is None:
            self.a, self.d = [np.zeros_like(w) for w in ws], [np.zeros_like(w) for w in ws]
        for w, g, a, d in zip(ws, gs, self.a, self.d):
            assert w.dtype == g.dtype == a.dtype == d.dtype == np.float32
            a[...] = self.rho * a + self.omr * g * g
            u = g * np.sqrt(d + self.eps) / np.sqrt(a + self.eps)
            assert u.dtype == np.float32
            w -= lr * u
            d[...] = self.rho * d + self.omr * u * u


def tensor_error(got, want):
    """max |got - want| / max |want|: the error of a tensor against its largest value."""
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())

"""GPU tests (-m gpu) of the int8 network sweep (tests/net_sweep.py): every row through the general matrix-core kernel, the
layer-by-layer kernel, the planner's A/B knobs and the graph's own run-time-compiled kernel, bit for bit against oracle/net_ref.py.

Per row, n inputs for n in {1, batch - 1, batch, batch + 1, one more than a full pass of the persistent grid}:
  net(): logits, softmax and argmax equal net_ref; each input's answers do not depend on how many inputs share the call
  net_layers() (the layer-by-layer kernel) equals net_ref's activations, layer after layer
  under every knob of test_planner_cpu.KNOBS that changes the row's plan (a fresh load: the planner reads them at load time)
  and on the graph's own kernel (edison_net_specialize), whose tile counts stay those of a full batch even for the ragged counts
and every row cut behind each of its matrix-core layers (net_sweep.prefixes): the batch path's logits are then that layer's output."""
import numpy as np
import pytest

import net_sweep as ns
from test_net_sweep_cpu import _plan, knob_changes_plan
from test_planner_cpu import KNOBS

pytestmark = pytest.mark.gpu


def _full_pass(plan, n_cu):
    """Inputs one launch of ed_launch_net_mfma takes in one sweep of its persistent grid (cnn_net_mfma_kernels.hip:1219-1224)."""
    M = plan.M
    per_cu = max(1, min((160 * 1024) // (M.lds_bytes + 256), 32 // M.waves))
    return M.batch * M.waves * n_cu * per_cu


def _counts(plan, n_cu):
    b = plan.M.batch
    return sorted({n for n in (1, b - 1, b, b + 1, _full_pass(plan, n_cu) + 1) if n > 0})


def _first_diff(got, want, info):
    """'layer i byte j of input k' of the first difference of two activation dumps."""
    k, j = (int(v) for v in np.argwhere(got != want)[0])
    layer = max(i for i, L in enumerate(info["layers"]) if L["acts_offset"] <= j)
    return "layer %d byte %d of input %d: gpu %d, net_ref %d" % (layer, j - info["layers"][layer]["acts_offset"], k, got[k, j], want[k, j])


def _check_batch(c, name, x, ref, counts, what):
    for n in counts:
        out = c.net(x[:n])
        for k in ("logits", "softmax", "argmax"):
            if ref[k] is None:
                assert out[k] is None, (name, what, k)
                continue
            bad = np.argwhere(out[k] != ref[k][:n])
            assert not bad.size, "%s (%s), %d inputs: %d %s differ, first at %s (gpu %s, net_ref %s)" % (
                name, what, n, len(bad), k, bad[0].tolist(), out[k][tuple(bad[0])], ref[k][:n][tuple(bad[0])])


@pytest.fixture()
def jit_cache(tmp_path, monkeypatch):
    d = tmp_path / "jit"
    monkeypatch.setenv("EDISON_JIT_CACHE", str(d))
    monkeypatch.setenv("EDISON_NET_SPECIALIZE", "cache")
    return d


@pytest.mark.parametrize("name", list(ns.ROWS))
def test_row_bit_exact(built_lib, jit_cache, monkeypatch, name):
    from edison_amd import _lib
    from edison_amd.context import Context
    from oracle import net_ref
    blob = ns.blob(name)
    plan = _plan(name)
    accel0 = isinstance(plan, int)
    c = Context(0, model_path=None)
    try:
        c.load_model_bytes(blob)
        info = c.net_info()
        assert info["accelerated"] == (0 if accel0 else 2), name
        in_n = info["in_h"] * info["in_w"] * info["in_c"]
        n_cu = c.device_info()["n_cu"]
        counts = [1, 2, 3, 65] if accel0 else _counts(plan, n_cu)
        x = ns.inputs(name, counts[-1], in_n)
        ref = net_ref.run(blob, x)
        # the batch path: the general matrix-core kernel
        _check_batch(c, name, x, ref, counts, "general kernel")
        # per-layer dumps: the layer-by-layer kernel
        m = min(counts[-1], 67)
        got, want = c.net_layers(x[:m]), np.concatenate(ref["acts"], axis=1)[:m]
        assert np.array_equal(got, want), "%s net_layers: %s" % (name, _first_diff(got, want, info))
        if accel0:
            with pytest.raises(_lib.EdisonError):
                c.net_specialize()
            return
        # the planner's knobs, each on a fresh load; a few counts around the knob's own batch and one pass over several workgroups
        for k in KNOBS[1:]:
            knobs = tuple(sorted(k.items()))
            if not knob_changes_plan(name, knobs):
                continue
            kp = _plan(name, knobs)
            with monkeypatch.context() as mp:
                for kk, v in knobs:
                    mp.setenv(kk, v)
                c.load_model_bytes(blob)
            b = kp.M.batch
            kc = sorted({n for n in (1, b + 1, 3 * b * kp.M.waves + 1, counts[-1]) if n <= counts[-1]})
            _check_batch(c, name, x, ref, kc, "knobs %s" % dict(knobs))
        # the graph's own kernel, on the default plan
        c.load_model_bytes(blob)
        assert c.net_specialize() in (1, 3), name
        _check_batch(c, name, x, ref, counts, "own kernel")
    finally:
        c.close()


@pytest.mark.parametrize("name", list(ns.ROWS))
def test_layer_cuts_bit_exact(built_lib, name):
    """Row `name` cut behind each matrix-core layer (net_sweep.prefixes): the batch path's logits are that layer's output, so a
    wrong byte cannot be washed out by the layers behind it."""
    from edison_amd.context import Context
    from oracle import net_ref
    c = Context(0, model_path=None)
    try:
        for li, blob in ns.prefixes(name):
            c.load_model_bytes(blob)
            info = c.net_info()
            in_n = info["in_h"] * info["in_w"] * info["in_c"]
            x = ns.inputs(name, 97, in_n)
            ref = net_ref.run(blob, x)
            _check_batch(c, name, x, ref, (1, 2, 3, 5, 97), "cut behind layer %d, accelerated %d" % (li, info["accelerated"]))
    finally:
        c.close()

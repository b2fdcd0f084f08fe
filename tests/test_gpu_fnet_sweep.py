"""GPU tests (-m gpu) of the float-network sweep (tests/fnet_rows.py): every row's layers and logits bit for bit against the host
model of the kernel (tests/fnet_host.py), at utterance counts around the workgroup's tile; the loader's refusals; the device entry
point with one output at a time.

Per row and count n in {1, batch - 1, batch, batch + 1, 3 batch + 2}:
  fnet_info = the restated plan (batch, lds_bytes, acts_floats, n_layers)
  every layer of fnet_layers, layer i fed the kernel's own layer i - 1, and the logits of fnet: bit-equal to fnet_host
  every layer within 8e-7 S of the float64 restatement (tests/fnet_host.py; plus the underflow term on the subnormal row)
  probs within 1e-6 of the float64 softmax of the kernel's logits; argmax the first maximum of the kernel's probs
  each utterance's layers and answers independent of how many utterances share the call"""
import numpy as np
import pytest

import fnet_host as fh
import fnet_plan as fpl
import fnet_rows as fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built_lib):
    from edison_amd.context import Context
    c = Context(0)
    yield c
    c.close()


def _counts(batch):
    return sorted({n for n in (1, batch - 1, batch, batch + 1, 3 * batch + 2) if n > 0})


@pytest.mark.parametrize("name", list(fr.SWEEP))
def test_row_bit_exact(ctx, name):
    blob = fr.blob(name)
    p, m = fpl.plan(blob), fh.load(blob)
    ctx.fnet_load(blob)
    info = ctx.fnet_info()
    assert (info["batch"], info["lds_bytes"], info["acts_floats"], info["n_layers"], info["n_out"]) == \
        (p["batch"], p["lds_bytes"], p["acts_floats"], p["n_layers"], p["n_out"])
    counts = _counts(p["batch"])
    x = fr.inputs(name, counts[-1], p["in_n"])
    acts = ctx.fnet_layers(x)
    want, got = fh.layers_from(m, x, acts)
    prev = x
    for i, (L, w, g) in enumerate(zip(fh.conv_records(m), want, got)):
        diff = w != g
        assert np.array_equal(w, g), "%s layer %d: %d of %d outputs differ from the fmaf chain (first at %s: gpu %r, model %r)" % (
            name, i, diff.sum(), diff.size, np.argwhere(diff)[0], g[diff][0], w[diff][0])
        w64, S = fh.layer_from(m, i, prev)
        assert (np.abs(g - w64) <= fh.bound(L, S)).all(), (name, i)
        prev = g
    full = ctx.fnet(x)
    assert np.array_equal(full["logits"], want[-1])
    for n in counts:
        a = ctx.fnet_layers(x[:n])
        assert np.array_equal(a, acts[:n]), (name, n)
        r = ctx.fnet(x[:n])
        assert np.array_equal(r["logits"], want[-1][:n]), (name, n)
        assert np.abs(r["probs"] - fh.softmax(r["logits"].astype(np.float64))).max() <= 1e-6
        assert np.array_equal(r["argmax"], np.argmax(r["probs"], axis=1))
        assert np.array_equal(r["probs"], full["probs"][:n]) and np.array_equal(r["argmax"], full["argmax"][:n])
    zero = ~want[-1].any(axis=1)
    if fh.conv_records(m)[-1]["relu"] and zero.any():
        assert not full["logits"][zero].any() and not full["argmax"][zero].any()


def test_refusals_keep_the_loaded_network(ctx):
    """Every refusal returns its code and leaves the network loaded before it answering bit-identically."""
    from edison_amd import _lib
    name = "pool22_trunc_hw"
    ctx.fnet_load(fr.blob(name))
    p = fpl.plan(fr.blob(name))
    x = fr.inputs(name, 3 * p["batch"] + 2, p["in_n"])
    before, acts = ctx.fnet(x), ctx.fnet_layers(x)
    for ref, (build, code, note) in fr.SWEEP_REFUSALS.items():
        with pytest.raises(_lib.EdisonError) as e:
            ctx.fnet_load(build())
        assert e.value.code == code, (ref, note)
        after = ctx.fnet(x)
        assert all(np.array_equal(before[k], after[k]) for k in before), ref
        assert np.array_equal(ctx.fnet_layers(x), acts), ref


def test_device_one_output_at_a_time(ctx):
    """edison_fnet_batch_dev on a torch stream with only logits, only probs or only argmax equals the host call."""
    torch = pytest.importorskip("torch")
    name = "inc3_oc64_oc65_s21"
    ctx.fnet_load(fr.blob(name))
    p = fpl.plan(fr.blob(name))
    n = 3 * p["batch"] + 2
    x = fr.inputs(name, n, p["in_n"])
    want = ctx.fnet(x)
    dev = torch.device("cuda", 0)
    xt = torch.from_numpy(x).to(dev)
    outs = dict(logits=torch.full((n, p["n_out"]), -1.0, dtype=torch.float32, device=dev),
                probs=torch.full((n, p["n_out"]), -1.0, dtype=torch.float32, device=dev),
                argmax=torch.full((n,), -1, dtype=torch.int32, device=dev))
    ctx.use_torch_stream()
    try:
        for k in outs:
            ctx.fnet_t(xt, n, **{k: outs[k]})
        torch.cuda.current_stream().synchronize()
    finally:
        ctx.use_own_stream()
    for k in outs:
        assert np.array_equal(outs[k].cpu().numpy(), want[k]), k

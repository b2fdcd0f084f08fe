"""GPU tests (-m gpu) of the branching sweep (tests/branch_sweep.py): every row through the fused one-launch kernel -- its DW_Conv2D,
AvgPool, Add / Sub / Mult and Concat passes, its held areas -- or, where the note says the fused planner declines the graph,
through the layer-by-layer kernel; bit for bit against tests/res_ref.py.

Per row, in one in-process Context:
  net_info()["accelerated"] is what the note claims
  net(): logits, softmax and argmax equal res_ref at 1, ipw - 1, ipw + 1 and 3 ipw + 2 inputs (ipw: the plan's inputs per wave)
  net_layers() (the layer-by-layer kernel) equals res_ref at every record
  every cut of the row (branch_sweep.cuts) equals res_ref at its logits: a record's own output, which nothing behind it can wash out
and all rows once more under EDISON_NET_NO_MFMA=1, in one child process (the library reads the variable once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import branch_sweep as bs
import res_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _ipw(blob):
    """Inputs a wavefront of the fused kernel takes at a time (ed_mm_plan_t.batch); 4, its largest, for a graph without a fused plan."""
    import plan_emulator
    from edison_amd import _lib
    try:
        return int(plan_emulator.Plan(blob).M.batch)
    except _lib.EdisonError:
        return 4


def _batches(ipw):
    return sorted({1, max(ipw - 1, 1), ipw + 1, 3 * ipw + 2})


@pytest.fixture(scope="module")
def refs(built_lib):
    """name -> (blob, 14 inputs, res_ref.run of them): computed once, shared, never changed."""
    out = {}
    for name in bs.ROWS:
        blob = bs.blob(name)
        x = bs.inputs(name, 14)
        r = res_ref.run(blob, x)
        for a in r["acts"]:
            a.setflags(write=False)
        out[name] = (blob, x, r)
    return out


def _check_net(c, x, r, n, what):
    out = c.net(x[:n])
    for k in ("logits", "softmax", "argmax"):
        if r[k] is None:
            assert out[k] is None, (what, k)
            continue
        bad = np.argwhere(out[k] != r[k][:n])
        assert not bad.size, "%s, %d inputs: %d %s differ, first at %s (gpu %s, res_ref %s)" % (
            what, n, len(bad), k, bad[0].tolist(), out[k][tuple(bad[0])], r[k][:n][tuple(bad[0])])


@pytest.mark.parametrize("name", list(bs.ROWS))
def test_row_bit_exact(built_lib, refs, name):
    from edison_amd.context import Context
    blob, x, r = refs[name]
    note = bs.claims(bs.ROWS[name][1])
    c = Context(0, model_path=None)
    try:
        c.load_model_bytes(blob)
        info = c.net_info()
        assert info["accelerated"] == note.get("accelerated", 2), name
        ipw = _ipw(blob)
        assert "batch" not in note or note["batch"] == ipw
        assert 3 * ipw + 2 <= len(x)
        for n in _batches(ipw):
            _check_net(c, x, r, n, name)
        got = c.net_layers(x)
        for i, (L, want) in enumerate(zip(info["layers"], r["acts"])):
            seg = got[:, L["acts_offset"]:L["acts_offset"] + want.shape[1]]
            bad = np.argwhere(seg != want)
            assert not bad.size, "%s net_layers: record %d (type %d) differs at %s" % (name, i, L["type"], bad[0].tolist())
        assert got.shape[1] == sum(a.shape[1] for a in r["acts"])
    finally:
        c.close()


@pytest.mark.parametrize("name", list(bs.ROWS))
def test_cuts_bit_exact(built_lib, refs, name):
    from edison_amd.context import Context
    _, x, full = refs[name]
    c = Context(0, model_path=None)
    try:
        for li, blob in bs.cuts(name):
            c.load_model_bytes(blob)
            r = res_ref.run(blob, x)
            assert np.array_equal(r["logits"], full["acts"][li])
            for n in _batches(_ipw(blob)):
                _check_net(c, x, r, n, "%s cut behind record %d, accelerated %d" % (name, li, c.net_info()["accelerated"]))
    finally:
        c.close()


NO_MFMA_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from edison_amd.context import Context
g = np.load(sys.argv[2])
names = [k[5:] for k in g.files if k.startswith("blob_")]
assert names
c = Context(0, model_path=None)
for name in names:
    c.load_model_bytes(g["blob_" + name].tobytes())
    x = g["x_" + name]
    for n in (1, 3, x.shape[0]):
        out = c.net(x[:n])
        assert np.array_equal(out["logits"], g["logits_" + name][:n]), name
        assert np.array_equal(out["argmax"], g["argmax_" + name][:n]), name
        if "softmax_" + name in g.files:
            assert np.array_equal(out["softmax"], g["softmax_" + name][:n]), name
        else:
            assert out["softmax"] is None, name
c.close()
print("ok", len(names))
"""


def test_every_row_on_the_layer_by_layer_route_of_net_batch(built_lib, refs, tmp_path):
    """EDISON_NET_NO_MFMA=1 (read once per process, so one fresh child process): net() on the layer-by-layer kernel equals res_ref
    for every row; the parent hands over blobs, inputs and expected values in one file."""
    data = {}
    for name, (blob, x, r) in refs.items():
        data["blob_" + name], data["x_" + name] = np.frombuffer(blob, np.uint8), x
        data["logits_" + name], data["argmax_" + name] = r["logits"], r["argmax"]
        if r["softmax"] is not None:
            data["softmax_" + name] = r["softmax"]
    np.savez(tmp_path / "rows.npz", **data)
    script = tmp_path / "no_mfma.py"
    script.write_text(NO_MFMA_CHILD)
    env = dict(os.environ, EDISON_NET_NO_MFMA="1")
    p = subprocess.run([sys.executable, "-u", str(script), os.path.dirname(HERE), str(tmp_path / "rows.npz")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok %d" % len(refs)), p.stdout[-1000:] + p.stderr[-3000:]

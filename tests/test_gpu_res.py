"""GPU tests of the branching graphs (Add, Sub, Mult, Concat and hooks from earlier layers) on the general int8 network path.
Integer arithmetic: every comparison is bit for bit.

Expected values: tests/golden/res_golden.npz (tests/golden/gen_fixtures_res.py: the reference's model_run() for `cat`; for the
other four, whose Add / Sub / Mult layers the reference cannot compile, tests/res_ref.py with every merge step checked against
the reference's own arm_*_q7 / local_*_q7 routines) and tests/res_ref.py itself, pinned on the CPU by tests/test_res_cpu.py.
The graphs are small (12 x 10 x 1 inputs, up to 34 channels); every GPU step is one in-process call.

Routes: the layer-by-layer kernel (cnn_net_kernels.hip) runs all five graphs. The fused one-launch kernel runs `kws` and `edges`
(held areas in the wave's LDS slice, ED_RUN_MERGE passes), `pool` (a MaxPool fused into a convolution that reads a held tensor) and
`cat2` (ED_RUN_CAT passes); the last two at two inputs per wave: accelerated == 2. `cat` is documented to stay layer by layer
(accelerated == 0): its stem feeds a 1x1 convolution, a zero-padded 3x3 convolution and a pool, which want three LDS layouts of one
tensor (model_net_mm.c). net() of a graph with a fused plan runs the fused kernel, net_layers() always the layer-by-layer one, so
the first test compares both routes with the vectors.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
NAMES = ["kws", "edges", "cat", "pool", "cat2"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "res_golden.npz"))


def _header(name):
    return os.path.join(GOLDEN, "alt_models", "res_%s.h" % name)


def _blob(name):
    from edison_amd import nnom_import
    with open(_header(name)) as f:
        shape, layers = nnom_import.parse_weights_h(f.read())
    return nnom_import.build_blob(shape, layers)


@pytest.fixture(scope="module")
def refs(golden):
    """name -> (blob, inputs, res_ref.run of them): computed once, shared, never changed."""
    import res_ref
    out = {}
    for name in NAMES:
        blob = _blob(name)
        x = golden["in_" + name]
        r = res_ref.run(blob, x)
        for a in r["acts"]:
            a.setflags(write=False)
        out[name] = (blob, x, r)
    return out


def _inputs_per_wave(blob):
    """Inputs a wavefront of the fused kernel takes at a time, from the planner (ed_mm_plan_t.batch); 4, its largest, for a graph
    without a fused plan."""
    import plan_emulator
    from edison_amd import _lib
    try:
        return int(plan_emulator.Plan(blob).M.batch)
    except _lib.EdisonError:
        return 4


def _batches(ipw):
    return sorted({1, max(ipw - 1, 1), ipw + 1, 3 * ipw + 2})


def _check_net(c, x, r, acts_ref, argmax_ref, n):
    out = c.net(x[:n])
    assert np.array_equal(out["logits"], r["logits"][:n])
    if r["softmax"] is None:
        assert out["softmax"] is None
    else:
        assert np.array_equal(out["softmax"], r["softmax"][:n])
        assert np.array_equal(out["softmax"], acts_ref[:n, -r["softmax"].shape[1]:])
    assert np.array_equal(out["argmax"], argmax_ref[:n]) and np.array_equal(out["argmax"], r["argmax"][:n])


@pytest.mark.parametrize("name", NAMES)
def test_layers_and_net_match_the_reference(built_lib, golden, refs, name):
    """edison_net_layers at every layer and edison_net_batch, at batch sizes either side of a wave's share."""
    from edison_amd.context import Context
    blob, x, r = refs[name]
    acts_ref, argmax_ref = golden["acts_" + name], golden["argmax_" + name]
    assert np.array_equal(np.concatenate(r["acts"], axis=1), acts_ref)
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(_header(name))
        info = c.net_info()
        assert info["acts_bytes"] == acts_ref.shape[1]
        assert {L["type"] for L in info["layers"]} & {7, 8, 9, 10}
        ipw = _inputs_per_wave(blob)
        assert 3 * ipw + 2 <= x.shape[0]
        for n in _batches(ipw):
            got = c.net_layers(x[:n])
            for L, want in zip(info["layers"], r["acts"]):
                seg = got[:, L["acts_offset"]:L["acts_offset"] + want.shape[1]]
                assert np.array_equal(seg, want[:n]), "layer of type %d, %d inputs" % (L["type"], n)
            assert np.array_equal(got, acts_ref[:n])
            _check_net(c, x, r, acts_ref, argmax_ref, n)
    finally:
        c.close()


@pytest.mark.parametrize("name", ["kws", "edges", "pool", "cat2"])
def test_residual_graphs_take_the_fused_kernel(built_lib, name):
    """accelerated == 2: these graphs have a plan for the fused kernel, which net() then runs; `pool` and `cat2` with more than one
    input per wave, `cat2` through the Concat pass."""
    from edison_amd.context import Context
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(_header(name))
        assert c.net_info()["accelerated"] == 2
        if name in ("pool", "cat2"):
            assert _inputs_per_wave(_blob(name)) >= 2
    finally:
        c.close()


def test_inception_graph_stays_layer_by_layer(built_lib):
    """`cat`: the planner documents the layer-by-layer route for it (see the head of this file)."""
    from edison_amd.context import Context
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(_header("cat"))
        assert c.net_info()["accelerated"] == 0
    finally:
        c.close()


NO_MFMA_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from edison_amd.context import Context
g = np.load(os.path.join(sys.argv[1], "tests", "golden", "res_golden.npz"))
for name in ("kws", "edges", "cat", "pool", "cat2"):
    c = Context(0, model_path=None)
    c.load_weights_h(os.path.join(sys.argv[1], "tests", "golden", "alt_models", "res_%s.h" % name))
    info = c.net_info()
    x, acts = g["in_" + name], g["acts_" + name]
    n_out = info["n_out"]
    for n in (1, 3, x.shape[0]):
        out = c.net(x[:n])
        last = acts[:n, -n_out:]
        assert np.array_equal(out["argmax"], g["argmax_" + name][:n]), name
        if info["has_softmax"]:
            assert np.array_equal(out["softmax"], last) and np.array_equal(out["logits"], acts[:n, -2 * n_out:-n_out]), name
        else:
            assert out["softmax"] is None and np.array_equal(out["logits"], last), name
    c.close()
print("ok")
"""


def test_layer_by_layer_route_of_net_batch(built_lib, tmp_path):
    """EDISON_NET_NO_MFMA=1 (read once per process, so a child process): edison_net_batch on the layer-by-layer kernel equals the npz."""
    import subprocess
    import sys
    script = tmp_path / "no_mfma.py"
    script.write_text(NO_MFMA_CHILD)
    env = dict(os.environ, EDISON_NET_NO_MFMA="1")
    p = subprocess.run([sys.executable, "-u", str(script), os.path.dirname(HERE)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-1000:] + p.stderr[-3000:]


def _table(blob):
    head = np.frombuffer(blob, dtype="<i4", count=8, offset=8)
    return 40 + 48 * int(head[3]) + int(head[6])


def test_corrupted_source_table_is_refused_and_the_loaded_graph_stays(built_lib, golden, refs):
    import res_ref
    from edison_amd import _lib
    from edison_amd.context import Context
    blob, x, r = refs["edges"]
    src = res_ref.sources(blob)
    c = Context(0, model_path=None)
    try:
        c.load_model_bytes(blob)
        before = c.net_layers(x)
        at = _table(blob)
        words = np.frombuffer(blob, dtype="<i4", count=sum(len(s) + 1 for s in src), offset=at).copy()
        starts = np.cumsum([0] + [len(s) + 1 for s in src])
        # a forward reference: the Sub (record 3) reads record 5
        bad = words.copy()
        bad[starts[3] + 1] = 5
        b1 = bytearray(blob)
        b1[at:at + bad.nbytes] = bad.tobytes()
        with pytest.raises(_lib.EdisonError) as e:
            c.load_model_bytes(bytes(b1))
        assert e.value.code in (_lib.E_SIZE, _lib.E_NO_IMPL) and "layer 3" in str(e.value)
        # a shape mismatch: the Mult of 34-channel maps (record 8) reads the 6-channel record 5
        bad = words.copy()
        bad[starts[8] + 2] = 5
        b2 = bytearray(blob)
        b2[at:at + bad.nbytes] = bad.tobytes()
        with pytest.raises(_lib.EdisonError) as e:
            c.load_model_bytes(bytes(b2))
        assert e.value.code in (_lib.E_SIZE, _lib.E_NO_IMPL) and "layer 8" in str(e.value)
        assert np.array_equal(c.net_layers(x), before) and np.array_equal(before, golden["acts_edges"])
        _check_net(c, x, r, golden["acts_edges"], golden["argmax_edges"], x.shape[0])
    finally:
        c.close()


def test_specialize_declines_and_the_load_survives(built_lib, golden, refs, monkeypatch):
    from edison_amd import _lib
    from edison_amd.context import Context
    blob, x, r = refs["kws"]
    monkeypatch.setenv("EDISON_JIT_CACHE", "off")
    monkeypatch.setenv("EDISON_NET_SPECIALIZE", "1")
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(_header("kws"))
        assert c.net_specialized() == 0
        with pytest.raises(_lib.EdisonError) as e:
            c.net_specialize()
        assert e.value.code == _lib.E_NO_IMPL and "branching graph" in str(e.value)
        _check_net(c, x, r, golden["acts_kws"], golden["argmax_kws"], x.shape[0])
    finally:
        c.close()


def test_kws_geom_serves_the_residual_graph(built_lib, refs):
    """Audio to class in one call with res_kws loaded, at the 12-frame x 10-coefficient geometry its input implies."""
    import res_ref
    from edison_amd import _lib
    from edison_amd.context import Context
    from edison_amd.kws.geometry import KwsGeometry
    blob = refs["kws"][0]
    g = KwsGeometry.from_config(variant=_lib.MFCC_B, frame_len=441, frame_step=441, n_samples=5292, mel_nbins=16, first_mfcc=0, num_mfcc=10)
    assert (g.frame_count, g.num_mfcc) == (12, 10)
    rng = np.random.default_rng(78)
    audio = np.clip(np.rint(rng.normal(0, 1, (9, g.n_samples)) * rng.uniform(5, 20000, (9, 1))), -32768, 32767).astype(np.int16)
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(_header("kws"))
        r = c.kws_geom(audio, g)
        y = c.mfcc_geom(audio, g)
        feat = np.rint(np.clip(y.astype(np.float32) * np.float32(g.net_input_scale), np.float32(-128), np.float32(127))).astype(np.int8).reshape(9, -1)
        assert np.array_equal(r["feat"], feat)
        o = c.net(feat)
        want = res_ref.run(blob, feat)
        for k in ("logits", "softmax", "argmax"):
            assert np.array_equal(r[k], o[k]) and np.array_equal(r[k], want[k]), k
    finally:
        c.close()

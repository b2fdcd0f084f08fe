"""GPU tests of DW_Conv2D and AvgPool on the general int8 network path: the layer-by-layer kernel (cnn_net_kernels.hip), the
fused matrix-core kernel with the two layers on the VALU between its MFMA layers (cnn_net_mfma_kernels.hip, ED_RUN_DW /
ED_RUN_AVG) and the audio-to-class entry point in front of them. Integer arithmetic: every comparison is bit for bit.

Expected values: tests/golden/dscnn_golden.npz, the REFERENCE's own NNoM 0.3.0 + CMSIS-NN compiled around the three
dscnn_*.h headers (tests/golden/gen_fixtures_dscnn.py), and tests/dscnn_ref.py, the numpy restatement pinned to them on the
CPU (tests/test_dscnn_cpu.py). The graphs are small on purpose (inputs up to 12 x 10, 2 .. 66 channels; what each one
holds is listed in the generator); every GPU step is one in-process call.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
NAMES = ["kws", "edges", "square"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "dscnn_golden.npz"))


def _header(name):
    return os.path.join(GOLDEN, "alt_models", "dscnn_%s.h" % name)


def _blob(name):
    from edison_amd import nnom_import
    with open(_header(name)) as f:
        shape, layers = nnom_import.parse_weights_h(f.read())
    return nnom_import.build_blob(shape, layers)


def _inputs_per_wave(blob):
    """The fused kernel's inputs per wavefront for this graph, from the planner itself (ed_mm_plan_t.batch)."""
    import plan_emulator
    return int(plan_emulator.Plan(blob).M.batch)


def _batches(ipw):
    return sorted({1, max(ipw - 1, 1), ipw + 1, 3 * ipw + 2})


@pytest.fixture(scope="module")
def refs(golden):
    """name -> (blob, inputs, dscnn_ref.run of them): computed once, shared, never changed."""
    import dscnn_ref
    out = {}
    for name in NAMES:
        blob = _blob(name)
        x = golden["in_" + name]
        r = dscnn_ref.run(blob, x)
        for a in r["acts"]:
            a.setflags(write=False)
        out[name] = (blob, x, r)
    return out


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
def test_layers_and_fused_kernel_match_the_reference(built_lib, golden, refs, name):
    """edison_net_layers at every layer and edison_net_batch on the fused kernel, at batch sizes either side of the wave's share."""
    from edison_amd.context import Context
    blob, x, r = refs[name]
    acts_ref, argmax_ref = golden["acts_" + name], golden["argmax_" + name]
    assert np.array_equal(np.concatenate(r["acts"], axis=1), acts_ref)
    ipw = _inputs_per_wave(blob)
    assert 3 * ipw + 2 <= x.shape[0]
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(_header(name))
        info = c.net_info()
        assert info["acts_bytes"] == acts_ref.shape[1]
        assert info["accelerated"] == 2, "the graph must have a plan for the fused kernel"
        assert {5, 6} <= {L["type"] for L in info["layers"]}
        for n in _batches(ipw):
            got = c.net_layers(x[:n])
            for L, want in zip(info["layers"], r["acts"]):
                seg = got[:, L["acts_offset"]:L["acts_offset"] + want.shape[1]]
                assert np.array_equal(seg, want[:n]), "layer of type %d, %d inputs" % (L["type"], n)
            assert np.array_equal(got, acts_ref[:n])
            _check_net(c, x, r, acts_ref, argmax_ref, n)
    finally:
        c.close()


def test_batch_knobs_keep_working(built_lib, golden, refs, monkeypatch):
    """EDISON_NET_BATCH / EDISON_NET_MIN_WAVES still steer the planner for a graph with the new layers: 1 and 4 inputs per wave."""
    from edison_amd.context import Context
    blob, x, r = refs["kws"]
    for b in ("1", "4"):
        monkeypatch.setenv("EDISON_NET_BATCH", b)
        monkeypatch.setenv("EDISON_NET_MIN_WAVES", "1")
        assert _inputs_per_wave(blob) == int(b)
        c = Context(0, model_path=None)
        try:
            c.load_weights_h(_header("kws"))
            assert c.net_info()["accelerated"] == 2
            for n in (1, int(b) + 1, x.shape[0]):
                _check_net(c, x, r, golden["acts_kws"], golden["argmax_kws"], n)
        finally:
            c.close()


NO_MFMA_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from edison_amd.context import Context
g = np.load(os.path.join(sys.argv[1], "tests", "golden", "dscnn_golden.npz"))
for name in ("kws", "edges", "square"):
    c = Context(0, model_path=None)
    c.load_weights_h(os.path.join(sys.argv[1], "tests", "golden", "alt_models", "dscnn_%s.h" % name))
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


def test_refused_graph_leaves_the_loaded_one_in_place(built_lib, golden, refs):
    from edison_amd import _lib, nnom_import
    from edison_amd.context import Context
    blob, x, r = refs["edges"]
    c = Context(0, model_path=None)
    try:
        c.load_model_bytes(blob)
        before = c.net_layers(x)
        with open(_header("edges")) as f:
            shape, layers = nnom_import.parse_weights_h(f.read())
        bad = bytearray(blob)
        recs = np.frombuffer(bad, dtype="<i4", count=12 * len(layers), offset=40).reshape(-1, 12)
        avg = [i for i, L in enumerate(layers) if L["type"] == nnom_import.T_AVGPOOL][0]
        recs = recs.copy()
        recs[avg, 7] = 1                                          # an AvgPool output_shift no generated header can state
        bad[40:40 + recs.nbytes] = recs.tobytes()
        with pytest.raises(_lib.EdisonError) as e:
            c.load_model_bytes(bytes(bad))
        assert e.value.code == _lib.E_NO_IMPL and "AvgPool" in str(e.value)
        recs[avg, 7] = 0
        dw = [i for i, L in enumerate(layers) if L["type"] == nnom_import.T_DWCONV][0]
        recs[dw, 1] = 3                                           # a depth multiplier's worth of channels that the input does not have
        bad[40:40 + recs.nbytes] = recs.tobytes()
        with pytest.raises(_lib.EdisonError) as e:
            c.load_model_bytes(bytes(bad))
        assert e.value.code == _lib.E_SIZE and "DW_Conv2D" in str(e.value)
        assert np.array_equal(c.net_layers(x), before) and np.array_equal(before, golden["acts_edges"])
        _check_net(c, x, r, golden["acts_edges"], golden["argmax_edges"], x.shape[0])
    finally:
        c.close()


def test_specialize_declines_and_the_load_survives(built_lib, golden, refs, monkeypatch):
    """A graph with the new layers keeps the general kernel: edison_net_specialize says EDISON_E_NO_IMPL, EDISON_NET_SPECIALIZE=1 loads it."""
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
        assert e.value.code == _lib.E_NO_IMPL
        _check_net(c, x, r, golden["acts_kws"], golden["argmax_kws"], x.shape[0])
    finally:
        c.close()


def test_kws_geom_serves_the_ds_cnn(built_lib, refs):
    """Audio to class in one call with the DS-CNN loaded, at the 12-frame x 10-coefficient geometry its input implies: the features
    are mfcc_geom's coefficients rounded to int8, the outputs are net() of those features and the restatement's."""
    import dscnn_ref
    from edison_amd import _lib
    from edison_amd.context import Context
    from edison_amd.kws.geometry import KwsGeometry
    blob = refs["kws"][0]
    g = KwsGeometry.from_config(variant=_lib.MFCC_B, frame_len=441, frame_step=441, n_samples=5292, mel_nbins=16, first_mfcc=0, num_mfcc=10)
    assert (g.frame_count, g.num_mfcc) == (12, 10)
    rng = np.random.default_rng(77)
    audio = np.clip(np.rint(rng.normal(0, 1, (9, g.n_samples)) * rng.uniform(5, 20000, (9, 1))), -32768, 32767).astype(np.int16)
    c = Context(0, model_path=None)
    try:
        c.load_weights_h(_header("kws"))
        r = c.kws_geom(audio, g)
        y = c.mfcc_geom(audio, g)
        feat = np.rint(np.clip(y.astype(np.float32) * np.float32(g.net_input_scale), np.float32(-128), np.float32(127))).astype(np.int8).reshape(9, -1)
        assert np.array_equal(r["feat"], feat)
        o = c.net(feat)
        want = dscnn_ref.run(blob, feat)
        for k in ("logits", "softmax", "argmax"):
            assert np.array_equal(r[k], o[k]) and np.array_equal(r[k], want[k]), k
    finally:
        c.close()

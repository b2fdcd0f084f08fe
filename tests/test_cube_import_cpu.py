"""X-CUBE-AI float networks without a GPU: the importer (edison_amd/cube_import.py) on the reference's kws.c / kws_data.c and on
networks written in the same format, the float64 restatement (tests/fnet_host.py) on the fixture, and the kernel's compile."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from edison_amd import cube_import

import cube_synth
import fnet_host

CUBE = "/root/reference/firmware/src/ai/cube/kws"
FIXTURE = os.path.join(GOLDEN, "cube_kws.ednf")


@pytest.fixture(scope="module")
def model():
    return fnet_host.load(FIXTURE)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "cube_golden.npz"))


@pytest.mark.skipif(not os.path.exists(os.path.join(CUBE, "kws.c")), reason="the reference's X-CUBE-AI sources are not on this machine")
def test_import_reproduces_fixture(tmp_path):
    out = tmp_path / "kws.ednf"
    from edison_amd.cube_import import main
    assert main(["import_cube", os.path.join(CUBE, "kws.c"), os.path.join(CUBE, "kws_data.c"), str(out), os.path.join(CUBE, "keywords.txt")]) == 0
    with open(FIXTURE, "rb") as f:
        assert out.read_bytes() == f.read()


def test_fixture_layers(model):
    """kws.c's chain: conv2d_nl_pool x2, conv2d x2 (all ReLU), dense, softmax; HWC 31 x 13 x 1 in, 10 out."""
    assert model["in_shape"] == (31, 13, 1) and model["n_out"] == 10
    assert model["keywords"][0] == "edison" and len(model["keywords"]) == 10
    convs = fnet_host.conv_records(model)
    assert [L["out"] for L in convs] == [(13, 9, 16), (5, 7, 32), (3, 5, 64), (1, 3, 32), (1, 1, 10)]
    assert [L["p"] for L in convs] == [(2, 1), (2, 1), (1, 1), (1, 1), (1, 1)]
    assert [L["relu"] for L in convs] == [1, 1, 1, 1, 0]
    assert model["layers"][-1]["type"] == cube_import.T_SOFTMAX
    # 171 944 bytes of float32 weights and biases in the reference's blob
    assert sum(L["w"].size + L["b"].size for L in convs) * 4 == 171944


def test_restatement_pins_layout(model, golden):
    """The edison wav's host-flow features: class 0 ("edison") with p > 0.9; the kh / kw-swapped reading of the same weights does not."""
    x = golden["net_in_edison"][None]
    r = fnet_host.run64(model, x)
    assert r["argmax"][0] == 0 and r["probs"][0, 0] > 0.9
    np.testing.assert_allclose(r["probs"][0], golden["probs_edison"], rtol=0, atol=1e-12)
    s = fnet_host.run64(fnet_host.swapped(model), x)
    assert not (s["argmax"][0] == 0 and s["probs"][0, 0] > 0.9)


def _synth(specs, in_shape=(20, 9, 1), **kw):
    return cube_synth.cube_sources(in_shape, specs, seed=5, **kw)


def test_synth_network_round_trip():
    """A network in the importer's input format at another geometry, with every supported layer kind: strides, pools of 2 and 4
    elements, a ReLU folded into the dense before it, non-square kernels."""
    specs = [("conv", 6, (3, 2), (1, 1), (2, 2), 1), ("conv", 20, (2, 3), (2, 1), (1, 1), 0), ("dense", 12), ("relu",), ("dense", 5), ("softmax",)]
    net_c, data_c = _synth(specs)
    m = cube_import.read_blob(cube_import.build_blob(cube_import.convert(cube_import.parse_net_c(net_c), cube_import.parse_data_c(data_c))))
    convs = fnet_host.conv_records(m)
    assert [L["out"] for L in convs] == [(9, 4, 6), (4, 2, 20), (1, 1, 12), (1, 1, 5)]
    assert [L["relu"] for L in convs] == [1, 0, 1, 0] and [L["k"] for L in convs[:2]] == [(3, 2), (2, 3)]
    # the weights come back in [out][kh][kw][in], the order the generator drew them in
    rng = np.random.default_rng(5)
    w0 = rng.normal(0, 1.0 / np.sqrt(6), (6, 3, 2, 1)).astype(np.float32)
    assert np.array_equal(convs[0]["w"], w0)
    r = fnet_host.run64(m, np.random.default_rng(1).normal(0, 10, (3, 180)))
    np.testing.assert_allclose(r["probs"].sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("case,msg", [
    ("groups", "grouped convolution"),
    ("tanh", "nonlinearity nl_func_tanh_array_f32"),
    ("avgpool", "max pool only"),
    ("pool3", "pool window"),
    ("sigmoid_layer", "forward_sigmoid is not supported"),
    ("softmax_mid", "softmax is only supported as the last layer"),
    ("quantised", "only float32 networks"),
    ("softmax_map", "softmax over a 9x7 map"),
])
def test_unsupported_layer_refused(case, msg):
    specs = [("conv", 4, (3, 3), (1, 1), (2, 1), 1), ("dense", 5), ("softmax",)]
    ov = {}
    if case == "groups":
        ov = {"layer_0": dict(fields=[".groups = 2", ".nl_func = NULL"])}
    elif case == "tanh":
        ov = {"layer_0": dict(fields=[".groups = 1", ".nl_func = nl_func_tanh_array_f32"])}
    elif case == "avgpool":
        ov = {"layer_0": dict(fields=[".groups = 1", ".pool_size = AI_SHAPE_2D_INIT(1, 2)", ".pool_stride = AI_SHAPE_2D_INIT(1, 2)",
                                      ".pool_func = pool_func_ap_array_f32"])}
    elif case == "pool3":
        specs = [("conv", 4, (3, 3), (1, 1), (3, 1), 1), ("dense", 5), ("softmax",)]
    elif case == "sigmoid_layer":
        specs = [("conv", 4, (3, 3), (1, 1), (2, 1), 1), ("relu",), ("dense", 5), ("softmax",)]
        ov = {"layer_1": dict(kind=("NL_TYPE", "nl", "forward_sigmoid"))}
    elif case == "softmax_mid":
        specs = [("conv", 4, (3, 3), (1, 1), (2, 1), 1), ("softmax",), ("dense", 5), ("softmax",)]
    elif case == "softmax_map":
        specs = [("conv", 4, (3, 3), (1, 1), (2, 1), 1), ("softmax",)]
    net_c, data_c = _synth(specs, overrides=ov)
    if case == "quantised":
        net_c = net_c.replace("layer_0_weights_array, AI_ARRAY_FORMAT_FLOAT", "layer_0_weights_array, AI_ARRAY_FORMAT_S8")
    with pytest.raises(cube_import.CubeImportError) as e:
        cube_import.convert(cube_import.parse_net_c(net_c), cube_import.parse_data_c(data_c))
    assert msg in str(e.value)
    if case not in ("quantised",):
        assert "layer_" in str(e.value)  # the message names the layer


def test_cli_refuses_with_message(tmp_path, capsys):
    net_c, data_c = _synth([("conv", 4, (3, 3), (1, 1), (1, 1), 1), ("dense", 5)])
    (tmp_path / "n.c").write_text(net_c)
    (tmp_path / "n_data.c").write_text(data_c)
    from edison_amd.cube_import import main
    assert main(["import_cube", str(tmp_path / "n.c"), str(tmp_path / "n_data.c"), str(tmp_path / "o.ednf")]) == 1
    assert "softmax" in capsys.readouterr().err and not (tmp_path / "o.ednf").exists()


def test_kernel_compiles_without_scratch(tmp_path):
    """fnet_kernels.hip for gfx950: no scratch memory, the f32-input MFMA in the code object, and f32 subnormals kept by both kernels
    (float_denorm_mode_32 3: no build flag flushes them; tests/fnet_host.py models the kernel without flushing)."""
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    src = os.path.join(ROOT, "edison_amd", "csrc", "fnet_kernels.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize", "-O3", "--cuda-device-only", "-S", src, "-o",
                        str(tmp_path / "f.s"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(scratch) == 2 and all(v == 0 for v in scratch), r.stderr
    asm = (tmp_path / "f.s").read_text()
    assert "v_mfma_f32_16x16x4_f32" in asm or "v_mfma_f32_16x16x4f32" in asm
    modes = re.findall(r"\.amdhsa_float_denorm_mode_32 (\d+)", asm)
    assert modes == ["3", "3"], modes

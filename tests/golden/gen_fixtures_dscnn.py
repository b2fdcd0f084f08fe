#!/usr/bin/env python3
"""Golden vectors for DW_Conv2D and AvgPool on the general network path, produced by the reference's own code.

Modelled on gen_fixtures_net.py (whose header format, reference loader and input recipe it imports): this script writes
model headers of its own in NNoM's generated format (random int8 parameters: the DATA is ours), compiles the REFERENCE
NNoM 0.3.0 + CMSIS-NN around each of them with the committed recipe `make -C oracle alt`, handing it the two layers'
sources on make's command line (a variable given there overrides the Makefile's REF_SRC):

    nnom_dw_conv2d.c, nnom_avgpool.c, arm_depthwise_separable_conv_HWC_q7_nonsquare.c

and records what model_run() produces for seeded inputs, layer by layer. Committed results:

    tests/golden/alt_models/dscnn_<name>.h      the generated headers (input of tools/import_weights_h.py)
    tests/golden/dscnn_golden.npz               in_<name>, acts_<name> (all compute-layer outputs back to back), argmax_<name>

Graphs (inputs no larger than 12 x 10; channel counts 2, 6, 16, 18, 34, 66 sit either side of a dword of channels and of
the matrix-core path's 16-channel chunk):

  kws     a DS-CNN as ML-KWS draws it: Conv2D, 3 x (DW_Conv2D + 1x1 Conv2D), AvgPool over the whole map, Dense, Softmax.
          DW kernels 3x3 SAME, 5x1 SAME, 3x3 VALID at stride (2,1); the last pointwise layer has no ReLU, so the pool
          sums negative values on a non-square map (local_avepool_q7_HWC)
  edges   2 and 6 channels: a 1x1 DW kernel, an even kernel under SAME at stride (2,2) (windows overhang the far edge
          only), an AvgPool with a non-square kernel under SAME on a non-square map (windows cut on three sides), a DW
          kernel spanning the whole map; no Softmax
  square  a square map: AvgPool goes to arm_avepool_q7_HWC, which is handed kernel.w / pad.w / stride.w for BOTH axes
          (nnom_avgpool.c:76-86) -- with a (2,3) kernel under SAME that is not the window the header states; then a
          2x2/2 VALID pool on the square map and a DW kernel equal to the map under SAME

Run here only (needs the reference tree and gcc):   python3 tests/golden/gen_fixtures_dscnn.py
"""
import glob
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from edison_amd import nnom_import as imp         # noqa: E402
import gen_fixtures_net as gnet                   # noqa: E402
import dscnn_ref                                  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
NNOM = os.path.join(REF, "firmware", "src", "ai", "nnom")
CMSIS_NN = os.path.join(REF, "firmware", "src", "lib", "CMSIS", "NN", "Source")

# layer: ("conv", out_ch, (kh, kw), (sh, sw), pad, relu) | ("dw", (kh, kw), (sh, sw), pad, relu) | ("avg", (kh, kw), (sh, sw), pad) |
#        ("pool", ...) | ("dense", out, relu) | ("softmax",)
MODELS = {
    "kws": ((12, 10, 1), [("conv", 16, (3, 3), (2, 2), "SAME", 1),
                          ("dw", (3, 3), (1, 1), "SAME", 1), ("conv", 18, (1, 1), (1, 1), "VALID", 1),
                          ("dw", (5, 1), (1, 1), "SAME", 1), ("conv", 34, (1, 1), (1, 1), "VALID", 1),
                          ("dw", (3, 3), (2, 1), "VALID", 1), ("conv", 66, (1, 1), (1, 1), "VALID", 0),
                          ("avg", (2, 3), (2, 3), "VALID"), ("dense", 10, 0), ("softmax",)]),
    "edges": ((7, 5, 2), [("dw", (1, 1), (1, 1), "VALID", 0), ("conv", 6, (1, 1), (1, 1), "VALID", 0),
                          ("dw", (2, 2), (2, 2), "SAME", 0), ("avg", (3, 2), (1, 1), "SAME"),
                          ("dw", (4, 3), (1, 1), "VALID", 1), ("dense", 5, 0)]),
    "square": ((8, 8, 2), [("dw", (3, 3), (1, 1), "SAME", 0), ("avg", (2, 3), (1, 1), "SAME"),
                           ("avg", (2, 2), (2, 2), "VALID"), ("dw", (4, 4), (2, 2), "SAME", 0),
                           ("dense", 4, 0), ("softmax",)]),
}
N_INPUTS = 24


def ref_sources():
    """oracle/Makefile's REF_SRC (same files, same order) plus what the two new layers need."""
    layers = ["activation", "baselayer", "conv2d", "dense", "input", "output", "maxpool", "softmax", "dw_conv2d", "avgpool"]
    conv = os.path.join(CMSIS_NN, "ConvolutionFunctions")
    return (sorted(glob.glob(os.path.join(NNOM, "src", "core", "*.c"))) +
            [os.path.join(NNOM, "src", "layers", "nnom_%s.c" % n) for n in layers] +
            [os.path.join(NNOM, "src", "backends", "nnom_local.c")] +
            [os.path.join(conv, "arm_convolve_HWC_q7_%s.c" % n) for n in ("basic", "basic_nonsquare", "fast", "fast_nonsquare", "RGB")] +
            [os.path.join(conv, "arm_convolve_1x1_HWC_q7_fast_nonsquare.c"),
             os.path.join(conv, "arm_depthwise_separable_conv_HWC_q7_nonsquare.c"),
             os.path.join(CMSIS_NN, "FullyConnectedFunctions", "arm_fully_connected_q7_opt.c"),
             os.path.join(CMSIS_NN, "ActivationFunctions", "arm_relu_q7.c"),
             os.path.join(CMSIS_NN, "ActivationFunctions", "arm_nn_activations_q7.c"),
             os.path.join(CMSIS_NN, "SoftmaxFunctions", "arm_softmax_q7.c"),
             os.path.join(CMSIS_NN, "PoolingFunctions", "arm_pool_q7_HWC.c"),
             os.path.join(CMSIS_NN, "NNSupportFunctions", "arm_nntables.c")])


def write_header(name, in_shape, layers, rng):
    """A model header in the format NNoM's generator emits; the statements of the two new layers as nnom_layers.h declares them."""
    h, w, c = in_shape
    defs, decls, body = [], [], []
    count = {}
    idx = 0
    body.append("\tlayer[0] = Input(shape(%d, %d, %d), nnom_input_data);" % in_shape)

    def arr(v):
        return "{" + ", ".join(str(int(t)) for t in v) + "}"

    def tensors(tag, wn, bn, shifts):
        wv = rng.integers(-90, 91, wn)
        bv = rng.integers(-100, 101, bn)
        rs, bl = int(rng.integers(*shifts)), int(rng.integers(0, 6))
        up = tag.upper()
        defs.append("#define %s_KERNEL_0 %s\n\n#define %s_BIAS_0 %s\n" % (up, arr(wv), up, arr(bv)))
        defs.append("#define %s_OUTPUT_RSHIFT (%d)\n#define %s_BIAS_LSHIFT (%d)\n" % (up, rs, up, bl))
        decls.append("static const int8_t %s_weights[] = %s_KERNEL_0;" % (tag, up))
        decls.append("static const nnom_weight_t %s_w = { (const void*)%s_weights, %s_OUTPUT_RSHIFT};" % (tag, tag, up))
        decls.append("static const int8_t %s_bias[] = %s_BIAS_0;" % (tag, up))
        decls.append("static const nnom_bias_t %s_b = { (const void*)%s_bias, %s_BIAS_LSHIFT};" % (tag, tag, up))

    def tag_of(kind):
        count[kind] = count.get(kind, 0) + 1
        return "%s_%d" % (kind, count[kind])

    def hook(text, relu=0):
        nonlocal idx
        idx += 1
        body.append("\tlayer[%d] = model.hook(%s, layer[%d]);" % (idx, text, idx - 1))
        if relu:
            idx += 1
            body.append("\tlayer[%d] = model.active(act_relu(), layer[%d]);" % (idx, idx - 1))

    for L in layers:
        if L[0] == "conv":
            _, oc, (kh, kw), (sh, sw), pad, relu = L
            tag = tag_of("conv2d")
            tensors(tag, oc * kh * kw * c, oc, (6, 10))
            hook("Conv2D(%d, kernel(%d, %d), stride(%d, %d), PADDING_%s, &%s_w, &%s_b)" % (oc, kh, kw, sh, sw, pad, tag, tag), relu)
            h, w, c = gnet.out_dim(h, kh, sh, pad == "SAME"), gnet.out_dim(w, kw, sw, pad == "SAME"), oc
        elif L[0] == "dw":
            _, (kh, kw), (sh, sw), pad, relu = L
            tag = tag_of("depthwise_conv2d")
            # few taps per output: shifts small enough that full-scale inputs saturate at both ends, large enough that quiet ones do not
            tensors(tag, kh * kw * c, c, (4, 8))
            hook("DW_Conv2D(1, kernel(%d, %d), stride(%d, %d), PADDING_%s, &%s_w, &%s_b)" % (kh, kw, sh, sw, pad, tag, tag), relu)
            h, w = gnet.out_dim(h, kh, sh, pad == "SAME"), gnet.out_dim(w, kw, sw, pad == "SAME")
        elif L[0] in ("avg", "pool"):
            _, (kh, kw), (sh, sw), pad = L
            hook("%s(kernel(%d, %d), stride(%d, %d), PADDING_%s)" % ("AvgPool" if L[0] == "avg" else "MaxPool", kh, kw, sh, sw, pad))
            h, w = gnet.out_dim(h, kh, sh, pad == "SAME"), gnet.out_dim(w, kw, sw, pad == "SAME")
        elif L[0] == "dense":
            _, no, relu = L
            tag = tag_of("dense")
            tensors(tag, no * h * w * c, no, (6, 10))
            hook("Dense(%d, &%s_w, &%s_b)" % (no, tag, tag), relu)
            h, w, c = 1, 1, no
        elif L[0] == "softmax":
            hook("Softmax()")
    n_out = h * w * c
    hook("Output(shape(%d,1,1), nnom_output_data)" % n_out)
    text = ("/* generated by tests/golden/gen_fixtures_dscnn.py: model 'dscnn_%s', random int8 parameters (seeded) */\n"
            "#include \"nnom.h\"\n\n" % name + "\n".join(defs) + "\n/* weights for each layer */\n" + "\n".join(decls) +
            "\n\n/* nnom model */\nstatic int8_t nnom_input_data[%d];\nstatic int8_t nnom_output_data[%d];\n"
            "static nnom_model_t* nnom_model_create(void)\n{\n\tstatic nnom_model_t model;\n\tnnom_layer_t* layer[%d];\n\n"
            "\tnew_model(&model);\n\n" % (in_shape[0] * in_shape[1] * in_shape[2], n_out, idx + 1) + "\n".join(body) +
            "\n\tmodel_compile(&model, layer[0], layer[%d]);\n\treturn &model;\n}\n" % idx)
    with open(os.path.join(HERE, "alt_models", "dscnn_%s.h" % name), "w") as f:
        f.write(text)
    # the reference shim includes "kws_nnom/weights.h": give the compiler a scratch include directory of that shape
    d = os.path.join(ROOT, "oracle", "_ref", "alt_src", "dscnn_" + name)
    os.makedirs(os.path.join(d, "kws_nnom"), exist_ok=True)
    with open(os.path.join(d, "kws_nnom", "weights.h"), "w") as f:
        f.write(text)
    return d


def main():
    out = {}
    for k, (name, (in_shape, layers)) in enumerate(MODELS.items()):
        rng = np.random.default_rng(900 + k)
        alt_dir = write_header(name, in_shape, layers, rng)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "alt", "ALT_DIR=" + alt_dir, "ALT_NAME=dscnn_" + name,
                               "REF=" + REF, "REF_SRC=" + " ".join(ref_sources())])
        n_in = in_shape[0] * in_shape[1] * in_shape[2]
        x = rng.integers(-128, 128, (N_INPUTS, n_in)).astype(np.int8)
        x[0] = 0
        x[1] = 127
        x[2] = -128
        x[3:8] = rng.integers(-20, 21, (5, n_in))                                   # quiet inputs: unsaturated layers
        acts = gnet.reference_layers(os.path.join(ROOT, "oracle", "_ref", "alt_dscnn_%s.so" % name), x)
        # the importer + the numpy restatement must reproduce the reference before the vectors are worth committing
        with open(os.path.join(HERE, "alt_models", "dscnn_%s.h" % name)) as f:
            shape, parsed = imp.parse_weights_h(f.read())
        blob = imp.build_blob(shape, parsed)
        mine = dscnn_ref.run(blob, x)
        cat = np.concatenate(mine["acts"], axis=1)
        assert cat.shape == acts.shape, (name, cat.shape, acts.shape)
        assert np.array_equal(cat, acts), "%s: tests/dscnn_ref.py differs from the reference NNoM build" % name
        out["in_" + name] = x
        out["acts_" + name] = acts
        out["argmax_" + name] = np.argmax(acts[:, -mine["acts"][-1].shape[1]:], axis=1).astype(np.int32)   # first maximum (nnom_utils.c:275-284)
        print("%-8s input %s, %d bytes of layer outputs per input, numpy restatement == reference" % (name, in_shape, acts.shape[1]))
    np.savez_compressed(os.path.join(HERE, "dscnn_golden.npz"), **out)
    print("wrote tests/golden/dscnn_golden.npz")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for branching graphs (Add, Sub, Mult, Concat) on the general network path, produced by the reference's own code.

Modelled on gen_fixtures_dscnn.py (whose source list and reference loader it reuses): this script writes model headers of its
own in NNoM's generated format (random int8 parameters: the DATA is ours; the graph statements as nnom.h:283-284 and
nnom_layers.h declare them: model.hook from any earlier layer, model.merge, model.mergex, model.active on a merge layer),
compiles the REFERENCE NNoM 0.3.0 + CMSIS-NN around each of them with the committed recipe `make -C oracle alt`, handing it on
make's command line, beside gen_fixtures_dscnn.py's list,

    nnom_matrix.c, nnom_concat.c, CMSIS-DSP's arm_add_q7.c, arm_sub_q7.c, arm_mult_q7.c

and records what model_run() produces for seeded inputs, layer by layer. model_run() walks a branching graph in the order
compile_layers found it (depth first along the hooks), not in the order of the header's layer[] indices: every captured
tensor is matched to the record of tests/res_ref.py that produced the same bytes, and the vectors are stored in record order.

That holds for `cat`. A graph with Add, Sub or Mult does not get through the reference's model_compile(): the three layers
build with default_build (nnom_baselayer.c), which sets the tensor of the FIRST input only, and tensor_mem_set (nnom.c:841)
then writes through the second input's NULL tensor. For `kws` and `edges` the vectors are therefore what tests/res_ref.py
computes, after every merge step of every record has been checked against the reference's own routine, called directly in
the compiled reference build on the very tensors of the graph: arm_add_q7 / arm_sub_q7 / arm_mult_q7 at shift 0,
local_add_q7 / local_sub_q7 / local_mult_q7 otherwise; the order in which add_run combines a third input with the output
(nnom_matrix.c:123-137) is restated from the source. The single-input layers between them are run by restatements that
gen_fixtures_net.py and gen_fixtures_dscnn.py pin to model_run().

    tests/golden/alt_models/res_<name>.h      the generated headers (input of tools/import_weights_h.py)
    tests/golden/res_golden.npz               in_<name>, acts_<name> (all record outputs back to back), argmax_<name>

Graphs (12 x 10 x 1 inputs, 24 each; at most 16 NNoM layers each, which is what the reference shim captures):

  kws    res8-shaped: a conv to 18 channels, two residual blocks (conv, conv, Add(0) of the block input, ReLU tail) with a MaxPool
         between them, AvgPool over the whole map, Dense, Softmax
  edges  6 and 34 channels: a skip held across a MaxPool and a DW_Conv2D into Sub(1); Add(2) over three inputs with a ReLU tail;
         Mult(5) of a layer with itself; Mult(0) and Sub(0) (arm_mult_q7, arm_sub_q7); no Softmax
  cat    an inception block: a 1x1, a 3x3 SAME and a pool branch of 5 channels each, Concat(-1) to 15 channels, a second
         Concat(3) of two inputs to 30 with a ReLU tail, a conv, Dense, Softmax. The branches have EQUAL channel counts: the
         reference's concat_build / concat_run size and copy every input by the first one's channels (nnom_concat.c:95-103,
         197-214), so with unequal ones it computes no concatenation, and the importer refuses such a graph.
  pool   two 3x3 convolutions of one stem, each behind a MaxPool, then Add(0) with a ReLU tail, Dense. The second convolution's pool is
         stored by the convolution's own pass of the fused kernel while the stem is still being read: the held areas must not share.
  cat2   two 1x1 convolutions of one stem (they agree on its layout, so the fused kernel takes the graph), Concat(-1) with a ReLU
         tail, a second Concat(3), Mult(2) of a convolution and its input, Dense, Softmax; small maps, several inputs per wave.

Run here only (needs the reference tree and gcc):   python3 tests/golden/gen_fixtures_res.py
"""
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
import gen_fixtures_dscnn as gds                  # noqa: E402
import res_ref                                    # noqa: E402

REF = gds.REF
CMSIS_DSP = os.path.join(REF, "firmware", "src", "lib", "CMSIS", "DSP", "Source", "BasicMathFunctions")

# (layer, sources): sources index this list, -1 is the network input.
# layer: ("conv", out_ch, (kh, kw), (sh, sw), pad, relu) | ("dw", (kh, kw), (sh, sw), pad, relu) | ("avg" | "pool", (kh, kw), (sh, sw), pad) |
#        ("dense", out, relu) | ("softmax",) | ("add" | "sub" | "mult", shift, relu) | ("concat", axis, relu)
MODELS = {
    "kws": ((12, 10, 1), [(("conv", 18, (3, 3), (1, 1), "SAME", 0), [-1]),       # no ReLU: the first Add can clamp at -128 too
                          (("conv", 18, (3, 3), (1, 1), "SAME", 1), [0]), (("conv", 18, (3, 3), (1, 1), "SAME", 0), [1]),
                          (("add", 0, 1), [2, 0]),
                          (("pool", (2, 2), (2, 2), "VALID"), [3]),
                          (("conv", 18, (3, 3), (1, 1), "SAME", 1), [4]), (("conv", 18, (3, 3), (1, 1), "SAME", 0), [5]),
                          (("add", 0, 1), [6, 4]),
                          (("avg", (6, 5), (6, 5), "VALID"), [7]), (("dense", 10, 0), [8]), (("softmax",), [9])]),
    "edges": ((12, 10, 1), [(("conv", 6, (3, 3), (1, 1), "SAME", 0), [-1]),
                            (("pool", (3, 3), (1, 1), "SAME"), [0]), (("dw", (3, 3), (1, 1), "SAME", 0), [1]),
                            (("sub", 1, 0), [2, 0]),
                            (("add", 2, 1), [3, 0, 2]),
                            (("mult", 5, 0), [4, 4]),
                            (("conv", 34, (1, 1), (1, 1), "VALID", 1), [5]), (("conv", 34, (3, 3), (1, 1), "SAME", 0), [6]),
                            (("mult", 0, 0), [7, 6]),
                            (("sub", 0, 0), [8, 6]),
                            (("pool", (2, 2), (2, 2), "VALID"), [9]), (("dense", 7, 0), [10])]),
    "cat": ((12, 10, 1), [(("conv", 5, (3, 3), (2, 2), "SAME", 0), [-1]),
                          (("conv", 5, (1, 1), (1, 1), "VALID", 1), [0]), (("conv", 5, (3, 3), (1, 1), "SAME", 0), [0]),
                          (("pool", (3, 3), (1, 1), "SAME"), [0]),
                          (("concat", -1, 0), [1, 2, 3]),
                          (("conv", 15, (1, 1), (1, 1), "VALID", 0), [4]),
                          (("concat", 3, 1), [4, 5]),
                          (("conv", 8, (3, 3), (1, 1), "VALID", 1), [6]), (("dense", 6, 0), [7]), (("softmax",), [8])]),
    "pool": ((12, 10, 1), [(("conv", 16, (3, 3), (1, 1), "SAME", 0), [-1]),
                           (("conv", 16, (3, 3), (1, 1), "SAME", 0), [0]), (("conv", 16, (3, 3), (1, 1), "SAME", 0), [0]),
                           (("pool", (2, 2), (2, 2), "VALID"), [2]),       # fused into the convolution in front: stored while that one reads record 0
                           (("pool", (2, 2), (2, 2), "VALID"), [1]),
                           (("add", 0, 1), [3, 4]),
                           (("dense", 5, 0), [5])]),
    "cat2": ((12, 10, 1), [(("conv", 8, (3, 3), (2, 2), "SAME", 0), [-1]),
                           (("conv", 6, (1, 1), (1, 1), "VALID", 1), [0]), (("conv", 6, (1, 1), (1, 1), "VALID", 0), [0]),
                           (("concat", -1, 1), [1, 2]),
                           (("conv", 12, (1, 1), (1, 1), "VALID", 0), [3]),
                           (("concat", 3, 0), [3, 4]),
                           (("conv", 24, (1, 1), (1, 1), "VALID", 0), [5]),
                           (("mult", 2, 0), [6, 5]),
                           (("dense", 6, 0), [7]), (("softmax",), [8])]),
}
N_INPUTS = 24


def ref_sources():
    layers = os.path.join(gds.NNOM, "src", "layers")
    return gds.ref_sources() + [os.path.join(layers, "nnom_matrix.c"), os.path.join(layers, "nnom_concat.c")] + \
        [os.path.join(CMSIS_DSP, "arm_%s_q7.c" % n) for n in ("add", "sub", "mult")]


def write_header(name, in_shape, spec, rng):
    defs, decls, body = [], [], []
    count = {}
    idx = 0
    hdr = {-1: 0}        # spec index -> header layer[] index of the tensor (behind its ReLU statement where it has one)
    shapes = {-1: in_shape}
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

    def emit(stmt, relu):
        nonlocal idx
        idx += 1
        body.append("\tlayer[%d] = %s;" % (idx, stmt))
        if relu:
            idx += 1
            body.append("\tlayer[%d] = model.active(act_relu(), layer[%d]);" % (idx, idx - 1))
        return idx

    for i, (L, src) in enumerate(spec):
        h, w, c = shapes[src[0]]
        at = "layer[%d]" % hdr[src[0]]
        if L[0] == "conv":
            _, oc, (kh, kw), (sh, sw), pad, relu = L
            tag = tag_of("conv2d")
            tensors(tag, oc * kh * kw * c, oc, (6, 10))
            hdr[i] = emit("model.hook(Conv2D(%d, kernel(%d, %d), stride(%d, %d), PADDING_%s, &%s_w, &%s_b), %s)"
                          % (oc, kh, kw, sh, sw, pad, tag, tag, at), relu)
            shapes[i] = (gnet.out_dim(h, kh, sh, pad == "SAME"), gnet.out_dim(w, kw, sw, pad == "SAME"), oc)
        elif L[0] == "dw":
            _, (kh, kw), (sh, sw), pad, relu = L
            tag = tag_of("depthwise_conv2d")
            tensors(tag, kh * kw * c, c, (4, 8))
            hdr[i] = emit("model.hook(DW_Conv2D(1, kernel(%d, %d), stride(%d, %d), PADDING_%s, &%s_w, &%s_b), %s)"
                          % (kh, kw, sh, sw, pad, tag, tag, at), relu)
            shapes[i] = (gnet.out_dim(h, kh, sh, pad == "SAME"), gnet.out_dim(w, kw, sw, pad == "SAME"), c)
        elif L[0] in ("avg", "pool"):
            _, (kh, kw), (sh, sw), pad = L
            hdr[i] = emit("model.hook(%s(kernel(%d, %d), stride(%d, %d), PADDING_%s), %s)"
                          % ("AvgPool" if L[0] == "avg" else "MaxPool", kh, kw, sh, sw, pad, at), 0)
            shapes[i] = (gnet.out_dim(h, kh, sh, pad == "SAME"), gnet.out_dim(w, kw, sw, pad == "SAME"), c)
        elif L[0] == "dense":
            _, no, relu = L
            tag = tag_of("dense")
            tensors(tag, no * h * w * c, no, (6, 10))
            hdr[i] = emit("model.hook(Dense(%d, &%s_w, &%s_b), %s)" % (no, tag, tag, at), relu)
            shapes[i] = (1, 1, no)
        elif L[0] == "softmax":
            hdr[i] = emit("model.hook(Softmax(), %s)" % at, 0)
            shapes[i] = (h, w, c)
        elif L[0] in ("add", "sub", "mult"):
            _, shift, relu = L
            tag = tag_of(L[0]).upper() + "_OUTPUT_SHIFT"
            defs.append("#define %s (%d)\n" % (tag, shift))          # a macro, as the generator writes the other shifts
            ins = ", ".join("layer[%d]" % hdr[s] for s in src)
            call = "%s(%s)" % (L[0].capitalize(), tag)
            hdr[i] = emit("model.merge(%s, %s)" % (call, ins) if len(src) == 2 else "model.mergex(%s, %d, %s)" % (call, len(src), ins), relu)
            shapes[i] = (h, w, c)
        elif L[0] == "concat":
            _, axis, relu = L
            ins = ", ".join("layer[%d]" % hdr[s] for s in src)
            hdr[i] = emit("model.mergex(Concat(%d), %d, %s)" % (axis, len(src), ins), relu)
            shapes[i] = (h, w, c * len(src))
    n_out = int(np.prod(shapes[len(spec) - 1]))
    emit("model.hook(Output(shape(%d,1,1), nnom_output_data), layer[%d])" % (n_out, hdr[len(spec) - 1]), 0)
    text = ("/* generated by tests/golden/gen_fixtures_res.py: model 'res_%s', random int8 parameters (seeded) */\n"
            "#include \"nnom.h\"\n\n" % name + "\n".join(defs) + "\n/* weights for each layer */\n" + "\n".join(decls) +
            "\n\n/* nnom model */\nstatic int8_t nnom_input_data[%d];\nstatic int8_t nnom_output_data[%d];\n"
            "static nnom_model_t* nnom_model_create(void)\n{\n\tstatic nnom_model_t model;\n\tnnom_layer_t* layer[%d];\n\n"
            "\tnew_model(&model);\n\n" % (in_shape[0] * in_shape[1] * in_shape[2], n_out, idx + 1) + "\n".join(body) +
            "\n\tmodel_compile(&model, layer[0], layer[%d]);\n\treturn &model;\n}\n" % idx)
    with open(os.path.join(HERE, "alt_models", "res_%s.h" % name), "w") as f:
        f.write(text)
    d = os.path.join(ROOT, "oracle", "_ref", "alt_src", "res_" + name)
    os.makedirs(os.path.join(d, "kws_nnom"), exist_ok=True)
    with open(os.path.join(d, "kws_nnom", "weights.h"), "w") as f:
        f.write(text)
    return d


def coverage(name, blob, mine):
    """Each clamp direction of the arithmetic merges and the ReLU tail of a merge must be met, or the vectors pin nothing."""
    _, recs, _ = res_ref.net_ref.parse_blob(blob)
    src = res_ref.sources(blob)
    hi = lo = relu = False
    for i, v in enumerate(recs):
        if v[0] not in (res_ref.T_ADD, res_ref.T_SUB, res_ref.T_MULT, res_ref.T_CONCAT):
            continue
        ins = [mine["acts"][r].astype(np.int32) for r in src[i]]
        if v[0] != res_ref.T_CONCAT:
            # the whole chain, step by step as add_run takes it: (input 0, input 1), then (input k, the output so far)
            out = None
            for k in range(1, len(ins)):
                a, b = (ins[0], ins[1]) if k == 1 else (ins[k], out)
                r = a + b if v[0] == res_ref.T_ADD else a - b if v[0] == res_ref.T_SUB else a * b
                r = (r >> 7 if v[0] == res_ref.T_MULT else r) if v[7] == 0 else (r + (1 << (v[7] - 1))) >> v[7]
                hi |= bool((r > 127).any())
                lo |= bool((r < -128).any())
                out = np.clip(r, -128, 127)
            if v[8] & 1:
                relu |= bool((out < 0).any())
        elif v[8] & 1:
            relu |= any(bool((a < 0).any()) for a in ins)
    arith = any(v[0] in (res_ref.T_ADD, res_ref.T_SUB, res_ref.T_MULT) for v in recs)
    assert (hi and lo) or not arith, "%s: merges saturate high %s, low %s" % (name, hi, lo)
    assert relu, "%s: no merge's ReLU tail clamps anything" % name


def check_merges(so_path, blob, mine):
    """Every step of every Add / Sub / Mult record against the reference's routine on the same tensors."""
    import ctypes
    lib = ctypes.CDLL(so_path)
    names = {res_ref.T_ADD: "add", res_ref.T_SUB: "sub", res_ref.T_MULT: "mult"}
    _, recs, _ = res_ref.net_ref.parse_blob(blob)
    src = res_ref.sources(blob)
    for i, v in enumerate(recs):
        if v[0] not in names:
            continue

        def ref_step(a, b):
            a, b = np.ascontiguousarray(a, dtype=np.int8), np.ascontiguousarray(b, dtype=np.int8)
            dst = np.zeros_like(a)
            if v[7] == 0:
                getattr(lib, "arm_%s_q7" % names[v[0]])(ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(b.ctypes.data),
                                                        ctypes.c_void_p(dst.ctypes.data), ctypes.c_uint32(a.size))
            else:
                getattr(lib, "local_%s_q7" % names[v[0]])(ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(b.ctypes.data),
                                                          ctypes.c_void_p(dst.ctypes.data), ctypes.c_uint16(v[7]), ctypes.c_uint32(a.size))
            return dst
        ins = [mine["acts"][r] for r in src[i]]
        out = ref_step(ins[0], ins[1])
        assert np.array_equal(out, res_ref.merge2(v[0], v[7], ins[0], ins[1]).astype(np.int8)), "record %d: first step" % i
        for t in ins[2:]:
            nxt = ref_step(t, out)
            assert np.array_equal(nxt, res_ref.merge2(v[0], v[7], t, out).astype(np.int8)), "record %d: later step" % i
            out = nxt
        if v[8] & 1:
            out = np.maximum(out, 0)
        assert np.array_equal(out, mine["acts"][i]), "record %d" % i


def main():
    out = {}
    for k, (name, (in_shape, spec)) in enumerate(MODELS.items()):
        rng = np.random.default_rng(1100 + k)
        alt_dir = write_header(name, in_shape, spec, rng)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "alt", "ALT_DIR=" + alt_dir, "ALT_NAME=res_" + name,
                               "REF=" + REF, "REF_SRC=" + " ".join(ref_sources())])
        n_in = in_shape[0] * in_shape[1] * in_shape[2]
        x = rng.integers(-128, 128, (N_INPUTS, n_in)).astype(np.int8)
        x[0] = 0
        x[1] = 127
        x[2] = -128
        x[3:8] = rng.integers(-20, 21, (5, n_in))                                   # quiet inputs: unsaturated layers
        so = os.path.join(ROOT, "oracle", "_ref", "alt_res_%s.so" % name)
        with open(os.path.join(HERE, "alt_models", "res_%s.h" % name)) as f:
            shape, parsed = imp.parse_weights_h(f.read())
        blob = imp.build_blob(shape, parsed)
        mine = res_ref.run(blob, x)
        assert len(mine["acts"]) == len(spec)
        if any(L[0] in ("add", "sub", "mult") for L, _ in spec):
            check_merges(so, blob, mine)
        else:
            acts = gnet.reference_layers(so, x)
            assert sum(a.shape[1] for a in mine["acts"]) == acts.shape[1], (name, acts.shape)
            # the reference's execution order: every captured tensor is the output of exactly one record
            off, left = 0, list(range(len(spec)))
            while left:
                hit = [i for i in left if np.array_equal(acts[:, off:off + mine["acts"][i].shape[1]], mine["acts"][i])]
                assert hit, "%s: the tensor at byte %d of the reference's dump is no record's output in tests/res_ref.py" % (name, off)
                left.remove(hit[0])
                off += mine["acts"][hit[0]].shape[1]
            assert off == acts.shape[1]
        coverage(name, blob, mine)
        ordered = np.concatenate(mine["acts"], axis=1)                              # == the reference's bytes, in record order
        out["in_" + name] = x
        out["acts_" + name] = ordered
        out["argmax_" + name] = np.argmax(mine["acts"][-1], axis=1).astype(np.int32)  # first maximum (nnom_utils.c:275-284)
        print("%-8s input %s, %d bytes of record outputs per input, numpy restatement == reference" % (name, in_shape, ordered.shape[1]))
    np.savez_compressed(os.path.join(HERE, "res_golden.npz"), **out)
    print("wrote tests/golden/res_golden.npz")


if __name__ == "__main__":
    main()

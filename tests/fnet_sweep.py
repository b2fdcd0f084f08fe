"""The float-network sweep: named networks chosen so that together they take every path of the float32 network kernel
(ed_fnet_kernel, csrc/fnet_kernels.hip) and of its plan (parse() in csrc/edison_fnet.hip), plus blobs the loader must refuse.

Test infrastructure, not a test: tests/test_fnet_sweep_cpu.py checks that the rows cover every path of the restated plan
(fnet_exact.plan) and that each note agrees with it; tests/test_gpu_fnet_sweep.py runs every row on the GPU bit-for-bit against
the host model of the kernel (fnet_exact).

A row is (spec, note). spec: in_shape (h, w, c); layers, each ("conv", out_c, (kh, kw), (sh, sw), (ph, pw), relu) or ("dense", n,
relu) -- a softmax follows the last one --, or synth: cube_synth specs that go through the X-CUBE-AI source format and the importer;
wscale: per conv record, a factor on its N(0, 1 / K) weights; positive: |weights|; bias: "rand" (N(0, 0.1)) or "zero"; sets: the
input sets, utterance i drawn from sets[i % len(sets)]. The note starts with the plan facts it claims, "key=v[,v..]" tokens before
the ';': P, K4 (K % 4), nt (last group's channel tiles), NG (channel groups), batch, layers, n_out."""
import numpy as np

from edison_amd import cube_import

import cube_synth
import fnet_exact

S = 2.0 ** -60

ROWS = {
    # the arithmetic ladder: one dense layer on the input, zero bias, so that a failure points at the instruction first
    "ladder_k4": (dict(in_shape=(1, 4, 1), layers=[("dense", 1, 0)], bias="zero"),
                  "P=1 K4=0 nt=1 NG=1 batch=16 n_out=1; K = 4 -> 1 output: one MFMA, 15 padding channels, softmax of one logit"),
    "ladder_k5": (dict(in_shape=(1, 5, 1), layers=[("dense", 1, 0)], bias="zero"),
                  "P=1 K4=1 nt=1 NG=1 batch=16 n_out=1; K = 5: a second MFMA with 3 padding k lanes"),
    "ladder_k8": (dict(in_shape=(2, 4, 1), layers=[("dense", 2, 0)], bias="zero"),
                  "P=1 K4=0 nt=1 NG=1 batch=16 n_out=2; K = 8: two chained MFMAs"),
    # pool windows, each with conv outputs the pool floor truncates
    "pool21_trunc_h": (dict(in_shape=(11, 6, 1), layers=[("conv", 4, (3, 3), (1, 1), (2, 1), 1), ("dense", 3, 0)]),
                       "P=2,1 K4=1,0 nt=1 NG=1 batch=16; pool (2, 1) over 9 conv rows (one truncated)"),
    "pool12_trunc_w": (dict(in_shape=(6, 11, 1), layers=[("conv", 5, (3, 3), (1, 1), (1, 2), 0), ("dense", 3, 0)]),
                       "P=2,1 K4=1,0 nt=1 NG=1 batch=16; pool (1, 2) over 9 conv columns (one truncated), conv without ReLU"),
    "pool22_trunc_hw": (dict(in_shape=(10, 10, 2), layers=[("conv", 17, (2, 2), (1, 1), (2, 2), 1), ("dense", 4, 0)]),
                        "P=4,1 K4=0 nt=2,1 NG=1 batch=16; pool (2, 2) over a 9 x 9 map (both truncated), 17 channels"),
    "pool41_tail": (dict(in_shape=(13, 4, 1), layers=[("conv", 8, (3, 2), (1, 1), (4, 1), 1), ("dense", 5, 0)]),
                    "P=4,1 K4=2,0 nt=1 NG=1 batch=16; pool (4, 1) over 11 rows (3 truncated), 24 rows per utterance: M-tile tails at P = 4"),
    "pool14_tail": (dict(in_shape=(3, 15, 1), layers=[("conv", 15, (2, 3), (1, 1), (1, 4), 1), ("dense", 6, 0)]),
                    "P=4,1 K4=2 nt=1 NG=1 batch=16; pool (1, 4) over 13 columns (one truncated), 15 channels, 24 rows per utterance"),
    # channel tiles and groups, strides, K % 4, 1 x 1 convs and kernels that span their input
    "inc3_oc64_oc65_s21": (dict(in_shape=(8, 6, 3), layers=[("conv", 64, (1, 1), (1, 1), (1, 1), 1), ("conv", 65, (2, 2), (2, 1), (1, 1), 0),
                                                              ("dense", 7, 0)]),
                           "P=1 K4=3,0 nt=4,1 NG=1,2 batch=4; network input with 3 channels, a 1 x 1 conv to 64 channels (K = 3), stride (2, 1) "
                           "and K = 256 to 65 channels (NG 2, last group 1 tile)"),
    "oc130_s12": (dict(in_shape=(3, 8, 2), layers=[("conv", 130, (2, 3), (1, 2), (1, 1), 1), ("dense", 10, 0)]),
                  "P=1 K4=0 nt=1 NG=3,1 batch=16; stride (1, 2), 130 channels: 9 tiles in 3 groups"),
    "oc40_s32_span_h": (dict(in_shape=(14, 9, 1), layers=[("conv", 40, (3, 3), (3, 2), (1, 1), 1), ("conv", 16, (4, 1), (1, 1), (1, 1), 1),
                                                          ("dense", 9, 0)]),
                        "P=1 K4=1,0 nt=3,1 NG=1 batch=16; stride (3, 2), 40 channels (3 tiles), then a (4, 1) kernel over the whole height"),
    "oc16_span_w": (dict(in_shape=(20, 13, 1), layers=[("conv", 16, (3, 13), (1, 1), (2, 1), 1), ("dense", 12, 0)]),
                    "P=2,1 K4=3,0 nt=1 NG=1 batch=16; a (3, 13) kernel over the whole width (K = 39), pool (2, 1)"),
    "n_out_210": (dict(in_shape=(3, 3, 1), layers=[("conv", 12, (2, 2), (1, 1), (1, 1), 1), ("dense", 210, 0)]),
                  "P=1 K4=0 nt=1,2 NG=1,4 batch=16 n_out=210; 210 logits: 14 tiles in 4 groups, last group 2 tiles"),
    # network shapes
    "relu_logits": (dict(in_shape=(4, 4, 2), layers=[("dense", 8, 0), ("dense", 6, 1)], bias="zero", positive=True, sets=["neg", "n1"]),
                    "P=1 K4=0 nt=1 NG=1 batch=16; a dense-only network with ReLU on the logits: positive weights on all-negative inputs give 6 zero logits, "
                    "probs tie, argmax 0"),
    "conv_last_map": (dict(in_shape=(8, 8, 1), layers=[("conv", 6, (3, 3), (1, 1), (2, 2), 1), ("conv", 4, (2, 2), (1, 1), (1, 1), 0)]),
                      "P=4,1 K4=1,0 nt=1 NG=1 batch=16 n_out=16; a conv as the last layer: softmax over its 2 x 2 x 4 map"),
    "layers16": (dict(in_shape=(12, 3, 2), layers=[("conv", 8, (1, 1), (1, 1), (1, 1), 1)]
                      + [("conv", 8, (2, 1) if i % 4 == 0 else (1, 1), (1, 1), (1, 1), i % 2) for i in range(14)] + [("dense", 5, 0)]),
                 "P=1 K4=2,0 nt=1 NG=1 batch=16 layers=16; 16 conv / dense layers, the most the plan holds, ReLU on and off"),
    # batch and LDS
    "batch1_lds_max": (dict(in_shape=(8, 284, 1), layers=[("dense", 16, 0)]),
                       "P=1 K4=0 nt=1 NG=1 batch=1 n_out=16; K = 2272 x 16: the largest weights that load at batch 1, LDS 163 648 bytes"),
    "batch5": (dict(in_shape=(40, 30, 2), layers=[("conv", 4, (3, 3), (1, 1), (1, 1), 1), ("conv", 8, (3, 3), (2, 2), (2, 2), 1), ("dense", 5, 0)]),
               "P=1,4 K4=2,0 nt=1 NG=1 batch=5; a middle batch: 4256 floats of activations per utterance"),
    # the packed weight array: more floats than one pass of the optimiser's step kernel covers on 256 CUs (8 blocks of 256 a CU)
    "dense16_wide": (dict(in_shape=(1, 1, 192), layers=[("dense", 192, (i + 1) % 2) for i in range(15)] + [("dense", 5, 0)]),
                     "P=1 K4=0 nt=4,1 NG=3,1 batch=10 layers=16 n_out=5; fifteen dense 192 -> 192, ReLU on every other one, then 192 -> 5: "
                     "558 928 packed floats, one row per utterance in every record"),
    # subnormal products and partial sums; zero bias so nothing hides them
    "subnormal": (dict(in_shape=(6, 4, 1), layers=[("conv", 16, (2, 2), (1, 1), (1, 1), 0), ("dense", 8, 0)], bias="zero", wscale=[S, 1.0],
                       sets=["tiny", "sub", "n1"]),
                  "P=1 K4=0 nt=1 NG=1 batch=16; normal operands with subnormal products (2^-70 x 2^-60), then subnormal A operands"),
    # through the X-CUBE-AI source format and the importer
    "synth_pool12_relu": (dict(in_shape=(9, 7, 2), synth=[("conv", 20, (2, 2), (1, 1), (1, 2), 1), ("relu",), ("dense", 11), ("relu",), ("dense", 4),
                                                          ("softmax",)]),
                          "P=2,1 K4=0,3 nt=2,1 NG=1 batch=16; imported: pool (1, 2), standalone ReLUs folded into a conv and a dense"),
}

# name -> (blob builder, the loader's code, note): networks the importer never writes
REFUSALS = {}

SETS = ("n1", "n60", "i16", "zero", "neg")


def inputs(name, n, in_n):
    """n inputs [n][in_n] float32 of row `name`: utterance i from set sets[i % len(sets)], fixed seeds."""
    sets = ROWS[name][0].get("sets", SETS)
    rng = np.random.default_rng(sum(map(ord, name)))
    x = np.empty((n, in_n), np.float32)
    for i in range(n):
        s = sets[i % len(sets)]
        g = rng.normal(0, 1, in_n)
        x[i] = dict(n1=g, n60=60 * g, i16=rng.integers(-32768, 32768, in_n), zero=0 * g, neg=-np.abs(30 * g), tiny=g * 2.0 ** -70,
                    sub=g * 2.0 ** -130)[s]
    return x


def _records(in_shape, layers):
    h, w, c = in_shape
    out = []
    for L in layers:
        if L[0] == "dense":
            out.append(dict(type=cube_import.T_CONV, inp=(h, w, c), out=(1, 1, L[1]), k=(h, w), s=(1, 1), p=(1, 1), relu=L[2]))
        else:
            _, oc, (kh, kw), (sh, sw), (ph, pw), relu = L
            oh, ow = ((h - kh) // sh + 1) // ph, ((w - kw) // sw + 1) // pw
            out.append(dict(type=cube_import.T_CONV, inp=(h, w, c), out=(oh, ow, oc), k=(kh, kw), s=(sh, sw), p=(ph, pw), relu=relu))
        h, w, c = out[-1]["out"]
    return out


def model(name):
    """Row `name` -> the cube_import model dict (float32 weights)."""
    spec = ROWS[name][0]
    if "synth" in spec:
        return cube_import.read_blob(blob(name))
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    recs = _records(spec["in_shape"], spec["layers"])
    wscale = spec.get("wscale", [1.0] * len(recs))
    for L, f in zip(recs, wscale):
        oc, (kh, kw), ic = L["out"][2], L["k"], L["inp"][2]
        w = rng.normal(0, 1, (oc, kh, kw, ic)) / np.sqrt(kh * kw * ic)
        L["w"] = ((np.abs(w) if spec.get("positive") else w) * f).astype(np.float32)
        L["b"] = (np.zeros(oc) if spec.get("bias", "rand") == "zero" else rng.normal(0, 0.1, oc)).astype(np.float32)
    last = recs[-1]["out"]
    recs.append(dict(type=cube_import.T_SOFTMAX, inp=last, out=last))
    return dict(in_shape=spec["in_shape"], layers=recs)


def blob(name):
    spec = ROWS[name][0]
    if "synth" in spec:
        net_c, data_c = cube_synth.cube_sources(spec["in_shape"], spec["synth"], seed=sum(map(ord, name)))
        return _import(net_c, data_c)
    return cube_import.build_blob(model(name))


def _import(net_c, data_c):
    net = cube_import.parse_net_c(net_c)
    return cube_import.build_blob(cube_import.convert(net, cube_import.parse_data_c(data_c)))


def path(p):
    """The plan facts a note may claim: sets of per-layer values and the network's scalars."""
    L = p["layers"]
    return dict(P={x["P"] for x in L}, K4={x["K"] % 4 for x in L}, nt={x["nt_last"] for x in L}, NG={x["NG"] for x in L},
                batch={p["batch"]}, layers={p["n_layers"]}, n_out={p["n_out"]})


STEP_PASS = 2048     # floats a CU's 8 blocks of 256 threads cover in one pass of ed_ftrain_step_kernel (ed_launch_ftrain_step)


def w_floats(p):
    """The packed weight array of a plan, in floats: every record's B[k_pad][n_pad], then bias[n_pad]."""
    return sum(L["k_pad"] * L["n_pad"] + L["n_pad"] for L in p["layers"])


def claims(note):
    head = note.split(";")[0].split()
    return {k: {int(v) for v in vs.split(",")} for k, vs in (t.split("=") for t in head)}


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _pack(in_shape, recs, n_out, payload=b""):
    head = cube_import.HDR.pack(cube_import.MAGIC, cube_import.VERSION, len(recs), *in_shape, n_out) + b"\0\0\0\0"
    return head + b"".join(np.asarray(r, "<i4").tobytes() for r in recs) + payload


def _conv_rec(inp, out, k, s, p, relu, k_pad=None, n_pad=None):
    K = k[0] * k[1] * inp[2]
    return [cube_import.T_CONV, *inp, *out, *k, *s, relu, *p, k_pad or (K + 3) // 4 * 4, n_pad or (out[2] + 15) // 16 * 16]


def _sm_rec(shape):
    return [cube_import.T_SOFTMAX, *shape, *shape] + [0] * 9


def _refuse_pool31():
    return _pack((9, 4, 1), [_conv_rec((9, 4, 1), (2, 4, 4), (3, 1), (1, 1), (3, 1), 1), _sm_rec((2, 4, 4))], 32)


def _refuse_17_layers():
    recs = [_conv_rec((4, 4, 2), (4, 4, 2), (1, 1), (1, 1), (1, 1), 1) for _ in range(17)]
    return _pack((4, 4, 2), recs + [_sm_rec((4, 4, 2))], 32)


def _refuse_weights_lds():
    return _pack((1, 2564, 1), [_conv_rec((1, 2564, 1), (1, 1, 16), (1, 2564), (1, 1), (1, 1), 0), _sm_rec((1, 1, 16))], 16)


def _refuse_lds_batch1():
    h, w = 1, 2276
    recs = _records((h, w, 1), [("dense", 16, 0)])
    recs[0]["w"] = np.zeros((16, h, w, 1), np.float32)
    recs[0]["b"] = np.zeros(16, np.float32)
    return cube_import.build_blob(dict(in_shape=(h, w, 1), layers=recs + [dict(type=cube_import.T_SOFTMAX, inp=(1, 1, 16), out=(1, 1, 16))]))


def _refuse_k_pad():
    return _pack((6, 4, 1), [_conv_rec((6, 4, 1), (1, 1, 3), (6, 4), (1, 1), (1, 1), 0, k_pad=28), _sm_rec((1, 1, 3))], 3)


def _refuse_n_pad():
    return _pack((6, 4, 1), [_conv_rec((6, 4, 1), (1, 1, 3), (6, 4), (1, 1), (1, 1), 0, n_pad=32), _sm_rec((1, 1, 3))], 3)


REFUSALS.update({
    "pool31": (_refuse_pool31, fnet_exact.E_NO_IMPL, "a pool window of 3 elements"),
    "layers17": (_refuse_17_layers, fnet_exact.E_NO_IMPL, "17 conv records (18 with the softmax): the header's layer count refuses them; parse()'s in-loop "
                                                  "16-layer check is unreachable, the last record being the softmax"),
    "weights_over_lds": (_refuse_weights_lds, fnet_exact.E_NO_IMPL, "k_pad x n_pad = 2564 x 16 = 41 024 floats > 40 960"),
    "lds_batch1": (_refuse_lds_batch1, fnet_exact.E_NO_IMPL, "2276 x 16 weights fit, with one utterance's activations they do not"),
    "k_pad": (_refuse_k_pad, fnet_exact.E_SIZE, "k_pad 28 for K = 24"),
    "n_pad": (_refuse_n_pad, fnet_exact.E_SIZE, "n_pad 32 for 3 channels"),
})

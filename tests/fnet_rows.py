"""The rows of the float32 network's suites: named networks, their seeded weights, blobs and inputs, and the blobs the loader must
refuse. Test infrastructure, not a test. Three tables, whose row names never collide:

SWEEP: networks chosen so that together they take every path of the float32 network kernel (ed_fnet_kernel,
csrc/fnet_kernels.hip) and of its plan (fnet_plan.plan). tests/test_fnet_sweep_cpu.py checks that the rows cover every path of the
plan and that each note agrees with it; tests/test_gpu_fnet_sweep.py runs every row on the GPU bit for bit against fnet_host.
PAD (section 14b): padded networks ('same' convolutions and pools, .ednf version 2), every row taking a path no other row takes
(pad_facts); tests/test_fnet_pad_cpu.py, tests/test_gpu_fnet_pad.py.
LARGE (section 14c): networks whose layers exceed the LDS (edison_fnet_load_ex, the layer road), covering REQUIRED between them
(large_facts); tests/test_fnet_large_cpu.py, tests/test_gpu_fnet_large.py.

A row is (spec, note). spec: in_shape (h, w, c) and one of
  layers: each ("conv", out_c, (kh, kw), (sh, sw), (ph, pw), relu[, cpad, ppad]) or ("dense", n, relu); a softmax follows the last;
  synth:  cube_synth specs that go through the X-CUBE-AI source format and the importer;
  zoo:    one of kws_keras.get_model's padded architectures (zoo_specs), through the same format;
  arch:   one of train.get_model's architectures at in_shape x classes.
Weights of a `layers` or `arch` row are seeded (seeded(); TABLES gives each table's seed offset and distribution); wscale: per conv
record, a factor on its weights; positive: |weights|; bias: "rand", "zero" or a constant; sets: the input sets, utterance i drawn from
sets[i % len(sets)]; plain (LARGE): the code the plain loader answers (E_NO_IMPL unless stated). A SWEEP note starts with the plan
facts it claims, "key=v[,v..]" tokens before the ';': P, K4 (K % 4), nt (last group's channel tiles), NG (channel groups), batch,
layers, n_out."""
import numpy as np

from edison_amd import cube_import, train

import cube_synth
import fnet_plan
from fnet_host import Z4, conv_records, out_hw
from fnet_plan import E_NO_IMPL, E_SIZE, KC, LDS_BYTES, MB, WAVE_ROWS

S = 2.0 ** -60


def _c(oc, k, s=(1, 1), p=(1, 1), relu=1, cpad=Z4, ppad=Z4):
    return ("conv", oc, k, s, p, relu, cpad, ppad)


SWEEP = {
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


# ---- the zoo: kws_keras.get_model's padded architectures ------------------------------------------------------------------------------
def _same(h, w, k, s):
    (t, b), (l, r) = cube_import.same_pads(h, k[0], s[0]), cube_import.same_pads(w, k[1], s[1])
    return t, l, b, r


def zoo_specs(name, in_shape=(31, 13, 1), n_classes=10):
    """The layers of one of the reference training script's padded sequential architectures at in_shape, as cube_synth.cube_sources specs:
    padding='same' convolutions (ReLU) and MaxPooling2D((2, 2)), 'same' or 'valid', then Dense and Softmax."""
    arch = dict(tiny_conv=[(8, (8, 10), (2, 2), None)],
                medium_embedding_conv=[(16, (8, 8), (2, 2), "same"), (12, (4, 4), (1, 1), None)],
                tiny_embedding_conv=[(8, (8, 10), (2, 2), "same"), (8, (8, 10), (8, 8), None)],
                simple_conv=[(8, (8, 8), (1, 1), "valid")])[name]
    h, w, _ = in_shape
    specs = []
    for oc, k, s, pool in arch:
        cp = _same(h, w, k, s)
        ch, cw = -(-h // s[0]), -(-w // s[1])
        p, pp = ((2, 2), _same(ch, cw, (2, 2), (2, 2)) if pool == "same" else Z4) if pool else ((1, 1), Z4)
        specs.append(("conv", oc, k, s, p, 1, cp, pp))
        h, w = out_hw((h, w), k, s, p, cp, pp)
    return specs + [("dense", n_classes), ("softmax",)]


ZOO = ("tiny_conv", "medium_embedding_conv", "tiny_embedding_conv", "simple_conv")

PAD = {
    "sym3x3": (dict(in_shape=(5, 4, 1), layers=[_c(3, (3, 3), cpad=(1, 1, 1, 1)), ("dense", 3, 0)]),
               "one pad on every side of a 3x3 kernel: every corner and edge window has taps outside"),
    "asym_even": (dict(in_shape=(6, 5, 2), layers=[_c(5, (4, 2), cpad=(1, 0, 2, 1)), ("dense", 4, 0)]),
                  "even kernel extents, four different pads, two input channels (ci runs inside a tap), ReLU"),
    "stride2_same": (dict(in_shape=(7, 6, 1), layers=[_c(4, (3, 3), s=(2, 2), cpad=(1, 0, 1, 1)), ("dense", 3, 0)]),
                     "Keras's 'same' at stride 2: an odd extent pads both ends, an even one only the far end"),
    "top_only": (dict(in_shape=(4, 3, 1), layers=[_c(2, (3, 2), cpad=(2, 0, 0, 0)), ("dense", 3, 0)]),
                 "two rows above and nothing else: swapped axes or swapped ends change the shape or the values"),
    "left_only": (dict(in_shape=(3, 4, 1), layers=[_c(2, (2, 3), cpad=(0, 2, 0, 0)), ("dense", 3, 0)]),
                  "two columns on the left and nothing else"),
    "k_wider_than_input": (dict(in_shape=(4, 3, 2), layers=[_c(3, (2, 5), cpad=(0, 1, 0, 1)), ("dense", 3, 0)]),
                           "a 2x5 kernel over 3 columns: it fits only with the pads, the output is one column wide"),
    "pool22_odd": (dict(in_shape=(6, 4, 1), layers=[_c(4, (2, 2), p=(2, 2), ppad=(0, 0, 1, 1)), ("dense", 3, 0)]),
                   "pool (2, 2) over a 5x3 map padded at the far ends: windows of 4, 2, 2 and 1 present elements"),
    "pool21_tail": (dict(in_shape=(6, 3, 1), layers=[_c(3, (2, 2), p=(2, 1), ppad=(0, 0, 1, 0)), ("dense", 3, 0)]),
                    "pool (2, 1) over 5 rows: the last window has one present element"),
    "pool41_lead": (dict(in_shape=(6, 4, 1), layers=[_c(4, (2, 2), p=(4, 1), ppad=(1, 0, 2, 0)), ("dense", 3, 0)]),
                    "pool (4, 1) over 5 rows, pads 1 and 2: absent elements lead one window and trail the other; 24 rows per utterance, "
                    "so M tiles end inside an utterance"),
    "pool14_oc17": (dict(in_shape=(4, 6, 1), layers=[_c(17, (2, 2), p=(1, 4), ppad=(0, 1, 0, 2)), ("dense", 3, 0)]),
                    "the same along the width, 17 channels: two channel tiles in a padded layer"),
    "neg_no_relu": (dict(in_shape=(5, 5, 1), layers=[_c(4, (3, 3), p=(2, 2), relu=0, cpad=(1, 1, 1, 1), ppad=(1, 1, 0, 0)), ("dense", 3, 0)],
                         bias=-30.0, positive=True, sets=["neg"]),
                    "conv and pool pads together, no ReLU, bias -30, positive weights on all-negative inputs: every real value is below "
                    "-30, an absent element that turned into 0 would win every window it is in"),
    "mid_pads_batch": (dict(in_shape=(24, 20, 2), layers=[_c(4, (3, 3)), _c(8, (3, 3), cpad=(1, 2, 1, 0)),
                                                           _c(6, (3, 3), s=(2, 2), p=(1, 2), cpad=(1, 1, 0, 0), ppad=(0, 0, 0, 1)), ("dense", 5, 0)]),
                       "three convs, pads on the second and third (the padded gather reads both LDS buffers), 4752 floats of activations "
                       "per utterance: a plan batch below 16"),
    "oc65_pad": (dict(in_shape=(4, 4, 1), layers=[_c(65, (3, 3), cpad=(1, 0, 1, 0)), ("dense", 4, 0)]),
                 "65 channels on a padded layer: two channel groups, the second with one tile"),
}
PAD.update({name: (dict(in_shape=(31, 13, 1), zoo=name), "kws_keras.get_model's %s at the shipped 31x13x1 input, through the importer" % name)
            for name in ZOO})

LARGE = {
    "dense_over": (dict(in_shape=(1, 2564, 1), layers=[("dense", 16, 0)]),
                   "SWEEP_REFUSALS' weights_over_lds shape: k_pad 2564 x 16 = 41 024 floats, one N tile; k_pad = 40 KC + 4"),
    "acts_over": (dict(in_shape=(1, 2276, 1), layers=[("dense", 16, 0)]),
                  "SWEEP_REFUSALS' lds_batch1 shape: the record fits the LDS, with one utterance's activations it does not"),
    "dense_wide": (dict(in_shape=(1, 700, 1), layers=[("dense", 72, 1), ("dense", 10, 0)]),
                   "n_pad 80: two channel groups, the last of one tile, and 8 padding channels; then a fitting dense with k_pad 72"),
    "conv_valid_pool2": (dict(in_shape=(6, 3, 48), layers=[_c(96, (3, 3), p=(2, 1)), ("dense", 5, 0)]),
                         "K 432 x 96 = 41 472 floats: the unpadded instantiation with P = 2, 4 rows per utterance"),
    "conv_same_pool4": (dict(in_shape=(5, 4, 64), layers=[_c(64, (4, 3), p=(2, 2), cpad=(1, 1, 2, 1), ppad=(0, 0, 1, 0)), ("dense", 6, 0)]),
                        "K 768 x 64 = 12 KC: the padded instantiation with P = 4, Keras's 'same' pads of a 4x3 kernel and of a (2, 2) pool "
                        "over 5 rows: taps outside the image and absent rows, 24 rows per utterance"),
    "mixed": (dict(in_shape=(12, 10, 1), layers=[_c(24, (3, 3)), ("dense", 32, 1), ("dense", 6, 0)]),
              "a fitting conv (k_pad 12 < KC, 80 rows per utterance), a dense 1920 x 32 over the LDS, a fitting dense"),
    "conv_model": (dict(in_shape=(8, 6, 1), arch="conv_model", classes=4),
                   "train.get_model's conv_model at 8x6x1, 4 classes: 'same' convs and a 'same' pool, the second conv 2560 x 64"),
    "low_latency_conv": (dict(in_shape=(20, 9, 1), arch="low_latency_conv", classes=4, plain=E_SIZE),
                         "train.get_model's low_latency_conv at 20x9x1, 4 classes: 186 channels (three groups, the last of four tiles with 6 "
                         "padding channels), a dense 11160 x 128 whose in_c the plain loader turns away as a field out of range"),
}

# what the rows must cover between them; tests/test_fnet_large_cpu.py fails when the last row that covers one of them goes
REQUIRED = [("over", "weights"), ("over", "acts"), ("k", "below_KC"), ("k", "multiple_of_KC"), ("k", "multiple_of_KC_plus_4"), ("k", "partial_last_chunk"),
            ("NG", 1), ("NG", 2), ("nt_last", 1), ("nt_last", 4), ("padding_channels",), ("PAD", False, "P", 1), ("PAD", False, "P", 2),
            ("PAD", True, "P", 1), ("PAD", True, "P", 4), ("absent_rows", 4), ("outside_taps",), ("record", "over", "dense"), ("record", "over", "conv"),
            ("record", "fits", "conv"), ("record", "fits", "dense"), ("last_M_tile_partial",), ("tile_straddles_utterances",), ("M_blocks", 1),
            ("M_blocks", 2), ("idle_waves",), ("chunks", 3, "last", 5)]

# per table: the offset of the weights' seed and their distribution, what the "neg" input set subtracts from -|30 g|, and whether the
# records carry cpad / ppad (SWEEP's never heard of pads: test_fgrad_pad_cpu compares them with explicit zeros)
TABLES = {"sweep": dict(rows=SWEEP, seed=1000, dist="normal", neg=0.0, pad_keys=False),
          "pad": dict(rows=PAD, seed=2000, dist="normal", neg=1.0, pad_keys=True),
          "large": dict(rows=LARGE, seed=3000, dist="uniform", neg=1.0, pad_keys=True)}
ROWS = {name: row + (t,) for t in TABLES.values() for name, row in t["rows"].items()}
assert len(ROWS) == len(SWEEP) + len(PAD) + len(LARGE)

SETS = ("n1", "n60", "i16", "zero", "neg")
NS = (1, 5, 19)                          # LARGE's utterances: one; two whose M tiles straddle utterances and end in a partial tile
N_CHUNKED, CHUNK = 19, 7                 # with the workspace capped at CHUNK utterances: chunks of 7, 7 and 5


def _seed(name):
    return sum(map(ord, name))


def inputs(name, n, in_n=None):
    """n inputs [n][in_n] float32 of row `name` (in_n: the row's own unless given): utterance i from set sets[i % len(sets)], fixed
    seeds, the same whatever n is. Every utterance draws its normal vector and then its int16 vector, whichever set it takes."""
    spec, _, t = ROWS[name]
    sets = spec.get("sets", SETS)
    in_n = int(np.prod(spec["in_shape"])) if in_n is None else in_n
    rng = np.random.default_rng(_seed(name))
    x = np.empty((n, in_n), np.float32)
    for i in range(n):
        g = rng.normal(0, 1, in_n)
        x[i] = dict(n1=g, n60=60 * g, i16=rng.integers(-32768, 32768, in_n), zero=0 * g, neg=-np.abs(30 * g) - t["neg"], tiny=g * 2.0 ** -70,
                    sub=g * 2.0 ** -130)[sets[i % len(sets)]]
    return x


def _records(in_shape, layers, pad_keys=True):
    h, w, c = in_shape
    out = []
    for L in layers:
        if L[0] == "dense":
            L = ("conv", L[1], (h, w), (1, 1), (1, 1), L[2])
        _, oc, k, s, p, relu, cp, pp = L if len(L) == 8 else L + (Z4, Z4)
        out.append(dict(type=cube_import.T_CONV, inp=(h, w, c), out=out_hw((h, w), k, s, p, cp, pp) + (oc,), k=k, s=s, p=p, relu=relu))
        if pad_keys:
            out[-1].update(cpad=cp, ppad=pp)
        h, w, c = out[-1]["out"]
    return out


def network(in_shape, layers, pad_keys=True):
    """The model dict of `layers` on in_shape, a softmax behind them, without weights."""
    recs = _records(in_shape, layers, pad_keys)
    return dict(in_shape=in_shape, layers=recs + [dict(type=cube_import.T_SOFTMAX, inp=recs[-1]["out"], out=recs[-1]["out"])])


def seeded(m, seed, dist="normal", positive=False, wscale=None, bias="rand"):
    """Model dict m with float32 weights drawn from default_rng(seed), record by record the weights and then the bias: N(0, 1) or
    U(-1, 1) over sqrt(K) (times wscale[i], |.| if positive), biases N(0, 0.1) or U(-1, 1); bias "zero" or a constant is not drawn."""
    rng = np.random.default_rng(seed)
    for i, L in enumerate(conv_records(m)):
        shape = (L["out"][2],) + tuple(L["k"]) + (L["inp"][2],)
        w = (rng.normal(0, 1, shape) if dist == "normal" else rng.uniform(-1, 1, shape)) / np.sqrt(np.prod(shape[1:]))
        L["w"] = ((np.abs(w) if positive else w) * (wscale[i] if wscale else 1.0)).astype(np.float32)
        if bias == "rand":
            L["b"] = (rng.normal(0, 0.1, shape[0]) if dist == "normal" else rng.uniform(-1, 1, shape[0])).astype(np.float32)
        else:
            L["b"] = np.full(shape[0], 0.0 if bias == "zero" else bias, np.float32)
    return m


_MODELS, _BLOBS = {}, {}


def model(name):
    """Row `name` -> its cube_import model dict (float32 weights), built once; the dicts are the caller's own, the arrays shared."""
    if name not in _MODELS:
        spec, _, t = ROWS[name]
        if "synth" in spec or "zoo" in spec:
            _MODELS[name] = cube_import.read_blob(blob(name))
        else:
            m = train.get_model(spec["arch"], spec["in_shape"], spec["classes"]) if "arch" in spec else network(spec["in_shape"], spec["layers"], t["pad_keys"])
            _MODELS[name] = seeded(m, t["seed"] + _seed(name), t["dist"], **{k: spec[k] for k in ("positive", "wscale", "bias") if k in spec})
    m = _MODELS[name]
    return dict(m, layers=[dict(L) for L in m["layers"]])


def sources(name):
    """The X-CUBE-AI sources (net_c, data_c) of a synth or zoo row."""
    spec = ROWS[name][0]
    return cube_synth.cube_sources(spec["in_shape"], spec["synth"] if "synth" in spec else zoo_specs(spec["zoo"], spec["in_shape"]), seed=_seed(name))


def blob(name):
    if name not in _BLOBS:
        spec = ROWS[name][0]
        _BLOBS[name] = cube_synth.import_sources(*sources(name)) if "synth" in spec or "zoo" in spec else cube_import.build_blob(model(name))
    return _BLOBS[name]


_PLANS = {}


def plan_of(name, large=False):
    """fnet_plan.plan of row `name`'s blob, computed once."""
    if (name, large) not in _PLANS:
        _PLANS[name, large] = fnet_plan.plan(blob(name), large=large)
    return _PLANS[name, large]


def unpadded(m):
    """The same layers with every pad removed (shapes shrink; a dense layer's weights are cut to its new input). None when a kernel
    no longer fits."""
    h, w, c = was = m["in_shape"]
    out = []
    for L in m["layers"]:
        L, before = dict(L), was
        was = L["out"]
        if L["type"] == cube_import.T_CONV:
            dense = tuple(L["k"]) == tuple(L["inp"][:2]) and not any(L.get("cpad", Z4))
            if dense:
                flat = tuple(L["inp"][:2]) == (1, 1) and tuple(before[:2]) != (1, 1)      # the importer's dense: 1 x 1 over a flat view
                L["w"] = np.ascontiguousarray(L["w"].reshape((-1,) + tuple(before))[:, :h, :w, :c])
                if flat:
                    L["w"] = L["w"].reshape(-1, 1, 1, h * w * c)
                    h, w, c = 1, 1, h * w * c
                L["k"] = (h, w)
            L["inp"] = (h, w, c)
            L["cpad"] = L["ppad"] = Z4
            oh, ow = out_hw((h, w), L["k"], L["s"], L["p"], Z4, Z4)
            if oh < 1 or ow < 1:
                return None
            L["out"] = (oh, ow, L["out"][2])
        else:
            L["inp"] = L["out"] = (h, w, c)
        h, w, c = L["out"]
        out.append(L)
    return dict(in_shape=m["in_shape"], layers=out)


# ---- what a row takes --------------------------------------------------------------------------------------------------------------
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


def pad_facts(name):
    """What row `name` takes that another row may not: its padded layers' pads, strides and pools, kernels wider than their input,
    padded layers behind the first, channel groups in a padded layer, a plan batch below 16."""
    p = plan_of(name)
    f = set()
    for i, L in enumerate(p["layers"]):
        if not L["pad"]:
            continue
        if any(L["cpad"]):
            f.add(("cpad", L["cpad"], L["s"], any(L["ppad"])))
        if any(L["ppad"]):
            f.add(("ppad", L["p"], L["ppad"]))
        f |= {("k>in", a) for a in (0, 1) if L["k"][a] > L["inp"][a]}
        f |= {("pad_layer", i)} if i else set()
        f |= {("pad_NG", L["NG"])} if L["NG"] > 1 else set()
        f |= {("pad_nt", L["nt_last"])} if L["nt_last"] > 1 else set()
        f |= {("pad_no_relu",)} if not L["relu"] else set()
        if L["P"] == 4 and L["live"] < L["rows"] and any(nu * L["rows"] % 16 for nu in range(1, p["batch"] + 1)):
            f.add(("m_tail_P4_absent",))
    if 1 < p["batch"] < 16:
        f.add(("batch_mid",))
    return frozenset(f)


def large_facts(name):
    """What row `name` makes the layer kernel do at the utterance counts NS, from the tiling: K cases of the chunk loop, channel groups
    and tiles, instantiations, pool windows, absent rows and outside taps, and how M tiles and M blocks fall on the utterances."""
    p = plan_of(name, large=True)
    f = {("over", p["lifted"])}
    for L in p["layers"]:
        k = L["k_pad"]
        f.add(("k", "below_KC" if k < KC else "multiple_of_KC" if k % KC == 0 else "multiple_of_KC_plus_4" if k % KC == 4 else "partial_last_chunk"))
        f.add(("NG", min(L["NG"], 2)))
        f.add(("nt_last", L["nt_last"]))
        f |= {("padding_channels",)} if L["out_c"] < L["n_pad"] else set()
        f.add(("PAD", L["pad"], "P", L["P"]))
        f |= {("absent_rows", L["P"])} if L["live"] < L["rows"] else set()
        f |= {("outside_taps",)} if any(L["cpad"]) else set()
        over = L["k_pad"] * L["n_pad"] > LDS_BYTES // 4
        f.add(("record", "over" if over else "fits", "dense" if L["rows"] == 1 else "conv"))
        for n in NS:
            M = n * L["rows"]
            f |= {("last_M_tile_partial",)} if M % WAVE_ROWS else set()
            f |= {("tile_straddles_utterances",)} if n > 1 and L["rows"] % WAVE_ROWS and L["rows"] > 1 else set()
            f |= {("M_blocks", min(-(-M // MB), 2))}
            f |= {("idle_waves",)} if -(-(M % MB) // WAVE_ROWS) not in (0, MB // WAVE_ROWS) else set()
    f.add(("chunks", -(-N_CHUNKED // fnet_plan.chunk_of(p, fnet_plan.cap_for(p, CHUNK))), "last", N_CHUNKED % CHUNK))
    return frozenset(f)


# ---- refusals: name -> (blob builder, the loader's code, note): networks the importer never writes ------------------------------------
def _pack(ver, in_shape, recs, n_out, payload=b""):
    head = cube_import.HDR.pack(cube_import.MAGIC, ver, len(recs), *in_shape, n_out) + b"\0\0\0\0"
    return head + b"".join(np.asarray(r, "<i4").tobytes() for r in recs) + payload


def _conv_rec(inp, out, k, s, p, relu, k_pad=None, n_pad=None, ver=1, cpad=Z4, ppad=Z4):
    K = k[0] * k[1] * inp[2]
    rec = [cube_import.T_CONV, *inp, *out, *k, *s, relu, *p, k_pad or (K + 3) // 4 * 4, n_pad or (out[2] + 15) // 16 * 16]
    return rec + (list(cpad) + list(ppad) if ver == 2 else [])


def _sm_rec(shape, ver=1):
    return [cube_import.T_SOFTMAX, *shape, *shape] + [0] * (9 if ver == 1 else 17)


def _refuse_pool31():
    return _pack(1, (9, 4, 1), [_conv_rec((9, 4, 1), (2, 4, 4), (3, 1), (1, 1), (3, 1), 1), _sm_rec((2, 4, 4))], 32)


def _refuse_17_layers():
    recs = [_conv_rec((4, 4, 2), (4, 4, 2), (1, 1), (1, 1), (1, 1), 1) for _ in range(17)]
    return _pack(1, (4, 4, 2), recs + [_sm_rec((4, 4, 2))], 32)


def _refuse_weights_lds():
    return _pack(1, (1, 2564, 1), [_conv_rec((1, 2564, 1), (1, 1, 16), (1, 2564), (1, 1), (1, 1), 0), _sm_rec((1, 1, 16))], 16)


def _refuse_lds_batch1():
    h, w = 1, 2276
    m = network((h, w, 1), [("dense", 16, 0)])
    m["layers"][0].update(w=np.zeros((16, h, w, 1), np.float32), b=np.zeros(16, np.float32))
    return cube_import.build_blob(m)


def _refuse_k_pad():
    return _pack(1, (6, 4, 1), [_conv_rec((6, 4, 1), (1, 1, 3), (6, 4), (1, 1), (1, 1), 0, k_pad=28), _sm_rec((1, 1, 3))], 3)


def _refuse_n_pad():
    return _pack(1, (6, 4, 1), [_conv_rec((6, 4, 1), (1, 1, 3), (6, 4), (1, 1), (1, 1), 0, n_pad=32), _sm_rec((1, 1, 3))], 3)


SWEEP_REFUSALS = {
    "pool31": (_refuse_pool31, E_NO_IMPL, "a pool window of 3 elements"),
    "layers17": (_refuse_17_layers, E_NO_IMPL, "17 conv records (18 with the softmax): the header's layer count refuses them; parse()'s in-loop "
                                                  "16-layer check is unreachable, the last record being the softmax"),
    "weights_over_lds": (_refuse_weights_lds, E_NO_IMPL, "k_pad x n_pad = 2564 x 16 = 41 024 floats > 40 960"),
    "lds_batch1": (_refuse_lds_batch1, E_NO_IMPL, "2276 x 16 weights fit, with one utterance's activations they do not"),
    "k_pad": (_refuse_k_pad, E_SIZE, "k_pad 28 for K = 24"),
    "n_pad": (_refuse_n_pad, E_SIZE, "n_pad 32 for 3 channels"),
}


def _payload(recs):
    return b"\0" * (4 * sum(r[14] * r[15] + r[15] for r in recs if r[0] == cube_import.T_CONV))


def _v2(in_shape, conv, n_out=None):
    recs = [conv, _sm_rec(tuple(conv[4:7]), ver=2)]
    return _pack(2, in_shape, recs, n_out or conv[4] * conv[5] * conv[6], _payload(recs))


PAD_REFUSALS = {
    # a pad as large as the window on its axis: a window wholly in padding
    "conv_pad_is_kernel": (lambda: _v2((5, 4, 1), _conv_rec((5, 4, 1), (6, 4, 3), (3, 3), (1, 1), (1, 1), 1, cpad=(3, 1, 0, 1), ver=2)), E_NO_IMPL,
                           "top pad 3 under a 3x3 kernel (the shape follows from the formula: only the pad is wrong)"),
    "pool_pad_is_pool": (lambda: _v2((6, 4, 1), _conv_rec((6, 4, 1), (3, 3, 4), (2, 2), (1, 1), (2, 1), 1, ppad=(2, 0, 0, 0), ver=2)), E_NO_IMPL,
                         "top pool pad 2 under a (2, 1) pool"),
    "out_shape_off_by_one": (lambda: _v2((5, 4, 1), _conv_rec((5, 4, 1), (5, 5, 3), (3, 3), (1, 1), (1, 1), 1, cpad=(1, 1, 1, 1), ver=2)), E_SIZE,
                             "pads (1, 1, 1, 1) under 3x3 give 5x4, the record declares 5x5"),
    "negative_pad": (lambda: _v2((5, 4, 1), _conv_rec((5, 4, 1), (4, 4, 3), (4, 3), (1, 1), (1, 1), 1, cpad=(-1, 1, 3, 1), ver=2)), E_SIZE,
                     "top pad -1 under a 4x3 kernel (with bottom 3 the sums still give the declared shape)"),
    "version3": (lambda: blob("sym3x3")[:4] + b"\x03" + blob("sym3x3")[5:], E_NO_IMPL, "a version the loader does not know"),
}

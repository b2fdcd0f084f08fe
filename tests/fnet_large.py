"""Float32 networks whose layers exceed the LDS (edison_fnet_load_ex, the layer road): the rows, their inputs, and a
restatement of the road's tiling (csrc/fnet.h's ED_FNET_LAYER_* and ws_chunk() in csrc/edison_fnet.hip). Test infrastructure, not a test:
tests/test_fnet_large_cpu.py holds the rows to the coverage they claim and the host model to its float64 restatement;
tests/test_gpu_fnet_large.py holds the layer kernel to the host model (tests/fnet_pad.py's run: the k-ordered fmaf chain) bit for bit.

A row is (spec, note). spec: in_shape and layers in fnet_pad's form (("conv", out_c, (kh, kw), (sh, sw), (ph, pw), relu, cpad, ppad) or
("dense", n, relu)), or arch: one of train.get_model's architectures at in_shape x classes; plain: the code the plain loader answers
(E_NO_IMPL unless stated). Every record's weights and bias are seeded uniform values in [-1, 1], the weights over sqrt(K) so that
activations keep their scale through a K of thousands. The models are cube_import.build_blob model dicts."""
import numpy as np

from edison_amd import cube_import, train

import fnet_exact as fe
import fnet_pad as fp
import fnet_sweep as fs

# csrc/fnet.h
MB, NB, KC = 128, 64, 64                 # ED_FNET_LAYER_MB / _NB / _KC: a workgroup's rows and channels, the K chunk
WAVE_ROWS = 16                           # one M tile per wave
LAYER_LDS_BYTES = 4 * (MB * (KC + 2) + KC * (NB + 16) + 3 * MB)     # ED_FNET_LAYER_LDS_BYTES
WS_DEFAULT = 256 << 20                   # ED_FNET_WORKSPACE_DEFAULT
INT32_MAX = 2 ** 31 - 1

NS = (1, 5, 19)                          # utterances: one; two whose M tiles straddle utterances and end in a partial tile
N_CHUNKED, CHUNK = 19, 7                 # with the workspace capped at CHUNK utterances: chunks of 7, 7 and 5

_c, Z4 = fp._c, fp.Z4

ROWS = {
    "dense_over": (dict(in_shape=(1, 2564, 1), layers=[("dense", 16, 0)]),
                   "fnet_sweep's weights_over_lds shape: k_pad 2564 x 16 = 41 024 floats, one N tile; k_pad = 40 KC + 4"),
    "acts_over": (dict(in_shape=(1, 2276, 1), layers=[("dense", 16, 0)]),
                  "fnet_sweep's lds_batch1 shape: the record fits the LDS, with one utterance's activations it does not"),
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
    "low_latency_conv": (dict(in_shape=(20, 9, 1), arch="low_latency_conv", classes=4, plain=fe.E_SIZE),
                         "train.get_model's low_latency_conv at 20x9x1, 4 classes: 186 channels (three groups, the last of four tiles with 6 "
                         "padding channels), a dense 11160 x 128 whose in_c the plain loader turns away as a field out of range"),
}


def _seed(name):
    return sum(map(ord, name))


_MODELS, _BLOBS = {}, {}


def model(name):
    """Row `name` -> the cube_import model dict with its seeded weights."""
    if name in _MODELS:
        return _MODELS[name]
    spec = ROWS[name][0]
    if "arch" in spec:
        m = train.get_model(spec["arch"], spec["in_shape"], spec["classes"])
    else:
        recs = fp._records(spec["in_shape"], spec["layers"])
        last = recs[-1]["out"]
        m = dict(in_shape=spec["in_shape"], layers=recs + [dict(type=cube_import.T_SOFTMAX, inp=last, out=last)])
    rng = np.random.default_rng(3000 + _seed(name))
    for L in fe.conv_records(m):
        oc, (kh, kw), ic = L["out"][2], L["k"], L["inp"][2]
        L["w"] = (rng.uniform(-1, 1, (oc, kh, kw, ic)) / np.sqrt(kh * kw * ic)).astype(np.float32)
        L["b"] = rng.uniform(-1, 1, oc).astype(np.float32)
    _MODELS[name] = m
    return m


def blob(name):
    if name not in _BLOBS:
        _BLOBS[name] = cube_import.build_blob(model(name))
    return _BLOBS[name]


def in_n(name):
    return int(np.prod(ROWS[name][0]["in_shape"]))


def inputs(name, n):
    """n inputs [n][in_n] float32 of row `name`, as fnet_pad.inputs draws them from fnet_sweep's input sets: utterance i is the same
    whatever n is."""
    rng = np.random.default_rng(_seed(name))
    x = np.empty((n, in_n(name)), np.float32)
    for i in range(n):
        g = rng.normal(0, 1, x.shape[1])
        x[i] = dict(n1=g, n60=60 * g, i16=rng.integers(-32768, 32768, x.shape[1]), zero=0 * g, neg=-np.abs(30 * g) - 1.0)[fs.SETS[i % len(fs.SETS)]]
    return x


# ---- the road's plan and tiling, restated ---------------------------------------------------------------------------------------------
def records(m):
    """What parse() keeps of each conv record of model dict m, and the network's buf_n: (layers, buf_n)."""
    layers, buf = [], [int(np.prod(m["in_shape"])), 0]
    for i, L in enumerate(fe.conv_records(m)):
        (ih, iw, ic), (kh, kw), (ph, pw), (cp, pp) = L["inp"], L["k"], L["p"], fp.pads(L)
        oh, ow, oc = L["out"]
        ch, cw = fp.conv_map(L)
        K, P = kh * kw * ic, ph * pw
        live = sum(pp[0] <= y < pp[0] + ch for y in range(oh * ph)) * sum(pp[1] <= x < pp[1] + cw for x in range(ow * pw))
        k_pad, n_pad = (K + 3) // 4 * 4, (oc + 15) // 16 * 16
        layers.append(dict(K=K, k_pad=k_pad, n_pad=n_pad, out_c=oc, P=P, rows=oh * ow * P, live=live, pad=any(cp) or any(pp), cpad=cp, ppad=pp,
                           out_n=oh * ow * oc, NG=-(-n_pad // NB), nt_last=n_pad // 16 - 4 * (-(-n_pad // NB) - 1), src=i & 1, dst=(i & 1) ^ 1))
        buf[(i & 1) ^ 1] = max(buf[(i & 1) ^ 1], oh * ow * oc)
    return layers, [(b + 3) & ~3 for b in buf]


def chunk_of(m, cap=WS_DEFAULT):
    """ws_chunk(): utterances per chunk under a workspace cap of `cap` bytes; 0 when one utterance does not fit."""
    layers, buf_n = records(m)
    chunk = min([cap // (4 * (buf_n[0] + buf_n[1])), INT32_MAX // max(buf_n)] + [INT32_MAX // 16 // L["rows"] for L in layers])
    return chunk - chunk % MB if chunk > MB else chunk


def cap_for(m, chunk):
    """A workspace cap that holds `chunk` utterances of model m and not one more."""
    _, buf_n = records(m)
    return 4 * (buf_n[0] + buf_n[1]) * chunk + 4


def launches(m, n, cap=WS_DEFAULT):
    """(n_layers + 1) * chunks: the kernel launches of one call on n utterances."""
    return (len(records(m)[0]) + 1) * -(-n // chunk_of(m, cap))


def over_lds(m):
    """Which of the plain loader's two LDS refusals model m meets: "weights", "acts", or None for a network that fits."""
    layers, buf_n = records(m)
    w_lds = max(L["k_pad"] * L["n_pad"] for L in layers)
    k_lds = max((2 if L["pad"] else 1) * L["k_pad"] for L in layers)
    if w_lds > fe.LDS_BYTES // 4:
        return "weights"
    return "acts" if (fe.LDS_BYTES - 4 * (w_lds + k_lds)) // (4 * (buf_n[0] + buf_n[1])) < 1 else None


def facts(name):
    """What row `name` makes the layer kernel do at the utterance counts NS, from the tiling: K cases of the chunk loop, channel groups
    and tiles, instantiations, pool windows, absent rows and outside taps, and how M tiles and M blocks fall on the utterances."""
    m = model(name)
    layers, _ = records(m)
    f = {("over", over_lds(m))}
    for L in layers:
        k = L["k_pad"]
        f.add(("k", "below_KC" if k < KC else "multiple_of_KC" if k % KC == 0 else "multiple_of_KC_plus_4" if k % KC == 4 else "partial_last_chunk"))
        f.add(("NG", min(L["NG"], 2)))
        f.add(("nt_last", L["nt_last"]))
        f |= {("padding_channels",)} if L["out_c"] < L["n_pad"] else set()
        f.add(("PAD", L["pad"], "P", L["P"]))
        f |= {("absent_rows", L["P"])} if L["live"] < L["rows"] else set()
        f |= {("outside_taps",)} if any(L["cpad"]) else set()
        over = L["k_pad"] * L["n_pad"] > fe.LDS_BYTES // 4
        f.add(("record", "over" if over else "fits", "dense" if L["rows"] == 1 else "conv"))
        for n in NS:
            M = n * L["rows"]
            f |= {("last_M_tile_partial",)} if M % WAVE_ROWS else set()
            f |= {("tile_straddles_utterances",)} if n > 1 and L["rows"] % WAVE_ROWS and L["rows"] > 1 else set()
            f |= {("M_blocks", min(-(-M // MB), 2))}
            f |= {("idle_waves",)} if -(-(M % MB) // WAVE_ROWS) not in (0, MB // WAVE_ROWS) else set()
    f.add(("chunks", -(-N_CHUNKED // chunk_of(m, cap_for(m, CHUNK))), "last", N_CHUNKED % CHUNK))
    return frozenset(f)


# what the rows must cover between them; tests/test_fnet_large_cpu.py fails when the last row that covers one of them goes
REQUIRED = [("over", "weights"), ("over", "acts"), ("k", "below_KC"), ("k", "multiple_of_KC"), ("k", "multiple_of_KC_plus_4"), ("k", "partial_last_chunk"),
            ("NG", 1), ("NG", 2), ("nt_last", 1), ("nt_last", 4), ("padding_channels",), ("PAD", False, "P", 1), ("PAD", False, "P", 2),
            ("PAD", True, "P", 1), ("PAD", True, "P", 4), ("absent_rows", 4), ("outside_taps",), ("record", "over", "dense"), ("record", "over", "conv"),
            ("record", "fits", "conv"), ("record", "fits", "dense"), ("last_M_tile_partial",), ("tile_straddles_utterances",), ("M_blocks", 1),
            ("M_blocks", 2), ("idle_waves",), ("chunks", 3, "last", 5)]

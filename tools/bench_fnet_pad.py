"""What the padded gather of the float32 network kernel costs: utterances/s and MAC/s of
edison_fnet_batch_dev on

  padded    kws_keras.get_model's medium_embedding_conv at the 31x13x1 input (two 'same' convolutions and a 'same' pool: the kernel's
            PAD = true instantiation on both conv records), seeded random weights
  unpadded  the same layers with every pad removed (PAD = false throughout). Without its pads this network's second kernel (4x4) no
            longer fits the map the first conv and the pool leave (6x1), so the input grows instead, to the smallest (50x34x1) at which
            the last conv keeps its padded output shape and the dense layer its weights. The shapes differ either way, so compare
            MAC/s, not utterances/s.

MACs count real multiply-adds only: a tap in the padding is not one, although the kernel multiplies a zero there.

    python tools/bench_fnet_pad.py [--utts 262144] [--steps 10] [--warmup 3]

One JSON line per figure, timed with device events as tools/bench_fnet.py. Every figure is a single run of one process.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_fnet import timed  # noqa: E402


def macs_per_utt(model):
    """Real multiply-adds of one utterance: per conv output, its taps inside the image x in_c x out_c."""
    import fnet_host
    total = 0
    for L in fnet_host.conv_records(model):
        (ih, iw, ic), (kh, kw), (sh, sw), (c, _) = L["inp"], L["k"], L["s"], fnet_host.pads(L)
        ch, cw = fnet_host.conv_map(L)
        ty = sum(sum(0 <= y * sh - c[0] + ky < ih for ky in range(kh)) for y in range(ch))
        tx = sum(sum(0 <= x * sw - c[1] + kx < iw for kx in range(kw)) for x in range(cw))
        total += ty * tx * ic * L["out"][2]
    return total


def unpadded_grown(m):
    """m without pads, its input grown to the smallest at which the last conv before the dense layers keeps its output shape."""
    import fnet_rows
    from edison_amd import cube_import
    recs = [L for L in m["layers"] if L["type"] == cube_import.T_CONV]
    convs = [L for L in recs if tuple(L["k"]) != tuple(L["inp"][:2]) or any(L["cpad"])]
    h, w = convs[-1]["out"][:2]
    for L in reversed(convs):
        h, w = (h * L["p"][0] - 1) * L["s"][0] + L["k"][0], (w * L["p"][1] - 1) * L["s"][1] + L["k"][1]
    out = fnet_rows.unpadded(dict(m, in_shape=(h, w, m["in_shape"][2])))
    assert out is not None and tuple(out["layers"][len(convs) - 1]["out"]) == tuple(convs[-1]["out"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import fnet_rows
    from edison_amd import cube_import
    from edison_amd.context import Context
    dev = torch.device("cuda", 0)
    padded = fnet_rows.model("medium_embedding_conv")
    nets = [("padded", padded), ("unpadded", fnet_rows.unpadded(padded) or unpadded_grown(padded))]
    c = Context(0, model_path=None)
    board = c.device_info()["name"]
    n = args.utts
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    x = torch.randn((n, max(int(np.prod(m["in_shape"])) for _, m in nets)), generator=gen, device=dev) * 200
    lg = torch.empty((n, 10), dtype=torch.float32, device=dev)
    pr = torch.empty((n, 10), dtype=torch.float32, device=dev)
    am = torch.empty(n, dtype=torch.int32, device=dev)
    for what, m in nets:
        c.fnet_load(cube_import.build_blob(m))
        info = c.fnet_info()
        c.use_torch_stream()
        xin = x[:, :info["in_h"] * info["in_w"] * info["in_c"]].contiguous()
        sec = timed(lambda: c.fnet_t(xin, n, lg, pr, am), args.steps, args.warmup)
        c.use_own_stream()
        macs = macs_per_utt(m)
        shapes = [tuple(L["out"]) for L in m["layers"] if L["type"] == cube_import.T_CONV]
        print(json.dumps(dict(board=board, what="throughput", route="fnet", net="medium_embedding_conv " + what, in_shape=tuple(m["in_shape"]),
                              layer_outputs=shapes,
                              utts=n, batch_per_workgroup=info["batch"], lds_bytes=info["lds_bytes"], seconds=round(sec, 6),
                              utts_per_s=round(n / sec, 1), macs_per_utt=macs, gmacs_per_s=round(macs * n / sec / 1e9, 1))), flush=True)
    c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

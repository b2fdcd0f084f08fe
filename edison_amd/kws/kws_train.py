"""``kws train <net.ednf> <x.npy> <y.npy> <out.ednf>`` -- train a float32 X-CUBE-AI network on the GPU (``Context.trainer``,
edison_amd/train.py): what the reference does with ``kws_keras.train`` (kws_keras.py:400-416), for every network
the float path runs, 'same' convs and pools included. The network file gives the architecture and the starting weights: an imported network to fine-tune, or
``cube_import.build_blob`` of a freshly initialised model dict.

    x.npy           float32 [n, in_h * in_w * in_c] (or [n, in_h, in_w, in_c]): the network inputs, the float flow's features
    y.npy           integer class indices [n]
    --epochs N      (30)      --batch N   (100)      --lr r   (0.0005, Adam)      --seed s   (0: the shuffle)
    --val x.npy y.npy         a validation set: its loss drives ReduceLROnPlateau(0.5, patience 1) and EarlyStopping(patience 10)
    --dropout r0,r1,..        a Dropout rate behind each conv / dense record's output (the last is 0), e.g. 0,0,0.2,0.3,0
    --dropout-before-pool b0,b1,..   1: that record's Dropout stands between ReLU and the pool, 0 (default): behind the pool
    --dropout-arch NAME       the reference's placement for one of its architectures (train.KERAS_DROPOUT), e.g. kws_conv
The masks are seeded by --seed; validation runs without dropout.

Prints the history per epoch and writes the trained network, which ``kws quantize`` takes.
"""
import sys

import numpy as np

USAGE = "usage: kws train <net.ednf> <x.npy> <y.npy> <out.ednf> [--epochs N] [--batch N] [--lr r] [--seed s] [--val <x.npy> <y.npy>] [--dropout r,..] [--dropout-before-pool b,..] [--dropout-arch NAME]"


def run(net, x_path, y_path, out_path, epochs=30, batch=100, lr=None, seed=0, val=None, ctx=None, out=None, dropout=None, before_pool=None,
        dropout_arch=None):
    from .. import train
    from ..context import default_context
    out = out or sys.stdout
    ctx = ctx or default_context()
    x, y = np.load(x_path), np.load(y_path)
    v = (np.load(val[0]), np.load(val[1])) if val else None
    if dropout_arch is not None:
        if dropout is not None or dropout_arch not in train.KERAS_DROPOUT:
            raise ValueError("--dropout-arch is one of %s, and not given beside --dropout" % ", ".join(sorted(train.KERAS_DROPOUT)))
        dropout = train.KERAS_DROPOUT[dropout_arch]
    if dropout is None and before_pool is not None:
        raise ValueError("--dropout-before-pool needs --dropout")
    ctx.fnet_load(net)
    with ctx.trainer(padded=True) as tr:
        if dropout is not None:
            tr.set_dropout(dropout, before_pool, seed=seed)
        hist = tr.fit(x, y, epochs, batch_size=batch, val=v, seed=seed, lr=train.LEARNING_RATE if lr is None else lr)
        blob = tr.export()
    for i, (l, a) in enumerate(zip(hist["loss"], hist["acc"])):
        line = "epoch %3d  lr %.3g  loss %.6f  acc %.4f" % (i + 1, hist["lr"][i], l, a)
        if v is not None:
            line += "  val_loss %.6f  val_acc %.4f" % (hist["val_loss"][i], hist["val_acc"][i])
        out.write(line + "\n")
    if hist["stopped_early"]:
        out.write("stopped early: the validation loss has not improved for 10 epochs\n")
    with open(out_path, "wb") as f:
        f.write(blob)
    out.write("wrote %s: %d bytes after %d steps\n" % (out_path, len(blob), hist["steps"]))
    return blob, hist


def main(argv):
    opts = {"--epochs": "30", "--batch": "100", "--lr": None, "--seed": "0", "--dropout": None, "--dropout-before-pool": None, "--dropout-arch": None}
    rest, val = [], None
    i = 1
    while i < len(argv):
        if argv[i] == "--val":
            if i + 2 >= len(argv):
                print("--val needs two files")
                return 1
            val = (argv[i + 1], argv[i + 2])
            i += 3
        elif argv[i] in opts:
            if i + 1 >= len(argv):
                print("%s needs a value" % argv[i])
                return 1
            opts[argv[i]] = argv[i + 1]
            i += 2
        else:
            rest.append(argv[i])
            i += 1
    if len(rest) != 4:
        print(USAGE)
        return 1
    try:
        epochs, batch, seed = int(opts["--epochs"]), int(opts["--batch"]), int(opts["--seed"])
        lr = None if opts["--lr"] is None else float(opts["--lr"])
        dropout = None if opts["--dropout"] is None else [float(v) for v in opts["--dropout"].split(",")]
        before = None if opts["--dropout-before-pool"] is None else [int(v) for v in opts["--dropout-before-pool"].split(",")]
    except ValueError:
        print(USAGE)
        return 1
    from .._lib import EdisonError
    try:
        run(rest[0], rest[1], rest[2], rest[3], epochs=epochs, batch=batch, lr=lr, seed=seed, val=val, dropout=dropout, before_pool=before,
            dropout_arch=opts["--dropout-arch"])
    except (EdisonError, ValueError) as e:
        print("kws train: %s" % e)
        return 1
    return 0

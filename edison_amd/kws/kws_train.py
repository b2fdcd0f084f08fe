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
    --batchnorm b0,b1,..      1: that record is conv -> BatchNorm -> ReLU -> pool (the last is 0), e.g. 1,1,1,1,0; no record may have a pad
    --batchnorm-arch NAME     the reference's placement for one of its architectures (train.KERAS_BATCHNORM): kws_conv has BatchNorm
    --bn-momentum m (0.99)    --bn-eps e (0.001)    --bn-unbiased   the moving variance takes var N / (N - 1) (torch's rule)
The masks are seeded by --seed; validation runs without dropout and on BatchNorm's moving statistics. With BatchNorm the written network
has it folded into the convolutions, as X-CUBE-AI and NNoM do: the .ednf stays a plain conv / dense network. The dropout and BatchNorm
options combine: --batchnorm-arch kws_conv --dropout-arch kws_conv is the reference's recipe for its shipped network.

Prints the history per epoch and writes the trained network, which ``kws quantize`` takes.
"""
import sys

import numpy as np

USAGE = "usage: kws train <net.ednf> <x.npy> <y.npy> <out.ednf> [--epochs N] [--batch N] [--lr r] [--seed s] [--val <x.npy> <y.npy>] [--dropout r,..] [--dropout-before-pool b,..] [--dropout-arch NAME] [--batchnorm b,.. | --batchnorm-arch NAME] [--bn-momentum m] [--bn-eps e] [--bn-unbiased]"


def run(net, x_path, y_path, out_path, epochs=30, batch=100, lr=None, seed=0, val=None, ctx=None, out=None, dropout=None, before_pool=None,
        dropout_arch=None, batchnorm=None, batchnorm_arch=None, bn_momentum=None, bn_eps=None, bn_unbiased=False):
    from .. import train
    out = out or sys.stdout
    if batchnorm_arch is not None:
        if batchnorm is not None or batchnorm_arch not in train.KERAS_BATCHNORM:
            raise ValueError("--batchnorm-arch is one of %s, and not given beside --batchnorm" % ", ".join(sorted(train.KERAS_BATCHNORM)))
        batchnorm = train.KERAS_BATCHNORM[batchnorm_arch]
    if batchnorm is None and (bn_momentum is not None or bn_eps is not None or bn_unbiased):
        raise ValueError("--bn-momentum, --bn-eps and --bn-unbiased need --batchnorm or --batchnorm-arch")
    if batchnorm is not None:
        bn_momentum = train.BN_MOMENTUM if bn_momentum is None else bn_momentum
        bn_eps = train.BN_EPS if bn_eps is None else bn_eps
        if not 0.0 <= bn_momentum < 1.0 or not bn_eps > 0.0:
            raise ValueError("--bn-momentum is in [0, 1) and --bn-eps above 0")
        if batchnorm[-1]:
            raise ValueError("--batchnorm: the last record's output is the logits; it takes no BatchNorm")
    from ..context import default_context
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
        if batchnorm is not None and any(batchnorm):
            tr.set_batchnorm(batchnorm, momentum=bn_momentum, eps=bn_eps, max_rows=max(int(batch), 1), unbiased=bn_unbiased)
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
    opts = {"--epochs": "30", "--batch": "100", "--lr": None, "--seed": "0", "--dropout": None, "--dropout-before-pool": None, "--dropout-arch": None,
            "--batchnorm": None, "--batchnorm-arch": None, "--bn-momentum": None, "--bn-eps": None}
    rest, val, unbiased = [], None, False
    i = 1
    while i < len(argv):
        if argv[i] == "--val":
            if i + 2 >= len(argv):
                print("--val needs two files")
                return 1
            val = (argv[i + 1], argv[i + 2])
            i += 3
        elif argv[i] == "--bn-unbiased":
            unbiased = True
            i += 1
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
        batchnorm = None if opts["--batchnorm"] is None else [int(v) for v in opts["--batchnorm"].split(",")]
        momentum = None if opts["--bn-momentum"] is None else float(opts["--bn-momentum"])
        bn_eps = None if opts["--bn-eps"] is None else float(opts["--bn-eps"])
    except ValueError:
        print(USAGE)
        return 1
    from .._lib import EdisonError
    try:
        run(rest[0], rest[1], rest[2], rest[3], epochs=epochs, batch=batch, lr=lr, seed=seed, val=val, dropout=dropout, before_pool=before,
            dropout_arch=opts["--dropout-arch"], batchnorm=batchnorm, batchnorm_arch=opts["--batchnorm-arch"], bn_momentum=momentum, bn_eps=bn_eps,
            bn_unbiased=unbiased)
    except (EdisonError, ValueError) as e:
        print("kws train: %s" % e)
        return 1
    return 0

"""``kws train <net.ednf> <x.npy> <y.npy> <out.ednf>`` -- train a float32 X-CUBE-AI network on the GPU (``Context.trainer``,
edison_amd/train.py; DESIGN.md sections 19 and 19d): what the reference does with ``kws_keras.train`` (kws_keras.py:400-416), for every network
the float path runs, 'same' convs and pools included. The network file gives the architecture and the starting weights: an imported network
to fine-tune. ``kws train --arch NAME <x.npy> <y.npy> <out.ednf>`` trains one of the reference's architectures from scratch instead
(``train.get_model``: kws_keras.py:170-403 with Keras's default initialisation, drawn from --seed).

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
    --arch NAME [--classes N (10)] [--in-shape h,w,c (31,13,1)]   no network file: train.get_model(NAME, ...) with --seed. It builds the
                              convs and dense layers only: --batchnorm-arch / --dropout-arch turn the reference's BatchNorm / Dropout on
    --resident                hold the features on the device and train with Trainer.fit_data: one library call and one
                              synchronisation an epoch (edison_ftrain_epoch) instead of one round trip a batch
    --audio [--geometry k=v,..]   x.npy (and --val's x) is int16 audio [n][samples]: the float flow's features are computed on the
                              device straight into the data set (``kws eval``'s geometry); implies --resident
    --opt adam|sgd|adadelta   the optimiser (adam); --rho r (0.95) is Adadelta's. Adadelta without --lr runs at 1.0: Keras's 'adadelta'
                              as remembered (lr 1.0, rho 0.95, epsilon 1e-7; unpinned), what kws_nnom.train compiles with
The masks are seeded by --seed; validation runs without dropout and on BatchNorm's moving statistics. With BatchNorm the written network
has it folded into the convolutions, as X-CUBE-AI and NNoM do: the .ednf stays a plain conv / dense network. The dropout and BatchNorm
options combine: --batchnorm-arch kws_conv --dropout-arch kws_conv is the reference's recipe for its shipped network.

Prints the history per epoch and writes the trained network, which ``kws quantize`` takes.
"""
import sys

import numpy as np

USAGE = "usage: kws train <net.ednf> | --arch NAME [--classes N] [--in-shape h,w,c]  <x.npy> <y.npy> <out.ednf> [--resident] [--audio [--geometry k=v,...]] [--opt adam|sgd|adadelta] [--rho r] [--epochs N] [--batch N] [--lr r] [--seed s] [--val <x.npy> <y.npy>] [--dropout r,..] [--dropout-before-pool b,..] [--dropout-arch NAME] [--batchnorm b,.. | --batchnorm-arch NAME] [--bn-momentum m] [--bn-eps e] [--bn-unbiased]"


OPTS = ("adam", "sgd", "adadelta")


def check_opts(arch=None, opt="adam", rho=None, geometry=None, audio=False):
    """The refusals of the new options that need nothing but their values (ValueError): main checks them before run, run again."""
    from .. import train
    if arch is not None and arch not in train.ARCHS:
        raise ValueError("--arch is one of %s" % ", ".join(train.ARCHS))
    if opt not in OPTS:
        raise ValueError("--opt is one of %s" % ", ".join(OPTS))
    if rho is not None and opt != "adadelta":
        raise ValueError("--rho needs --opt adadelta")
    if rho is not None and not 0.0 <= rho < 1.0:
        raise ValueError("--rho is in [0, 1)")
    if geometry is not None and not audio:
        raise ValueError("--geometry needs --audio")


def run(net, x_path, y_path, out_path, epochs=30, batch=100, lr=None, seed=0, val=None, ctx=None, out=None, dropout=None, before_pool=None,
        dropout_arch=None, batchnorm=None, batchnorm_arch=None, bn_momentum=None, bn_eps=None, bn_unbiased=False, arch=None, classes=10,
        in_shape=None, resident=False, audio=False, geometry=None, opt="adam", rho=None):
    """net: the .ednf file, or None with arch (train.get_model(arch, in_shape, classes, seed)). Returns (trained blob, history)."""
    from .. import cube_import, train
    out = out or sys.stdout
    check_opts(arch, opt, rho, geometry, audio)
    if (net is None) == (arch is None):
        raise ValueError("kws train takes a network file or --arch, not both")
    if arch is None and (in_shape is not None or classes != 10):
        raise ValueError("--classes and --in-shape need --arch")
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
    ctx.fnet_load(net if arch is None else cube_import.build_blob(train.get_model(arch, (31, 13, 1) if in_shape is None else in_shape, classes, seed)))
    if lr is None:
        lr = train.ADADELTA_LR if opt == "adadelta" else train.LEARNING_RATE
    sets = []
    try:
        if audio or resident:
            g = None
            if audio:
                from .. import config as cfg
                from .kws_eval import parse_geometry
                g = parse_geometry(geometry, net_input_scale=cfg.net_input_scale) if geometry else None
            for a, b in [(x, y)] + ([v] if v is not None else []):
                sets.append(ctx.train_data(audio=a, y=b, geometry=g) if audio else ctx.train_data(a, b))
        with ctx.trainer(padded=True) as tr:
            if opt == "adadelta":
                tr.set_opt("adadelta", rho=train.ADADELTA_RHO if rho is None else rho, eps=train.ADADELTA_EPS)
            elif opt == "sgd":
                tr.set_opt("sgd")
            if dropout is not None:
                tr.set_dropout(dropout, before_pool, seed=seed)
            if batchnorm is not None and any(batchnorm):
                tr.set_batchnorm(batchnorm, momentum=bn_momentum, eps=bn_eps, max_rows=max(int(batch), 1), unbiased=bn_unbiased)
            if sets:
                hist = tr.fit_data(sets[0], epochs, batch_size=batch, val=sets[1] if v is not None else None, seed=seed, lr=lr)
            else:
                hist = tr.fit(x, y, epochs, batch_size=batch, val=v, seed=seed, lr=lr)
            blob = tr.export()
    finally:
        for d in sets:
            d.close()
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
            "--batchnorm": None, "--batchnorm-arch": None, "--bn-momentum": None, "--bn-eps": None, "--arch": None, "--classes": "10", "--in-shape": None,
            "--geometry": None, "--opt": "adam", "--rho": None}
    flags = {"--bn-unbiased": False, "--resident": False, "--audio": False}
    rest, val = [], None
    i = 1
    while i < len(argv):
        if argv[i] == "--val":
            if i + 2 >= len(argv):
                print("--val needs two files")
                return 1
            val = (argv[i + 1], argv[i + 2])
            i += 3
        elif argv[i] in flags:
            flags[argv[i]] = True
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
    if len(rest) != (4 if opts["--arch"] is None else 3):
        print(USAGE)
        return 1
    if opts["--arch"] is not None:
        rest = [None] + rest
    try:
        epochs, batch, seed = int(opts["--epochs"]), int(opts["--batch"]), int(opts["--seed"])
        lr = None if opts["--lr"] is None else float(opts["--lr"])
        dropout = None if opts["--dropout"] is None else [float(v) for v in opts["--dropout"].split(",")]
        before = None if opts["--dropout-before-pool"] is None else [int(v) for v in opts["--dropout-before-pool"].split(",")]
        batchnorm = None if opts["--batchnorm"] is None else [int(v) for v in opts["--batchnorm"].split(",")]
        momentum = None if opts["--bn-momentum"] is None else float(opts["--bn-momentum"])
        bn_eps = None if opts["--bn-eps"] is None else float(opts["--bn-eps"])
        classes = int(opts["--classes"])
        in_shape = None if opts["--in-shape"] is None else tuple(int(v) for v in opts["--in-shape"].split(","))
        rho = None if opts["--rho"] is None else float(opts["--rho"])
        if in_shape is not None and len(in_shape) != 3:
            raise ValueError("--in-shape is h,w,c")
        check_opts(opts["--arch"], opts["--opt"], rho, opts["--geometry"], flags["--audio"])
    except ValueError as e:
        print(USAGE if str(e).startswith(("invalid literal", "could not convert")) else "kws train: %s" % e)
        return 1
    from .._lib import EdisonError
    try:
        run(rest[0], rest[1], rest[2], rest[3], epochs=epochs, batch=batch, lr=lr, seed=seed, val=val, dropout=dropout, before_pool=before,
            dropout_arch=opts["--dropout-arch"], batchnorm=batchnorm, batchnorm_arch=opts["--batchnorm-arch"], bn_momentum=momentum, bn_eps=bn_eps,
            bn_unbiased=flags["--bn-unbiased"], arch=opts["--arch"], classes=classes, in_shape=in_shape, resident=flags["--resident"], audio=flags["--audio"],
            geometry=opts["--geometry"], opt=opts["--opt"], rho=rho)
    except (EdisonError, ValueError) as e:
        print("kws train: %s" % e)
        return 1
    return 0

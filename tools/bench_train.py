"""Training rate of the float32 network on the GPU (edison_ftrain_*): samples per second of one gradient call
plus one Adam step on the shipped network (tests/golden/cube_kws.ednf) at batch 100 -- the reference's batch -- and at 4096, and beside
them, from the same process, the forward-only rate of edison_fnet_batch on the same inputs: the yardstick a gradient is priced against.

Device calls on the context's stream: inputs and labels are device tensors, nothing is staged. A region is `--region-ms` of calls
between two host clock readings, ended by a device synchronise, so it holds the enqueue cost as well as the kernels; the legs alternate
(train, forward, train, ...), `--repeats` regions each, after a warm-up of every shape. Reported per batch: the median over regions of
samples per second, its minimum and maximum. The learning rate is 0, so the weights the forward leg runs never move.

    python tools/bench_train.py [--net FILE.ednf] [--batches 100,4096] [--repeats 7] [--region-ms 300] [--out FILE.json]
                                [--dropout 0,0,0.2,0.3,0 | --dropout-arch kws_conv] [--dropout-before-pool 0,1,..]
                                [--batchnorm [1,1,1,1,0]]
    python tools/bench_train.py --fit [--fit-rows 8192] [--fit-batch 100] [--repeats 7] [--out FILE.json]

--net: another float network than the shipped one, 'same' convs and pools included (the trainer is created with padded=True; on a
network without pads that is the plain trainer).

--dropout: the training leg runs with these Dropout rates per conv / dense record, a new mask every call.

--batchnorm: the training leg runs with BatchNorm behind these records (without a value: kws_conv's
1,1,1,1,0), on the network's geometry with its loaded weights as the starting master weights; the forward leg then runs the folded
network. "launches" is the number of kernel launches of one training call plus one step (the fold included), which depends on the
records and not on the batch.

--fit: another measurement (report only, no threshold): wall-clock seconds of one epoch of Trainer.fit, which gathers each batch on the
host and synchronises per batch, and of Trainer.fit_data on a device-resident data set, one library call and one synchronisation an
epoch. A plain kws_conv built by train.get_model on the shipped geometry, --fit-rows rows (8192), batch
--fit-batch (100), the two run alternately in one process after a warm-up epoch of each, median of --repeats; then the same pair with one
validation pass over as many rows. The other options do not apply.

One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dropout_on(spec):
    return [(s[0] if isinstance(s, (tuple, list)) else s) > 0 for s in spec]


def fit_main(args):
    """Seconds an epoch of Trainer.fit against Trainer.fit_data, without and with a validation pass."""
    import torch
    from edison_amd import cube_import, train
    from edison_amd.context import Context
    if not torch.cuda.is_available():
        sys.exit("bench_train: no GPU (there is no CPU path to time)")
    ctx = Context(0)
    model = train.get_model("kws_conv")
    ctx.fnet_load(cube_import.build_blob(model))
    n, bs = args.fit_rows, args.fit_batch
    rng = np.random.default_rng(19)
    x = rng.normal(0, 30, (n, int(np.prod(model["in_shape"])))).astype(np.float32)
    y = (np.arange(n) % 10).astype(np.int32)
    tr = ctx.trainer(padded=True)
    data = ctx.train_data(x, y)
    kw = dict(epochs=1, batch_size=bs, lr=0.0, callbacks=False)          # lr 0: every epoch of either leg runs the same weights

    def timed(call):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        return time.perf_counter() - t0

    legs = dict(fit=lambda: tr.fit(x, y, **kw), fit_data=lambda: tr.fit_data(data, **kw),
                fit_val=lambda: tr.fit(x, y, val=(x, y), **kw), fit_data_val=lambda: tr.fit_data(data, val=data, **kw))
    for call in legs.values():
        call()
    secs = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, call in legs.items():
            secs[k].append(timed(call))
    row = dict(mode="fit", network="kws_conv (train.get_model)", device=torch.cuda.get_device_name(0), rows=n, batch=bs, steps_per_epoch=-(-n // bs),
               repeats=args.repeats, seconds_per_epoch={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in secs.items()})
    row["fit_over_fit_data"] = row["seconds_per_epoch"]["fit"]["median"] / row["seconds_per_epoch"]["fit_data"]["median"]
    row["fit_over_fit_data_with_validation"] = row["seconds_per_epoch"]["fit_val"]["median"] / row["seconds_per_epoch"]["fit_data_val"]["median"]
    data.close()
    tr.close()
    ctx.close()
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default=os.path.join(ROOT, "tests", "golden", "cube_kws.ednf"))
    ap.add_argument("--batches", default="100,4096")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--region-ms", type=float, default=300.0)
    ap.add_argument("--out")
    ap.add_argument("--dropout")
    ap.add_argument("--dropout-before-pool")
    ap.add_argument("--dropout-arch")
    ap.add_argument("--batchnorm", nargs="?", const="1,1,1,1,0")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--fit-rows", type=int, default=8192)
    ap.add_argument("--fit-batch", type=int, default=100)
    args = ap.parse_args()
    if args.fit:
        return fit_main(args)
    import torch
    from edison_amd.context import Context
    if not torch.cuda.is_available():
        sys.exit("bench_train: no GPU (there is no CPU path to time)")
    ctx = Context(0)
    ctx.fnet_load(args.net)
    info = ctx.fnet_info()
    in_n, n_out = info["in_h"] * info["in_w"] * info["in_c"], info["n_out"]
    dev = torch.device("cuda", 0)
    ctx.use_torch_stream()
    tr = ctx.trainer(padded=True)
    from edison_amd import train
    dropout = train.KERAS_DROPOUT[args.dropout_arch] if args.dropout_arch else [float(v) for v in args.dropout.split(",")] if args.dropout else None
    if dropout is not None:
        tr.set_dropout(dropout, [int(v) for v in args.dropout_before_pool.split(",")] if args.dropout_before_pool else None, seed=19)
    batches = [int(b) for b in args.batches.split(",")]
    launches = 3                                            # the gradient kernel, the slab reduce, the step
    if args.batchnorm:
        has_bn = [int(v) for v in args.batchnorm.split(",")]
        tr.set_batchnorm(has_bn, max_rows=max(batches))
        n_bn, nl = sum(has_bn), len(has_bn)
        # keys (with dropout), per record conv + apply and the backward launch, per BatchNorm record stats + two for dy's sums, the loss,
        # the slab reduce, two steps (weights; gamma and beta) and the fold
        launches = (1 if dropout is not None and any(dropout_on(dropout)) else 0) + 3 * nl + 3 * n_bn + 1 + 1 + 2 + 1
    tinfo = tr.info()
    rng = np.random.default_rng(19)
    row = dict(network=os.path.basename(args.net), device=torch.cuda.get_device_name(0), train_batch=tinfo["batch"], grid=tinfo["grid"], lds_bytes=tinfo["lds_bytes"],
               w_floats=tinfo["w_floats"], dropout=tr.dropout()["rates"], dropout_before_pool=tr.dropout()["before_pool"], batchnorm=tr.batchnorm()["has_bn"], bn_batch=tr.batchnorm()["batch"], launches=launches, repeats=args.repeats, region_ms=args.region_ms, results=[])
    for n in batches:
        x = torch.from_numpy(rng.normal(0, 30, (n, in_n)).astype(np.float32)).to(dev)
        y = torch.from_numpy((np.arange(n) % n_out).astype(np.int32)).to(dev)
        loss = torch.zeros(n, dtype=torch.float32, device=dev)
        am = torch.zeros(n, dtype=torch.int32, device=dev)
        logits = torch.zeros((n, n_out), dtype=torch.float32, device=dev)

        def train_call():
            tr.grad_t(x, y, n, loss=loss, argmax=am)
            tr.step(0.0)

        def forward_call():
            ctx.fnet_t(x, n, logits=logits, argmax=am)

        def region(call):
            ctx.sync()
            calls, t0 = 0, time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < args.region_ms:
                for _ in range(8):
                    call()
                calls += 8
            ctx.sync()
            return calls * n / (time.perf_counter() - t0)

        for call in (train_call, forward_call):
            for _ in range(5):
                call()
        ctx.sync()
        rates = dict(train=[], forward=[])
        for _ in range(args.repeats):
            rates["train"].append(region(train_call))
            rates["forward"].append(region(forward_call))
        res = dict(batch=n)
        for k, v in rates.items():
            res[k + "_samples_per_s"] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
        res["train_over_forward"] = res["forward_samples_per_s"]["median"] / res["train_samples_per_s"]["median"]
        row["results"].append(res)
    tr.close()
    ctx.use_own_stream()
    ctx.close()
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()

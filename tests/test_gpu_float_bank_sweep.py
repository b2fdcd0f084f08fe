"""GPU tests (-m gpu) of the float bank over the rows of tests/float_bank_sweep.py: microphone counts against the network kernel's tiles
up to 4096 in both flows, shifts of float rows whose source and destination overlap, one slot of room, more than 256 frames in a push at
256 classes, outputs not asked for, clip range and input scale, resets, and pushes that leave microphones out -- the hold over
overlapping, touching and disjoint histories, the fill's rounds, 4096 workgroups. Every comparison is exact: float32 as uint32, the
final machines as raw fields.

Rows with more than 8 microphones play bank_sweep.BASES seeded recordings (microphone m plays base_of(m)). Two references:
  independent  no stream, no bank, none of the core's kernels: every frame's float row from the batch call on the zero-led recording
               (Context.kws_float(..., utt_stride=frame_step)["feat"], in the row's flow, clip range and scale), the windows cut in
               numpy behind F - 1 zero rows, Context.fnet on them, the logits also against the CPU fmaf chain (tests/fnet_host.py:
               every window of a recording of at most 2048, else the first and last 64), the filter in numpy
               (stream_drive.filter_ref) and edisonFSM from the host binding (stream.Fsm)
  streams      one stream.FloatStream per base recording and per reset, same options, same schedule: rows with resets only
A microphone's expected stream is the reference on the concatenation of the pushes it was present in since its last reset; the pushes
it was absent from carry noise over the whole int16 range, and at those its rows must hold the fill exactly."""
import numpy as np
import pytest

import bank_sweep as bs
import float_bank_sweep as fs
import fnet_host
import stream_drive as sd
from stream_drive import filter_ref, recordings, same

pytestmark = pytest.mark.gpu

ASKED = {"all": ("logits", "probs", "argmax"), "no_probs": ("logits", "argmax"), "no_logits": ("probs", "argmax"), "none": ()}


def _open(row):
    from edison_amd.context import Context
    c = Context(0, model_path=None)
    c.fnet_load(fs.blob_of(row["net"], row["geom"]))
    return c, fs.geometry(row)


# ---- the references ----------------------------------------------------------------------------------------------------------------
def _net_ref(c, g, row, model, x):
    """The network's outputs for every frame of recording x without a sliding buffer (see the module text)."""
    F, nm, hop = g.frame_count, g.num_mfcc, g.frame_step
    K = x.shape[0] // hop
    Kp = max(K, F)                               # the batch call needs one full window: frames of silence behind a short recording
    z = np.concatenate([np.zeros(max(0, g.frame_len - hop), np.int16), x, np.zeros((Kp - K) * hop, np.int16)])
    feat = c.kws_float(z, g, q15=row["q15"], n_utt=Kp - F + 1, utt_stride=hop, clip_min=row["clip"][0], clip_max=row["clip"][1])["feat"].reshape(-1, F, nm)
    rows = np.concatenate([feat[0], feat[1:, F - 1]])[:K]
    r = np.concatenate([np.zeros((F - 1, nm), np.float32), rows])
    win = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(r, (F, nm))[:, 0].reshape(K, -1))
    out = c.fnet(win)
    idx = np.arange(K) if K <= 2048 else np.concatenate([np.arange(64), np.arange(K - 64, K)])
    same(out["logits"][idx], fnet_host.run(model, win[idx])[-1], "the reference's logits against the fmaf chain")
    return out


def _finish_ref(g, row, net, thr):
    """The filter (numpy) and the state machine (host binding) behind the network outputs of one recording."""
    from edison_amd.stream import Fsm, _fsm_dict
    filt, likely, spotted = filter_ref(net["probs"], row["alpha"], thr)
    out = dict(net, filtered=filt, likely=likely, spotted=spotted)
    snap = None
    if row["fsm"]:
        f = Fsm(threshold=thr)
        dt = int(np.floor(g.frame_step * 1e6 / g.sample_rate))
        best = filt[np.arange(filt.shape[0]), likely]
        out["fsm_states"] = np.array([Fsm.STATES.index(f.step(float(b), int(i), dt)) for b, i in zip(best, likely)], np.int32)
        snap = _fsm_dict(f._f)["raw"]
    return out, snap


def _kind(row):
    return sd.Kind("float", q15=row["q15"])


def _expected(c, g, row, xb, base):
    """(dict of [K][n_mics][..], [final machine per microphone], threshold) from the row's reference."""
    from edison_amd import cube_import
    if row["ref"] == "streams":
        assert row["resets"] and not row["present"] and row["thr"] != "tie"

        def stream_of(x, life):
            """A new FloatStream fed recording x by the pushes of `life`: (dict of [frames][..], final machine)."""
            return sd.drive_stream(_kind(row), c, g, x, [row["sched"][p] for p in life], chunk=row["chunk"], filt=True, fsm=row["fsm"],
                                   alpha=row["alpha"], threshold=row["thr"], clip_min=row["clip"][0], clip_max=row["clip"][1])

        return sd.masked_expected(row, xb, base, g.frame_step, stream_of, lambda net, thr: net)
    model = cube_import.read_blob(fs.blob_of(row["net"], row["geom"]))
    return sd.masked_expected(row, xb, base, g.frame_step, lambda x, life: _net_ref(c, g, row, model, x), lambda net, thr: _finish_ref(g, row, net, thr))


# ---- the bank ------------------------------------------------------------------------------------------------------------------------
def _bank(c, g, row, x, thr):
    """The bank on x [n_mics][K * hop] by the row's schedule, pushes, masks, resets and outputs. Returns (dict of [K][n_mics][..] without
    what was not asked for, [final machine per microphone])."""
    return sd.drive_bank(_kind(row), c, g, x, row["sched"], chunk=row["chunk"], filt=True, fsm=row["fsm"], alpha=row["alpha"], threshold=thr,
                         asked=ASKED[row["outputs"]], counts=sd.present_counts(row), clip_min=row["clip"][0], clip_max=row["clip"][1],
                         **sd.pushes_of(row))


def _run_row(name):
    """One row: the bank against its reference, every output key the row asks for, and the final machines."""
    row = fs.ROWS[name]
    c, g = _open(row)
    try:
        assert int(c.fnet_info()["batch"]) == fs.plan_of(row["net"], row["geom"])["batch"]      # the tiles the walk counted
        M, K = row["n_mics"], sum(row["sched"])
        base = [bs.base_of(m, M) for m in range(M)]
        assert all(base[m] != base[m + 1] for m in range(M - 1))
        xb = recordings(g, max(base) + 1, K, 500 + len(name))
        exp, exp_snaps, thr = _expected(c, g, row, xb, base)
        x = xb[base]
        got, snaps = _bank(c, g, row, sd.garbage(row, x, g.frame_step) if row["present"] else x, thr)
        compared = 0
        for k in sd.Kind("float").keys(True, True):
            if k not in exp or got.get(k) is None:
                assert k in ("logits", "probs", "argmax", "fsm_states"), (name, k)
                continue
            same(got[k], exp[k], "%s %s" % (name, k))
            compared += 1
        assert compared >= 3 and (row["outputs"] != "all" or compared == len(exp))
        assert snaps == (exp_snaps if row["fsm"] else []), name
        if len(xb) > 1:
            assert not np.array_equal(exp["logits"][:, 0], exp["logits"][:, 1])      # the recordings do differ
        if tuple(row["clip"]) != fs.DEFAULT_CLIP:
            assert exp["logits"].any()            # (the clip is the reference's too: Context.kws_float's clip_min / clip_max)
    finally:
        c.close()


def test_rows_cover_every_item_at_this_gpus_cu_count():
    from edison_amd.context import Context
    c = Context(0, model_path=None)
    try:
        n_cu = c.device_info()["n_cu"]
    finally:
        c.close()
    have = set().union(*(fs.walk(r, n_cu=n_cu, check=False)[0] for r in fs.ROWS.values()))
    assert sorted(fs.full_set() - set(fs.EXCLUDED) - have, key=str) == []
    assert not set(fs.EXCLUDED) & have


@pytest.mark.parametrize("name", list(fs.ROWS))
def test_row(built_lib, name):
    _run_row(name)

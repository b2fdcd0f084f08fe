"""GPU tests (-m gpu) of the stream bank over the rows of tests/bank_sweep.py: microphone counts against every network kernel's units
up to 4096, push shapes, shifts whose source and destination overlap, one slot of room, more than 256 frames in a push, outputs not
asked for, resets. Every comparison is exact (np.array_equal): the pipeline is integer but for the filter, whose arithmetic is fixed.

Rows with more than 8 microphones play bank_sweep.BASES seeded recordings (microphone m plays base_of(m)), so the reference is that
many streams whatever the row's size. Two references:
  streams      one stream.GeomStream per base recording (and per reset: a new stream fed the rest), same options, same schedule
  independent  no sliding buffer and no shift kernel: every frame's int8 row from the batch float64 MFCC (Context.mfcc_geom) on the
               zero-led recording, the windows cut in numpy behind F - 1 zero rows, Context.net on them, the filter in numpy
               (stream_drive.filter_ref) and edisonFSM from the host binding (stream.Fsm).
Rows with masks (present) use the independent reference: a microphone's expected stream is that reference on the concatenation of the
pushes it was present in (since its last reset), the pushes it was absent from carry noise over the whole int16 range, and at those its
rows must hold the fill exactly: zero bytes, -1, its machine's unchanged state; frames_seen_mics() counts the present frames."""
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

import bank_sweep as bs
import stream_drive as sd
from geom_sweep import header
from stream_drive import filter_ref, recordings, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_PROCESS = [n for n, r in bs.ROWS.items() if r["route"] != "lbl"]
LBL = [n for n, r in bs.ROWS.items() if r["route"] == "lbl"]
KIND = sd.Kind("int8")
ASKED = {"all": ("logits", "softmax", "argmax"), "no_softmax": ("logits", "argmax"), "no_logits": ("softmax", "argmax"), "none": ()}


def _open(row):
    from edison_amd.context import Context
    if row["graph"] == "shipped":
        return Context(0), bs.geometry(row["geom"])
    c = Context(0, model_path=None)
    c.load_weights_h(header(row["graph"]))
    return c, bs.geometry(row["geom"])


def _starts(row):
    """[per push: {microphone: the push its stream last started at}] after the resets in front of that push."""
    cur, out = {m: 0 for m in range(row["n_mics"])}, []
    for p in range(len(row["sched"])):
        for at, who in row["resets"]:
            if at == p:
                cur.update({m: p for m in (range(row["n_mics"]) if who == "all" else [who])})
        out.append(dict(cur))
    return out


# ---- the references ----------------------------------------------------------------------------------------------------------------
def _net_ref(c, g, x):
    """The network's outputs for every frame of recording x without a sliding buffer (see the module text)."""
    K, F, nm = x.shape[0] // g.frame_step, g.frame_count, g.num_mfcc
    z = np.concatenate([np.zeros(max(0, g.frame_len - g.frame_step), np.int16), x])
    y = c.mfcc_geom(z, replace(g, frame_count_=K, n_samples=z.shape[0]), n_utt=1)[0]
    # mfcc_geom_kernels.hip:32-33, kws_nnom.py:359-361: float32 product, clip, round half to even
    rows = np.rint(np.clip(y.astype(np.float32) * np.float32(g.net_input_scale), -128.0, 127.0)).astype(np.int8)
    r = np.concatenate([np.zeros((F - 1, nm), np.int8), rows])
    win = np.lib.stride_tricks.sliding_window_view(r, (F, nm))[:, 0].reshape(K, F * nm)
    return c.net(np.ascontiguousarray(win))


def _finish_ref(c, g, row, net, thr):
    """The filter (numpy) and the state machine (host binding) behind the network outputs of one recording."""
    from edison_amd.stream import Fsm, _fsm_dict
    xin = net["softmax"] if net["softmax"] is not None else net["logits"]
    filt, likely, spotted = filter_ref(xin, row["alpha"], thr)
    out = dict(net, filtered=filt, likely=likely, spotted=spotted)
    snap = None
    if row["fsm"]:
        f = Fsm(threshold=thr)
        dt = int(np.floor(g.frame_step * 1e6 / g.sample_rate))
        best = filt[np.arange(filt.shape[0]), likely]
        out["fsm_states"] = np.array([Fsm.STATES.index(f.step(float(b), int(i), dt)) for b, i in zip(best, likely)], np.int32)
        snap = _fsm_dict(f._f)["raw"]
    return out, snap


def _expected(c, g, row, xb, base):
    """(dict of [K][n_mics][..], [final machine per microphone], threshold) from the row's reference."""
    M, sched = row["n_mics"], row["sched"]
    K = sum(sched)
    starts = _starts(row)
    thr = row["thr"]
    refs = {}
    if row["ref"] == "independent":
        assert not row["resets"]
        nets = [_net_ref(c, g, x) for x in xb]
        if thr == "tie":
            # a threshold that a filtered maximum equals exactly: the middle one of the reference's own maxima (strict >: not spotted)
            best = np.concatenate([filter_ref(n["softmax"] if n["softmax"] is not None else n["logits"], row["alpha"], 0.0)[0].max(axis=1) for n in nets])
            vals = np.unique(best)
            thr = float(vals[len(vals) // 2])
            assert (best == np.float32(thr)).any() and (best > thr).any(), "no tie to test"
        for b in range(len(xb)):
            refs[(b, 0)] = _finish_ref(c, g, row, nets[b], thr)
    else:
        assert thr != "tie"
        for key in sorted({(base[m], p0) for st in starts for m, p0 in st.items()}):
            # a new GeomStream fed the base recording from push key[1] on, by the row's schedule
            refs[key] = sd.drive_stream(KIND, c, g, xb[key[0]], row["sched"], chunk=row["chunk"], filt=True, fsm=row["fsm"], alpha=row["alpha"],
                                        threshold=thr, first_push=key[1])
    info = c.net_info()
    no = info["n_out"]
    exp = dict(logits=np.zeros((K, M, no), np.int8), softmax=np.zeros((K, M, no), np.int8) if info["has_softmax"] else None,
               argmax=np.zeros((K, M), np.int32), filtered=np.zeros((K, M, no), np.float32), likely=np.zeros((K, M), np.int32),
               spotted=np.zeros((K, M), np.int32))
    if row["fsm"]:
        exp["fsm_states"] = np.zeros((K, M), np.int32)
    k0 = 0
    for p, n in enumerate(sched):
        for key in {(base[m], p0) for m, p0 in starts[p].items()}:
            mics = np.array([m for m, p0 in starts[p].items() if (base[m], p0) == key])
            lo = k0 - sum(sched[:key[1]])
            for k, v in exp.items():
                if v is not None:
                    v[k0:k0 + n, mics] = refs[key][0][k][lo:lo + n][:, None]
        k0 += n
    snaps = [refs[(base[m], starts[-1][m])][1] for m in range(M)]
    return exp, snaps, thr


# ---- the bank ------------------------------------------------------------------------------------------------------------------------
def _bank(c, g, row, x, thr):
    """The bank on x [n_mics][K * hop] by the row's schedule, pushes, resets and outputs. Returns (dict of [K][n_mics][..] without
    what was not asked for, [final machine per microphone])."""
    return sd.drive_bank(KIND, c, g, x, row["sched"], chunk=row["chunk"], filt=True, fsm=row["fsm"], alpha=row["alpha"], threshold=thr,
                         asked=ASKED[row["outputs"]], counts=sd.present_counts(row) if row["present"] else None, **sd.pushes_of(row))


def _run_row(name, tmp=None):
    """One row: the bank against its reference, every output key the row asks for, and the final machines."""
    from edison_amd import _lib
    row = bs.ROWS[name]
    c, g = _open(row)
    try:
        if row["route"] == "spec":
            try:
                c.net_specialize()
            except _lib.EdisonError as e:
                assert e.code == _lib.E_NO_IMPL
                return
        M, K = row["n_mics"], sum(row["sched"])
        base = [bs.base_of(m, M) for m in range(M)]
        assert all(base[m] != base[m + 1] for m in range(M - 1))
        xb = recordings(g, max(base) + 1, K, 300 + len(name))
        if row["present"]:
            assert row["ref"] == "independent"
            exp, exp_snaps, thr = sd.masked_expected(row, xb, base, g.frame_step, lambda x, life: _net_ref(c, g, x), lambda net, t: _finish_ref(c, g, row, net, t))
            got, snaps = _bank(c, g, row, sd.garbage(row, xb[base], g.frame_step), thr)
        else:
            exp, exp_snaps, thr = _expected(c, g, row, xb, base)
            got, snaps = _bank(c, g, row, xb[base], thr)
        compared = 0
        for k in KIND.keys(True, True):
            if k not in exp or exp[k] is None or got.get(k) is None:
                assert k in ("logits", "softmax", "argmax", "fsm_states"), (name, k)
                continue
            same(got[k], exp[k], "%s %s" % (name, k))
            compared += 1
        assert compared >= 3 and (row["outputs"] != "all" or compared == len([k for k in exp if exp[k] is not None]))
        assert snaps == (exp_snaps if row["fsm"] else []), name
        if len(xb) > 1:
            assert not np.array_equal(exp["logits"][:, 0], exp["logits"][:, 1])      # the recordings do differ
    finally:
        c.close()


def test_rows_cover_every_item_at_this_gpus_cu_count():
    from edison_amd.context import Context
    c = Context(0, model_path=None)
    try:
        n_cu = c.device_info()["n_cu"]
    finally:
        c.close()
    have = set().union(*(bs.walk(r, n_cu=n_cu, check=False)[0] for r in bs.ROWS.values()))
    assert sorted(bs.full_set() - set(bs.EXCLUDED) - have, key=str) == []
    assert not set(bs.EXCLUDED) & have and bs.ROWS["gen_cap"]["chunk"] > bs.general_cap(n_cu)


@pytest.mark.parametrize("name", IN_PROCESS)
def test_row(name, tmp_path, monkeypatch):
    row = bs.ROWS[name]
    monkeypatch.setenv("EDISON_JIT_CACHE", str(tmp_path))
    if row["route"] in ("general", "spec"):
        monkeypatch.setenv("EDISON_NET_FORCE_GENERAL", "1")
    else:
        monkeypatch.delenv("EDISON_NET_FORCE_GENERAL", raising=False)
    _run_row(name)


def test_layer_by_layer_rows_in_a_child_process(tmp_path):
    """EDISON_NET_NO_MFMA=1 is read once, when the library first launches a network: bank and reference run in one fresh process."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_bank_sweep as t
for name in %r:
    t._run_row(name)
print("child ok")
""" % (ROOT, os.path.join(ROOT, "tests"), LBL)
    env = dict(os.environ, EDISON_NET_NO_MFMA="1", EDISON_NET_FORCE_GENERAL="1", EDISON_JIT_CACHE=str(tmp_path))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])

"""The one driver of the stream and bank tests (test_gpu_stream_geom, test_gpu_stream_float, test_gpu_stream_bank, test_gpu_float_bank,
test_gpu_bank_present, test_gpu_bank_sweep, test_gpu_float_bank_sweep). Test infrastructure, not a test; tests/test_stream_drive_cpu.py
checks its pure pieces.

  Kind            one network type -- "int8" (GeomStream / StreamBank on an NNoM graph) or "float" (FloatStream / FloatBank on an
                  X-CUBE-AI network) -- behind the same calls: open, stream, bank, keys
  torch_stream    the context on torch's current stream for the length of a `with`
  outputs         the device tensors a schedule's outputs go to
  drive_stream    the device-push loop of one stream over a schedule of frame counts
  drive_bank      the same for a bank: masks, resets, host / device / device-without-output-pointers pushes
  reference, same_as_streams, host_pushes, cat   one stream per microphone, and a bank compared against them
  same            the one array comparison: bit for bit (float32 as uint32), shape and dtype included
  recording, recordings, tail, schedule, wraps, filter_ref, oracle_rows, start_machine, raw   signals, schedules and small references

The reaches into private members of the product's handles (s._h, s._fsm, b._fsms, _c) are gathered here."""
import contextlib
import ctypes
import functools
import os

import numpy as np

from bank_sweep import absent_of
from geom_sweep import GEOMS, geom, header, signals

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cube_kws.ednf")
SYNTH = [("conv", 8, (3, 3), (1, 1), (2, 2), 1), ("dense", 16), ("relu",), ("dense", 6), ("softmax",)]
HOST, DEV, DEV_NO_OUT = "host", "device", "device, no output pointers"


# ---- the two network types ----------------------------------------------------------------------------------------------------------
class Kind:
    """One network type, its single stream and its bank behind the same calls. `kind`, `second` (the name of the second output),
    `dtype` and `who` (the bank's message prefix) are fixed; `n_out`, `has_second`, `fsm`, `q15` and `model` (fnet_host's dict; None for
    int8) belong to what `open` or `of` last saw."""

    def __init__(self, kind, q15=False):
        assert kind in ("int8", "float"), kind
        self.kind, self.q15 = kind, q15
        self.second = "softmax" if kind == "int8" else "probs"
        self.who = "stream_bank" if kind == "int8" else "float_bank"
        self.dtype = np.int8 if kind == "int8" else np.float32
        self.n_out, self.has_second, self.fsm, self.model = None, True, False, None

    def open(self, name, geom_kw=None, layers=SYNTH):
        """(context with the model loaded, geometry). int8: the shipped graph, or the committed alt_models header `name` at
        GEOMS[name] (geom_kw: at these fields instead). float: "shipped" / "shipped_q15" are tests/golden/cube_kws.ednf in the host
        and in the firmware's flow; any other name a cube_synth network of `layers` at that geometry, seeded by len(name)."""
        from edison_amd.context import Context
        self.q15 = name.endswith("_q15")
        if self.kind == "int8":
            if name == "shipped":
                c, g = Context(0), geom(**(geom_kw or {}))
            else:
                c, g = Context(0, model_path=None), geom(**(geom_kw or GEOMS[name]))
                c.load_weights_h(header(name))
        else:
            from edison_amd import cube_import
            data, g = float_blob(name, geom_kw, layers)
            c = Context(0, model_path=None)
            c.fnet_load(data)
            self.model = cube_import.read_blob(data)
        return self.of(c), g

    def of(self, c):
        """Take n_out, has_second and fsm (edisonFSM runs on 10 outputs) from the model loaded on context c; returns c."""
        if self.kind == "int8":
            info = c.net_info()
            self.n_out, self.has_second = int(info["n_out"]), bool(info["has_softmax"])
        else:
            self.n_out, self.has_second = int(c.fnet_info()["n_out"]), True
        self.fsm = self.n_out == 10
        return c

    def _opts(self, opts):
        opts = {k: v for k, v in opts.items() if v is not None}        # None: the class's own default (alpha 0.9 / 0.5)
        if self.kind == "float":
            opts.setdefault("q15", self.q15)
        return opts

    def stream(self, c, g, chunk, **opts):
        from edison_amd import stream
        return (stream.GeomStream if self.kind == "int8" else stream.FloatStream)(c, g, chunk_frames=chunk, **self._opts(opts))

    def bank(self, c, g, n_mics, chunk, **opts):
        from edison_amd import stream
        if self.kind == "int8":
            return stream.StreamBank(c, g, n_mics, chunk_frames=chunk, **self._opts(opts))
        return stream.FloatBank(c, n_mics, g, chunk_frames=chunk, **self._opts(opts))

    def net_keys(self):
        return ("logits", self.second, "argmax")

    def all_keys(self):
        return self.net_keys() + ("filtered", "likely", "spotted", "fsm_states")

    def keys(self, filt=True, fsm=True):
        """The names of the outputs there are, in the order the tests walk them."""
        return ["logits"] + ([self.second] if self.has_second else []) + ["argmax"] + (["filtered", "likely", "spotted"] if filt or fsm else []) + \
            (["fsm_states"] if fsm else [])


def float_blob(name, geom_kw=None, layers=SYNTH):
    """(the .ednf bytes of a float network, its geometry): see Kind.open."""
    return _float_blob(name, None if geom_kw is None else tuple(sorted(geom_kw.items())), tuple(layers))


@functools.lru_cache(maxsize=None)
def _float_blob(name, geom_items, layers):
    import cube_synth
    from edison_amd import config as cfg
    from edison_amd.kws.geometry import KwsGeometry
    if name.startswith("shipped"):
        return open(FIXTURE, "rb").read(), KwsGeometry.from_config(net_input_scale=cfg.net_input_scale)
    g = geom(**(GEOMS[name] if geom_items is None else dict(geom_items)))
    return import_sources(cube_synth.cube_sources((g.frame_count, g.num_mfcc, 1), list(layers), seed=len(name))), g


def import_sources(sources):
    """(net_c, data_c) in X-CUBE-AI's format -> .ednf bytes."""
    import tempfile
    from edison_amd import cube_import
    with tempfile.TemporaryDirectory() as d:
        for fname, text in zip(("n.c", "n_data.c"), sources):
            with open(os.path.join(d, fname), "w") as f:
                f.write(text)
        return cube_import.import_files(os.path.join(d, "n.c"), os.path.join(d, "n_data.c"))


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    """Bit for bit: the same shape, the same dtype, float32 compared as uint32 (-0.0 is not +0.0, a NaN equals its own bit pattern)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(bits(got) != bits(want))
    at = tuple(int(i) for i in bad[0]) if bad.shape[0] else None
    assert at is None, "%s: %d of %d differ, first at %s: %r != %r" % (what, bad.shape[0], got.size, at, got[at], want[at])


def same_as_streams(K, got, ref, what, mics=None, rows=slice(None)):
    """Microphone m of the bank's outputs equals reference stream m's, in every output the reference has."""
    for m in (range(len(ref)) if mics is None else mics):
        for k in K.all_keys():
            if k not in ref[m]:
                assert k not in got, (what, k)
            elif ref[m][k] is None:
                assert got[k] is None, (what, k)
            else:
                same(got[k][rows, m], ref[m][k], "%s microphone %d %s" % (what, m, k))


def host_pushes(h, x, pushes, first=0):
    """Host pushes `first` .. of chunk frames each into a stream (x [samples]) or a bank (x [n_mics][samples]): the list of push dicts."""
    n = h.chunk * h.hop
    return [h.push(x[..., i * n:(i + 1) * n]) for i in range(first, first + pushes)]


def cat(K, parts):
    """The array outputs of consecutive pushes (host push dicts or driver results), put together."""
    return {k: (None if parts[0][k] is None else np.concatenate([p[k] for p in parts])) for k in K.all_keys() if k in parts[0]}


# ---- signals, schedules, small references -------------------------------------------------------------------------------------------
def tail(g):
    return max(0, g.frame_len - g.frame_step)


def recording(g, n_frames, seed):
    """n_frames hops of the geom_sweep.signals mix (silence, noise, tones, clipping, the `edison` utterance) back to back."""
    n = n_frames * g.frame_step
    per = max(g.n_samples, 8000)
    return signals(-(-n // per) + 1, per, seed).ravel()[:n].copy()


def recordings(g, n_mics, n_frames, seed):
    """int16 [n_mics][n_frames * hop]: another recording for every microphone -- the geom_sweep.signals mix (silence, noise, tones,
    clipping, the `edison` utterance) in stretches of five hops, seeded per microphone and starting at another kind."""
    per = 5 * g.frame_step
    rows = -(-n_frames // 5) + 5
    return np.stack([signals(rows, per, seed + 17 * m)[1 + m % 4:].ravel()[:n_frames * g.frame_step] for m in range(n_mics)])


def by_push(i, chunk):
    """The ragged length of test_gpu_stream_bank's and test_gpu_float_bank's schedules."""
    return 1 + i % (chunk - 1)


def by_round(i, chunk):
    """The ragged length of test_gpu_bank_present's schedules: 1 .. chunk - 1 in turn."""
    return 1 + (i // 4) % (chunk - 1)


def schedule(chunk, pushes, ragged=by_push):
    """Frames per push: full pushes, with a ragged one of ragged(i, chunk) < chunk frames at every push i = 2 mod 4 where the chunk
    allows one (ragged=None: full pushes only)."""
    return [chunk if ragged is None or chunk == 1 or i % 4 != 2 else ragged(i, chunk) for i in range(pushes)]


def whole(n_frames, chunk):
    """n_frames in pushes of chunk frames and a ragged last one."""
    return [chunk] * (n_frames // chunk) + [n_frames % chunk] * (n_frames % chunk != 0)


def wraps(frames, chunk, slots=8):
    """The pushes before which the core moves the history to the front (make_room: pos + n > slots * chunk)."""
    pos, at = 0, []
    for k, n in enumerate(frames):
        if pos + n > slots * chunk and pos != 0:
            at.append(k)
            pos = 0
        pos += n
    return at


def filter_ref(x, alpha, threshold):
    """The firmware's filter over n_out classes in numpy: float64 product, float64 sum (each rounded), float32 state; first maximum."""
    y = np.zeros(x.shape[1], np.float32)
    oma = 1.0 - alpha
    filt = np.zeros(x.shape, np.float32)
    for i in range(x.shape[0]):
        y = (alpha * y.astype(np.float64) + oma * x[i].astype(np.float64)).astype(np.float32)
        filt[i] = y
    likely = np.argmax(filt, axis=1).astype(np.int32)
    best = filt[np.arange(x.shape[0]), likely].astype(np.float64)
    return filt, likely, np.where(best > threshold, likely, -1).astype(np.int32)


def oracle_rows(oracle_mod, g, x):
    """int8 [K][num_mfcc]: the host flow's row of every frame of the stream on x."""
    import geom_sweep
    from dataclasses import replace
    K = x.shape[0] // g.frame_step
    z = np.concatenate([np.zeros(tail(g), np.int16), x])
    gk = replace(g, frame_count_=K, n_samples=z.shape[0])
    y = geom_sweep.oracle_mfcc(oracle_mod, z[None, :], gk)
    return geom_sweep.oracle_feat(oracle_mod, y, gk).reshape(K, g.num_mfcc)


def raw(f):
    return (f.state, f.hot_timeout_ms, f.wake_idx, f.loc_idx, f.val_idx, f.last_loc, f.last_val, f.commands)


def start_machine():
    """The raw fields of edison_fsm_init's machine: what a stream starts its first push with."""
    from edison_amd import _lib
    f = _lib.Fsm()
    _lib.lib().edison_fsm_init(ctypes.byref(f))
    return raw(f)


# ---- the device side ----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def torch_stream(c):
    """The context on torch's current stream: yields (torch, the context's device); back on its own stream afterwards."""
    import torch
    dev = torch.device("cuda", c.device)
    c.use_torch_stream(torch.cuda.current_stream(dev))
    try:
        yield torch, dev
    finally:
        c.use_own_stream()


def outputs(K, torch, dev, shape, filt, fsm):
    """Device tensors for the outputs of a schedule: shape = (rows,) for a stream, (rows, n_mics) for a bank. The second output is None
    where the graph has none."""
    tdt = torch.int8 if K.dtype == np.int8 else torch.float32
    z = lambda last, dt: torch.zeros(tuple(shape) + last, dtype=dt, device=dev)
    o = {"logits": z((K.n_out,), tdt), K.second: z((K.n_out,), tdt) if K.has_second else None, "argmax": z((), torch.int32)}
    if filt or fsm:
        o.update(filtered=z((K.n_out,), torch.float32), likely=z((), torch.int32), spotted=z((), torch.int32))
    if fsm:
        o.update(fsm_states=z((), torch.int32))
    return o


def _to_host(o):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _rows(K, o, sl, asked=None):
    """A stream's push_t output arguments: rows sl of the tensors o; of the network's three only those `asked` for (None: all three)."""
    skip = () if asked is None else set(K.net_keys()) - set(asked)
    return {k: (None if v is None or k in skip else v[sl]) for k, v in o.items() if k != "fsm_states"}


def drive_stream(K, c, g, x, sched, *, chunk, stream=None, filt=False, fsm=False, alpha=None, threshold=None, first_push=0, **opts):
    """Device pushes of recording x (from push `first_push` of `sched` on, x's samples before it skipped) into a new stream of K -- or
    into `stream`, which goes on from where it is and stays open -- a push of n < chunk frames through n_frames=. With fsm the states
    of every push are fetched behind it and the final machine at the end. Returns (dict of host arrays [frames][..], the machine's raw
    fields or None)."""
    K.of(c)
    hop, skip = g.frame_step, sum(sched[:first_push])
    sched = sched[first_push:]
    with torch_stream(c) as (torch, dev):
        s = stream or K.stream(c, g, chunk, output_filter=filt, fsm=fsm, alpha=alpha, threshold=threshold, **opts)
        try:
            before = s.frames_seen
            xt = torch.from_numpy(x[skip * hop:]).to(dev)
            o = outputs(K, torch, dev, (sum(sched),), filt, fsm)
            k0 = 0
            for n in sched:
                sl = slice(k0, k0 + n)
                s.push_t(xt[k0 * hop:(k0 + n) * hop], n_frames=None if n == s.chunk else n, **_rows(K, o, sl))
                if fsm:
                    c._check(s._c("fsm_dev")(s._h, ctypes.c_void_p(o["fsm_states"][sl].data_ptr())))
                k0 += n
            torch.cuda.synchronize(dev)
            machine = None
            if fsm:
                c._check(s._c("fsm")(s._h, ctypes.byref(s._fsm), None))
                machine = raw(s._fsm)
            assert s.frames_seen == before + k0
        finally:
            if stream is None:
                s.close()
    return _to_host(o), machine


def drive_bank(K, c, g, x, sched, *, chunk, bank=None, filt=False, fsm=False, alpha=None, threshold=None, present=None, mode=DEV, resets=None,
               asked=None, counts=None, **opts):
    """The bank on x [n_mics][frames * hop] by the same schedule: a new bank of K, or `bank`, which goes on from where it is and stays
    open. present: per push a uint8 [n_mics] mask or None; resets {push: ["all" or a microphone, ..]}, done in front of that push.
    mode, one for all pushes or one per push:
      HOST         b.push on the bank's own stream (one mode for all) or on torch's (in a list); every output comes back
      DEV          b.push_t into the caller's tensors; of logits / second / argmax only those `asked` for get a pointer (None: all)
      DEV_NO_OUT   b.push_t with none of the three
    counts: what frames_seen_mics() must give at the end.
    Returns (dict of host arrays [frames][n_mics][..] -- without the network outputs no device push asked for -- and the final
    machines' raw fields per microphone, [] without fsm)."""
    K.of(c)
    M, hop, resets = x.shape[0], g.frame_step, resets or {}
    modes = [mode] * len(sched) if isinstance(mode, str) else list(mode)
    asked = K.net_keys() if asked is None else asked
    with (contextlib.nullcontext((None, None)) if mode == HOST else torch_stream(c)) as (torch, dev):
        b = bank or K.bank(c, g, M, chunk, output_filter=filt, fsm=fsm, alpha=alpha, threshold=threshold, **opts)
        try:
            before = b.frames_seen()
            if torch is not None:
                X = torch.from_numpy(x).to(dev)
                o = outputs(K, torch, dev, (sum(sched), M), filt, fsm)
            k0, parts = 0, []
            for p, n in enumerate(sched):
                for who in resets.get(p, ()):
                    b.reset() if who == "all" else b.reset_mic(who)
                sl, mask = slice(k0, k0 + n), None if present is None else present[p]
                if modes[p] == HOST:
                    assert n == b.chunk
                    out = b.push(x[:, k0 * hop:(k0 + n) * hop], present=mask)
                    assert (out["present"] is None) if mask is None else np.array_equal(out["present"], mask)
                    parts.append((sl, out))
                else:
                    kw = _rows(K, o, sl, () if modes[p] == DEV_NO_OUT else asked)
                    if fsm:
                        kw.update(fsm_states=o["fsm_states"][sl])
                    b.push_t(X[:, k0 * hop:(k0 + n) * hop].contiguous(), n_frames=None if n == b.chunk and mask is None else n,
                             present=None if mask is None else torch.from_numpy(mask).to(dev), **kw)
                k0 += n
            if torch is not None:
                torch.cuda.synchronize(dev)
            machines = []
            if fsm:
                c._check(b._c("fsm")(b._h, ctypes.byref(b._fsms), None))
                machines = [raw(f) for f in b._fsms]
            if not any("all" in who for who in resets.values()):
                assert b.frames_seen() == before + k0
            assert counts is None or np.array_equal(b.frames_seen_mics(), counts)
        finally:
            if bank is None:
                b.close()
    if torch is None:
        return cat(K, [out for _, out in parts]), machines
    got = _to_host(o)
    for sl, out in parts:
        for k in got:
            if got[k] is not None:
                got[k][sl] = out[k]
    if any(m != HOST for m in modes):
        given = set().union(*[() if m == DEV_NO_OUT else asked for m in modes if m != HOST])
        got = {k: v for k, v in got.items() if k in given or k not in K.net_keys()}
    return got, machines


def reference(K, c, g, x, sched, **kw):
    """One stream per microphone of x [n_mics][..], device pushes by the schedule: ([per microphone: dict of [frames][..]], [final
    machines' raw fields], [] without fsm)."""
    runs = [drive_stream(K, c, g, x[m], sched, **kw) for m in range(x.shape[0])]
    return [r[0] for r in runs], [r[1] for r in runs if r[1] is not None]


# ---- the sweeps' rows (bank_sweep.ROWS, float_bank_sweep.ROWS): pushes, masks and what a masked row must give ------------------------
def pushes_of(row):
    """A row's push modes, masks and resets, as drive_bank takes them: "host" rows push from the host, "alt" rows every other full
    push, the others from the device; a mask for every push the row gives one."""
    modes, masks, fulls = [], [], 0
    for p, n in enumerate(row["sched"]):
        host = row["push"] == "host" or (row["push"] == "alt" and n == row["chunk"] and fulls % 2 == 0)
        fulls += n == row["chunk"]
        modes.append(HOST if host else DEV)
        masks.append(None)
        if row["present"] and row["present"][p] is not None:
            masks[p] = np.ones(row["n_mics"], np.uint8)
            masks[p][absent_of(row, p)] = 0
    resets = {}
    for at, who in row["resets"]:
        resets.setdefault(at, []).append(who)
    return dict(mode=modes, present=masks, resets=resets)


def lives_of(row):
    """Per microphone the lives of its stream, a new one at every reset: [[the pushes it was present in] per life]."""
    M = row["n_mics"]
    lives = [[[]] for _ in range(M)]
    for p in range(len(row["sched"])):
        for at, who in row["resets"]:
            if at == p:
                for m in (range(M) if who == "all" else [who]):
                    lives[m].append([])
        gone = set(absent_of(row, p))
        for m in range(M):
            if m not in gone:
                lives[m][-1].append(p)
    return lives


def present_counts(row):
    """frames_seen_mics() after the schedule: the frames of the pushes a microphone was present in since the last reset of the bank."""
    first = max([at for at, who in row["resets"] if who == "all"], default=0)
    counts = np.zeros(row["n_mics"], np.int64)
    for p, n in enumerate(row["sched"]):
        if p >= first:
            counts += n
            counts[absent_of(row, p)] -= n
    return counts


def garbage(row, x, hop, seed=11):
    """The push buffers: x [n_mics][K * hop] with the samples of every absent microphone replaced by noise over the whole int16 range."""
    rng = np.random.default_rng(seed)
    y, k0 = x.copy(), 0
    for p, n in enumerate(row["sched"]):
        gone = absent_of(row, p)
        if gone:
            y[gone, k0 * hop:(k0 + n) * hop] = rng.integers(-32768, 32768, (len(gone), n * hop)).astype(np.int16)
        k0 += n
    return y


def masked_expected(row, xb, base, hop, net_of, finish):
    """(dict of [K][n_mics][..], [final machine per microphone], threshold) for a row with masks or resets, for either bank.
    net_of(x, life): the network's outputs for every frame of recording x, the pushes `life` of the schedule put together, with no
    sliding buffer; finish(net, thr): (those with the filter's and the machine's behind them, the final machine). Microphones that play
    the same base recording through the same lives share a reference."""
    M, sched = row["n_mics"], row["sched"]
    off = np.concatenate([[0], np.cumsum(sched)])
    groups = {}
    for m, lv in enumerate(lives_of(row)):
        resets_at = tuple(sorted(at for at, who in row["resets"] if who in ("all", m)))
        groups.setdefault((base[m], tuple(tuple(life) for life in lv), resets_at), []).append(m)
    nets = {}
    for b, lv, _ in groups:
        for life in lv:
            if life and (b, life) not in nets:
                nets[(b, life)] = net_of(np.concatenate([xb[b][off[p] * hop:off[p + 1] * hop] for p in life]), life)
    thr = row["thr"]
    if thr == "tie":
        # a threshold that a filtered maximum equals exactly: the middle one of the reference's own maxima (strict >: not spotted)
        best = np.concatenate([filter_ref(_filter_input(n), row["alpha"], 0.0)[0].max(axis=1) for n in nets.values()])
        vals = np.unique(best)
        thr = float(vals[len(vals) // 2])
        assert (best == np.float32(thr)).any() and (best > thr).any(), "no tie to test"
    refs = {k: finish(n, thr) for k, n in nets.items()}
    some = next(iter(refs.values()))[0]
    exp = {k: (None if v is None else np.full((off[-1], M) + v.shape[1:], -1 if k in ("argmax", "likely", "spotted", "fsm_states") else 0, v.dtype))
           for k, v in some.items()}
    snaps, new = [None] * M, start_machine()          # a new machine's raw fields, its state first
    for (b, lv, resets_at), mics in groups.items():
        mics = np.array(mics)
        li, at, state, snap = 0, 0, new[0], new
        for p, n in enumerate(sched):
            for r in resets_at:
                if r == p:
                    li, at, state, snap = li + 1, 0, new[0], new
            sl = slice(off[p], off[p + 1])
            if p in lv[li]:
                out, snap = refs[(b, lv[li])]
                for k, v in exp.items():
                    if v is not None:
                        v[sl, mics] = out[k][at:at + n][:, None]
                at += n
                if row["fsm"]:
                    state = out["fsm_states"][at - 1]
            elif row["fsm"]:
                exp["fsm_states"][sl, mics] = state            # the fill: the machine's unchanged state
        for m in mics:
            snaps[m] = snap        # a life's reference gives its machine at the life's end, which is where the schedule leaves it
    return exp, snaps, thr


def _filter_input(net):
    second = net.get("softmax", net.get("probs"))
    return second if second is not None else net["logits"]


# ---- test bodies that the int8 and the float bank share ----------------------------------------------------------------------------
def check_bank_equals_independent_streams(K, c, g, n_mics, chunk, fsm, what):
    """24 device pushes by schedule(chunk, 24), filter on: the bank against one stream per microphone, final machines included."""
    sched = schedule(chunk, 24)
    assert chunk == 1 or (min(sched) < chunk and max(sched) == chunk)
    x = recordings(g, n_mics, sum(sched), 100 + n_mics)
    ref, ref_snaps = reference(K, c, g, x, sched, chunk=chunk, filt=True, fsm=fsm)
    got, snaps = drive_bank(K, c, g, x, sched, chunk=chunk, filt=True, fsm=fsm)
    same_as_streams(K, got, ref, "%s x%d chunk %d" % (what, n_mics, chunk))
    assert snaps == ref_snaps
    assert any(not np.array_equal(ref[0]["logits"], r["logits"]) for r in ref[1:])   # the microphones do differ


def check_one_microphone_equals_a_stream(K, c, g, fsm, threshold, what):
    sched = schedule(3, 24)
    x = recordings(g, 1, sum(sched), 9)
    ref, ref_snaps = reference(K, c, g, x, sched, chunk=3, filt=True, fsm=fsm, alpha=0.6, threshold=threshold)
    got, snaps = drive_bank(K, c, g, x, sched, chunk=3, filt=True, fsm=fsm, alpha=0.6, threshold=threshold)
    same_as_streams(K, got, ref, what + " one microphone")
    assert snaps == ref_snaps


def check_host_device_and_alternating_pushes(K, c, g, fsm, what, after_host):
    """Host pushes, device pushes after a reset, and the two alternating after another, each against the streams; after_host(b, host):
    the caller's own assertions on the bank and its list of host push dicts."""
    chunk, pushes, M = 3, 20, 3
    sched = [chunk] * pushes
    x = recordings(g, M, chunk * pushes, 55)
    ref, ref_snaps = reference(K, c, g, x, sched, chunk=chunk, filt=True, fsm=fsm)
    b = K.bank(c, g, M, chunk, output_filter=True, fsm=fsm)
    host = host_pushes(b, x, pushes)
    same_as_streams(K, cat(K, host), ref, what + " host pushes")
    after_host(b, host)
    assert b.frames_seen() == chunk * pushes
    if fsm:
        assert [f["raw"] for f in host[-1]["fsm"]] == ref_snaps
    b.reset()
    assert b.frames_seen() == 0
    dev, _ = drive_bank(K, c, g, x, sched, chunk=chunk, filt=True, fsm=fsm, bank=b)
    same_as_streams(K, dev, ref, what + " device pushes after reset")
    b.reset()
    parts = []
    h = chunk * g.frame_step
    for i in range(pushes):
        if i % 2 == 0:
            parts.append(host_pushes(b, x, 1, first=i)[0])
        else:
            parts.append(drive_bank(K, c, g, x[:, i * h:(i + 1) * h], [chunk], chunk=chunk, filt=True, fsm=fsm, bank=b)[0])
    same_as_streams(K, cat(K, parts), ref, what + " alternating pushes")
    b.close()


def check_reset_mic_reset_and_frames_seen(K, c, g):
    """After 10 pushes microphone 1 of 3 is reset: from then on it equals a new stream fed the rest of its samples, microphones 0 and
    2 equal their uninterrupted streams; then reset: the whole bank equals new streams again."""
    n, cut, on = 30, 10, dict(chunk=1, filt=True, fsm=True)
    x = recordings(g, 3, n, 41)
    full, full_snaps = reference(K, c, g, x, [1] * n, **on)
    rest, rest_snaps = reference(K, c, g, x[1:2, cut * g.frame_step:], [1] * (n - cut), **on)
    b = K.bank(c, g, 3, 1, fsm=True)
    head, _ = drive_bank(K, c, g, x[:, :cut * g.frame_step], [1] * cut, bank=b, **on)
    same_as_streams(K, head, [{k: v[:cut] for k, v in w.items()} for w in full], "before reset_mic")
    b.reset_mic(1)
    assert b.frames_seen() == cut
    rear, snaps = drive_bank(K, c, g, x[:, cut * g.frame_step:], [1] * (n - cut), bank=b, **on)
    assert b.frames_seen() == n
    same_as_streams(K, rear, [{k: v[cut:] for k, v in w.items()} for w in full], "after reset_mic", mics=(0, 2))
    for k in K.keys(True, True):
        same(rear[k][:, 1], rest[0][k], "the reset microphone " + k)
    assert [snaps[0], snaps[2]] == [full_snaps[0], full_snaps[2]] and snaps[1] == rest_snaps[0]
    b.reset()
    assert b.frames_seen() == 0
    again, again_snaps = drive_bank(K, c, g, x, [1] * n, bank=b, **on)
    same_as_streams(K, again, full, "after reset")
    assert again_snaps == full_snaps
    b.close()

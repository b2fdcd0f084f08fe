"""Continuous keyword spotting on a sample stream -- Python handle on ``edison_stream_*`` (include/edison_hip.h).

Counterpart of the firmware's continuous mode (firmware/src/app.c:288-371, 635-719) and of the host mirror
``kws_on_mcu.hostMicContinuous`` (kws_on_mcu.py:520-600): every new frame yields a fresh inference on the newest
31 MFCC rows. Note the reference's host mirror *prepends* new rows (kws_on_mcu.py:558-567) while the firmware
*appends* them (app.c:706-719); this stream follows the firmware (oldest row first), which is also the order the
network was trained on.

``q15=True`` computes the features with the firmware's own Q15 arithmetic (MFCC variant C) instead of the host
float model; ``output_filter=True`` adds the firmware's post-processing of the network output (moving average,
maximum, threshold: app.c:332-356). ``Fsm`` is the firmware's wake-word / location / value state machine
(app.c:727-928) without the LEDs.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import FRAME_LEN, NET_OUT, EdisonError
from .context import KEYWORDS, default_context


class _Handle:
    """What the stream and bank classes share: the life of the handle ``_h`` on the C functions ``<_C>*`` and the state machine's view."""
    _C = None    # "edison_stream_", "edison_stream_geom_", "edison_stream_bank_", "edison_stream_float_", "edison_float_bank_"
    n_mics = None    # a bank's microphones; None: one stream, whose pushes and outputs have no microphone axis

    def _c(self, name):
        return getattr(self._L, self._C + name)

    def close(self):
        if getattr(self, "_h", None):
            self._c("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.ctx._check(self._c("reset")(self._h))

    @property
    def frames_seen(self):
        return int(self._c("frames_seen")(self._h))

    def fsm_snapshot(self):
        """The state machine as the last edison_stream*_fsm call saw it: dict(state, hot_timeout_ms, last_command, commands)."""
        return _fsm_dict(self._fsm)

    def _options(self, o, chunk_frames, output_filter, alpha, threshold, fsm):
        """The options every stream has, into its struct ``o`` (a bank's ``o.stream``) and onto the handle."""
        o.chunk_frames = int(chunk_frames)
        o.filter = 1 if (output_filter or fsm) else 0
        o.fsm = 1 if fsm else 0         # the firmware's state machine as the last GPU stage of every push (edison_stream*_fsm)
        o.filter_alpha, o.true_threshold = float(alpha), float(threshold)
        self.chunk, self.output_filter, self.fsm = int(chunk_frames), bool(output_filter or fsm), bool(fsm)

    def _push_t(self, samples, logits, second, argmax, filtered, likely, spotted, n_frames, fsm_states=None, present=None):
        """push_t behind every signature: `second` is the softmax or the probabilities; `fsm_states` and `present` are the banks'."""
        n, m = self.chunk if n_frames is None else int(n_frames), self.n_mics
        if m is None:
            if samples.numel() != n * self.hop:
                raise ValueError("push needs exactly n_frames*hop = %d samples" % (n * self.hop))
        elif samples.numel() != m * n * self.hop or not samples.is_contiguous():
            raise ValueError("push needs contiguous [n_mics, n_frames*hop] = [%d, %d] samples" % (m, n * self.hop))
        q = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        if present is not None:
            if str(present.dtype) not in ("torch.uint8", "torch.bool") or tuple(present.shape) != (m,) or not present.is_contiguous() \
                    or present.device != samples.device:
                raise self._mask_error("a contiguous uint8 [n_mics] = [%d] tensor on the samples' device" % m)
            self.ctx._check(getattr(self._L, self._P + "push_present_n_dev")(self._h, q(samples), q(present), n, q(logits), q(second), q(argmax)))
        elif n_frames is None:
            self.ctx._check(self._c("push_dev")(self._h, q(samples), q(logits), q(second), q(argmax)))
        else:
            self.ctx._check(self._c("push_n_dev")(self._h, q(samples), n, q(logits), q(second), q(argmax)))
        if filtered is not None or likely is not None or spotted is not None:
            self.ctx._check(self._c("filtered_dev")(self._h, q(filtered), q(likely), q(spotted)))
        if fsm_states is not None:
            self.ctx._check(self._c("fsm_dev")(self._h, None, q(fsm_states)))

    def _filter_tail(self, out, lead, machine):
        """The filter's and the state machine's outputs of a host push, behind the network's: ``lead`` is their leading shape, (chunk,) or
        (chunk, n_mics), ``machine`` the handle's edison_fsm or its array of them."""
        if self.output_filter:
            fl, li, sp = np.zeros(lead + (self.n_out,), np.float32), np.zeros(lead, np.int32), np.zeros(lead, np.int32)
            self.ctx._check(self._c("filtered")(self._h, fl.ctypes.data, li.ctypes.data, sp.ctypes.data))
            out.update(filtered=fl, likely=li, spotted=sp)
        if self.fsm:
            st = np.zeros(lead, np.int32)
            self.ctx._check(self._c("fsm")(self._h, ctypes.byref(machine), st.ctypes.data))
            out.update(fsm_states=st, fsm=self.fsm_snapshot())
        return out


def _float_options(o, geometry, q15, clip_min, clip_max):
    """The float pair's own options into ``o``; returns the geometry (None: what ``Context.kws_float`` uses by default)."""
    from . import config as cfg
    from .kws.geometry import KwsGeometry
    o.q15 = 1 if q15 else 0
    o.clip_lo = float(cfg.net_input_clip_min if clip_min is None else clip_min)
    o.clip_hi = float(cfg.net_input_clip_max if clip_max is None else clip_max)
    return KwsGeometry.from_config(net_input_scale=cfg.net_input_scale) if geometry is None else geometry


def _fsm_dict(f):
    cmd = None if f.last_loc < 0 else (KEYWORDS[f.last_loc], KEYWORDS[f.last_val])
    return dict(state=Fsm.STATES[f.state], hot_timeout_ms=int(f.hot_timeout_ms), last_command=cmd, commands=int(f.commands),
                raw=(f.state, f.hot_timeout_ms, f.wake_idx, f.loc_idx, f.val_idx, f.last_loc, f.last_val, f.commands))


class _Bank(_Handle):
    """What StreamBank and FloatBank share: the per-microphone calls, and the mask of a push that leaves microphones out (``_P`` names
    those C functions, ``_WHO`` is the bank's message prefix)."""
    _P = _WHO = None

    def frames_seen(self):
        """Frames pushed per microphone since the bank was made or reset."""
        n = ctypes.c_int64()
        self.ctx._check(self._c("frames_seen")(self._h, ctypes.byref(n)))
        return int(n.value)

    def frames_seen_mics(self):
        """int64 [n_mics]: the frames each microphone was present for since the bank was made or reset (``reset_mic`` keeps the count).
        Waits for pushes in flight."""
        out = np.zeros(self.n_mics, np.int64)
        self.ctx._check(getattr(self._L, self._P + "frames_seen_mics")(self._h, out.ctypes.data))
        return out

    def reset_mic(self, m):
        """Microphone m alone back to a new stream's state; the others do not notice."""
        self.ctx._check(self._c("reset_mic")(self._h, int(m)))

    def _mask_error(self, what):
        return EdisonError(_lib.E_ARGUMENT, "%s: present must be %s" % (self._WHO, what))

    def _host_present(self, present):
        """None, or the mask of a host push as contiguous uint8 [n_mics] (bool counts as uint8)."""
        if present is None:
            return None
        p = np.asarray(present)
        if p.dtype == np.bool_:
            p = p.view(np.uint8)
        if p.dtype != np.uint8 or p.shape != (self.n_mics,):
            raise self._mask_error("uint8 [n_mics] = [%d], not %s %s" % (self.n_mics, p.dtype, list(p.shape)))
        return np.ascontiguousarray(p)

    def fsm_snapshot(self):
        """The state machines as the last host push saw them: one stream's ``fsm_snapshot`` dict per microphone."""
        return [_fsm_dict(f) for f in self._fsms]


class _SlidingStream(_Handle):
    """What GeomStream and FloatStream share in front of a host push: the sample check."""

    def _host_samples(self, samples):
        x = np.ascontiguousarray(samples, dtype=np.int16).ravel()
        if x.shape[0] != self.chunk * self.hop:
            raise ValueError("push needs exactly chunk_frames*hop = %d samples" % (self.chunk * self.hop))
        return x


class Stream(_Handle):
    _C = "edison_stream_"

    def __init__(self, ctx=None, hop=FRAME_LEN, chunk_frames=1, q15=False, output_filter=False, alpha=0.9,
                 threshold=0.5, graph=None, fsm=False):
        self.ctx = ctx or default_context()
        self._L = _lib.lib()
        o = _lib.StreamOpts()
        self._L.edison_stream_default_opts(ctypes.byref(o))
        self._options(o, chunk_frames, output_filter, alpha, threshold, fsm)
        o.hop = self.hop = int(hop)
        o.mfcc_variant = _lib.MFCC_C if q15 else _lib.MFCC_B
        if graph is not None:    # None: the library's default (direct launches unless EDISON_STREAM_GRAPH=1)
            o.launch_mode = 1 if graph else 0
        h = ctypes.c_void_p()
        self.ctx._check(self._L.edison_stream_create_ex(self.ctx._h, ctypes.byref(o), ctypes.byref(h)))
        self._h = h
        self._fsm_states = np.zeros(self.chunk, np.int32)
        self._fsm = _lib.Fsm()
        self._bufs = None

    def push(self, samples):
        """samples: chunk_frames*hop new int16 samples (host). Returns dict(logits, softmax, argmax, keywords) plus,
        with the output filter, filtered [chunk,10] fp32, likely [chunk], spotted [chunk] (-1 = below threshold)."""
        x = samples if (type(samples) is np.ndarray and samples.dtype == np.int16 and samples.ndim == 1 and samples.flags.c_contiguous) \
            else np.ascontiguousarray(samples, dtype=np.int16).ravel()
        if x.shape[0] != self.chunk * self.hop:
            raise ValueError("push needs exactly chunk_frames*hop = %d samples" % (self.chunk * self.hop))
        # the microphone path calls this once per frame: the result buffers and their addresses are made once, the call
        # writes into them, the caller gets copies (10 + 10 + 4 bytes per frame)
        b = self._bufs
        if b is None:
            b = self._bufs = self._make_bufs()
        r = self._push(self._h, x.ctypes.data, b[3], b[4], b[5])
        if r != _lib.OK:
            self.ctx._check(r)
        am = b[2].copy()
        out = dict(logits=b[0].copy(), softmax=b[1].copy(), argmax=am, keywords=[KEYWORDS[i] for i in am])
        if self.output_filter:
            self.ctx._check(self._L.edison_stream_filtered(self._h, b[9], b[10], b[11]))
            out.update(filtered=b[6].copy(), likely=b[7].copy(), spotted=b[8].copy())
        if self.fsm:
            self.ctx._check(self._L.edison_stream_fsm(self._h, ctypes.byref(self._fsm), self._fsm_states.ctypes.data))
            out.update(fsm_states=self._fsm_states.copy(), fsm=self.fsm_snapshot())
        return out

    def _make_bufs(self):
        c = self.chunk
        lo, so, am = np.zeros((c, NET_OUT), np.int8), np.zeros((c, NET_OUT), np.int8), np.zeros(c, np.int32)
        fl, li, sp = np.zeros((c, NET_OUT), np.float32), np.zeros(c, np.int32), np.zeros(c, np.int32)
        self._push = self._L.edison_stream_push
        return (lo, so, am, lo.ctypes.data, so.ctypes.data, am.ctypes.data, fl, li, sp, fl.ctypes.data, li.ctypes.data, sp.ctypes.data)

    def push_t(self, samples, logits=None, softmax=None, argmax=None, filtered=None, likely=None, spotted=None, n_frames=None):
        """Device tensors (torch, int16 / int8 / int32 / fp32 on the context's GPU); asynchronous on the context's stream.
        n_frames < chunk_frames: a ragged last push (edison_stream_push_n_dev: n_frames * hop samples); every output -- logits, softmax,
        argmax, filtered, likely, spotted -- is [n_frames][..]: the stream copies the entries of THIS push only."""
        self._push_t(samples, logits, softmax, argmax, filtered, likely, spotted, n_frames)


class GeomStream(_SlidingStream):
    """Continuous keyword spotting for a graph trained at ANY MFCC geometry -- Python handle on ``edison_stream_geom_*``: the continuous
    counterpart of ``Context.kws_geom``. The hop is ``geometry.frame_step``; the window is ``geometry.frame_count`` rows of
    ``num_mfcc`` features, oldest first (the firmware's order, as ``Stream``). The features are the float64 host flow's at every
    geometry, so for frames that fill a whole window the outputs equal ``Context.kws_geom`` on the same samples.

    ``output_filter=True`` adds the firmware's post-processing over the graph's n_out outputs (the softmax, or the last layer's output
    for a graph without Softmax); ``fsm=True`` puts edisonFSM behind it (graphs with 10 outputs only)."""

    _C = "edison_stream_geom_"

    def __init__(self, ctx, geometry, chunk_frames=1, output_filter=False, alpha=0.9, threshold=0.5, fsm=False):
        self.ctx = ctx or default_context()
        self._L = _lib.lib()
        o = _lib.StreamGeomOpts()
        self._L.edison_stream_geom_default_opts(ctypes.byref(o))
        self._options(o, chunk_frames, output_filter, alpha, threshold, fsm)
        g = geometry.to_ctypes()
        h = ctypes.c_void_p()
        self.ctx._check(self._L.edison_stream_geom_create(self.ctx._h, ctypes.byref(g), ctypes.byref(o), ctypes.byref(h)))
        self._h = h
        info = self.ctx.net_info()
        self.geometry, self.hop = geometry, int(geometry.frame_step)
        self.n_out, self.has_softmax = int(info["n_out"]), bool(info["has_softmax"])
        self._fsm = _lib.Fsm()

    def push(self, samples):
        """samples: chunk_frames * hop new int16 samples (host). Returns dict(logits, softmax, argmax) [chunk][n_out] / [chunk] (softmax
        None for a graph without Softmax), ``keywords`` for a graph with 10 outputs, and with the filter filtered [chunk][n_out] fp32,
        likely, spotted (-1 = below the threshold); with the state machine fsm_states and fsm (Stream.fsm_snapshot's dict)."""
        x = self._host_samples(samples)
        c, no = self.chunk, self.n_out
        lo, am = np.zeros((c, no), np.int8), np.zeros(c, np.int32)
        so = np.zeros((c, no), np.int8) if self.has_softmax else None
        ptr = lambda a: None if a is None else a.ctypes.data
        self.ctx._check(self._L.edison_stream_geom_push(self._h, x.ctypes.data, lo.ctypes.data, ptr(so), am.ctypes.data))
        out = dict(logits=lo, softmax=so, argmax=am)
        if no == NET_OUT:
            out["keywords"] = [KEYWORDS[i] for i in am]
        return self._filter_tail(out, (c,), self._fsm)

    def push_t(self, samples, logits=None, softmax=None, argmax=None, filtered=None, likely=None, spotted=None, n_frames=None):
        """Device tensors (torch, int16 / int8 / int32 / fp32 on the context's GPU); asynchronous on the context's stream. n_frames <
        chunk_frames: a ragged last push of n_frames * hop samples; every output is [n_frames][..]."""
        self._push_t(samples, logits, softmax, argmax, filtered, likely, spotted, n_frames)


class StreamBank(_Bank):
    """Many microphones through one graph -- Python handle on ``edison_stream_bank_*``: ``n_mics`` continuous streams at one geometry
    on the loaded graph, advancing in lockstep. Microphone m behaves exactly as a ``GeomStream`` of its own fed microphone m's samples;
    a push costs a number of launches that does not depend on ``n_mics``. Outputs are time-major, [frames of the push][n_mics][..].

    A push may leave microphones out (``present``, uint8 [n_mics], nonzero = present): an absent microphone's stream stays untouched,
    as if the push had not happened for it; its samples are ignored and its rows of the push hold a fill (zeros, -1 in argmax, likely
    and spotted, the unchanged state in fsm_states). ``frames_seen_mics`` counts each microphone's own frames."""

    _C, _P, _WHO = "edison_stream_bank_", "edison_bank_", "stream_bank"

    def __init__(self, ctx, geometry, n_mics, chunk_frames=1, output_filter=False, alpha=0.9, threshold=0.5, fsm=False):
        self.ctx = ctx or default_context()
        self._L = _lib.lib()
        o = _lib.StreamBankOpts()
        self._L.edison_stream_bank_default_opts(ctypes.byref(o))
        o.n_mics = int(n_mics)
        self._options(o.stream, chunk_frames, output_filter, alpha, threshold, fsm)
        g = geometry.to_ctypes()
        h = ctypes.c_void_p()
        self.ctx._check(self._L.edison_stream_bank_create(self.ctx._h, ctypes.byref(g), ctypes.byref(o), ctypes.byref(h)))
        self._h = h
        info = self.ctx.net_info()
        self.geometry, self.n_mics, self.hop = geometry, int(n_mics), int(geometry.frame_step)
        self.n_out, self.has_softmax = int(info["n_out"]), bool(info["has_softmax"])
        self._fsms = (_lib.Fsm * self.n_mics)()

    def push(self, samples, present=None):
        """samples: [n_mics, chunk_frames * hop] new int16 samples (host). Returns ``GeomStream.push``'s dict with the microphone axis
        added: logits / softmax [chunk][n_mics][n_out] (softmax None for a graph without Softmax), argmax [chunk][n_mics], ``keywords``
        [chunk][n_mics] for a graph with 10 outputs; with the filter filtered [chunk][n_mics][n_out] fp32, likely, spotted
        [chunk][n_mics]; with the state machine fsm_states [chunk][n_mics] and fsm, a list of n_mics snapshots. ``present``: uint8
        [n_mics] (host), nonzero = this microphone's samples count; None: everyone. It comes back as ``present``; an absent
        microphone's rows hold the fill and its keywords None."""
        x = np.ascontiguousarray(samples, dtype=np.int16)
        if x.shape != (self.n_mics, self.chunk * self.hop):
            raise ValueError("push needs [n_mics, chunk_frames*hop] = [%d, %d] samples" % (self.n_mics, self.chunk * self.hop))
        p = self._host_present(present)
        c, m, no = self.chunk, self.n_mics, self.n_out
        lo, am = np.zeros((c, m, no), np.int8), np.zeros((c, m), np.int32)
        so = np.zeros((c, m, no), np.int8) if self.has_softmax else None
        ptr = lambda a: None if a is None else a.ctypes.data
        if p is None:
            self.ctx._check(self._c("push")(self._h, x.ctypes.data, lo.ctypes.data, ptr(so), am.ctypes.data))
        else:
            self.ctx._check(self._L.edison_bank_push_present(self._h, x.ctypes.data, p.ctypes.data, lo.ctypes.data, ptr(so), am.ctypes.data))
        out = dict(logits=lo, softmax=so, argmax=am, present=p)
        if no == NET_OUT:
            out["keywords"] = [[KEYWORDS[i] if i >= 0 else None for i in row] for row in am]
        return self._filter_tail(out, (c, m), self._fsms)

    def push_t(self, samples, logits=None, softmax=None, argmax=None, filtered=None, likely=None, spotted=None, fsm_states=None, n_frames=None,
               present=None):
        """Device tensors (torch, int16 / int8 / int32 / fp32 on the context's GPU); asynchronous on the context's stream. samples
        [n_mics][n * hop]; every output [n][n_mics][..] with n = chunk_frames, or n_frames <= chunk_frames for a ragged push. ``present``:
        a device uint8 [n_mics] tensor, read on the context's stream (keep it unchanged until the push has run); None: everyone."""
        self._push_t(samples, logits, softmax, argmax, filtered, likely, spotted, n_frames, fsm_states, present)


class FloatStream(_SlidingStream):
    """Continuous keyword spotting with the float32 X-CUBE-AI network loaded on the context (``Context.fnet_load``) -- Python handle on
    ``edison_stream_float_*``: the continuous counterpart of ``Context.kws_float``, and the loop the reference's board runs for its
    default network type (app.c:288-371, 630-719). The hop is ``geometry.frame_step`` (``geometry=None``: what ``Context.kws_float``
    uses by default); the window is ``geometry.frame_count`` float rows, oldest first. ``q15=False`` is the host flow (float64 MFCC ->
    float32 x net_input_scale -> clip to [clip_min, clip_max], default audio/config.py's); ``q15=True`` the firmware's variant C ->
    (float), shipped framing only. For frames that fill a whole window the outputs equal ``Context.kws_float`` on the same samples.

    ``output_filter=True`` adds the firmware's moving average over the probabilities (alpha 0.5: the Cube build's, app.c:35-36), first
    maximum and threshold; ``fsm=True`` puts edisonFSM behind it (networks with 10 outputs only)."""

    _C = "edison_stream_float_"

    def __init__(self, ctx, geometry=None, q15=False, chunk_frames=1, output_filter=False, alpha=0.5, threshold=0.5, fsm=False,
                 clip_min=None, clip_max=None):
        self.ctx = ctx or default_context()
        self._L = _lib.lib()
        o = _lib.StreamFloatOpts()
        self._L.edison_stream_float_default_opts(ctypes.byref(o))
        self._options(o, chunk_frames, output_filter, alpha, threshold, fsm)
        geometry = _float_options(o, geometry, q15, clip_min, clip_max)
        g = geometry.to_ctypes()
        h = ctypes.c_void_p()
        self.ctx._check(self._L.edison_stream_float_create(self.ctx._h, ctypes.byref(g), ctypes.byref(o), ctypes.byref(h)))
        self._h = h
        self.geometry, self.hop = geometry, int(geometry.frame_step)
        self.n_out = int(self.ctx.fnet_info()["n_out"])
        self.keywords = getattr(self.ctx, "fnet_keywords", None)   # the names of the loaded .ednf (Context.fnet_load)
        self._fsm = _lib.Fsm()

    def push(self, samples):
        """samples: chunk_frames * hop new int16 samples (host). Returns dict(logits, probs) float32 [chunk][n_out], argmax [chunk],
        ``keywords`` (the names of the network's .ednf, ``self.keywords``; KEYWORDS for a 10-output network without names), and with
        the filter filtered [chunk][n_out] fp32, likely, spotted (-1 = below the threshold); with the state machine fsm_states and fsm."""
        x = self._host_samples(samples)
        c, no = self.chunk, self.n_out
        lo, pr, am = np.zeros((c, no), np.float32), np.zeros((c, no), np.float32), np.zeros(c, np.int32)
        self.ctx._check(self._L.edison_stream_float_push(self._h, x.ctypes.data, lo.ctypes.data, pr.ctypes.data, am.ctypes.data))
        out = dict(logits=lo, probs=pr, argmax=am)
        names = self.keywords or (list(KEYWORDS) if no == NET_OUT else None)
        if names is not None:
            out["keywords"] = [names[i] if i < len(names) else str(i) for i in am]
        return self._filter_tail(out, (c,), self._fsm)

    def push_t(self, samples, logits=None, probs=None, argmax=None, filtered=None, likely=None, spotted=None, n_frames=None):
        """Device tensors (torch, int16 / fp32 / int32 on the context's GPU); asynchronous on the context's stream. n_frames <
        chunk_frames: a ragged last push of n_frames * hop samples; every output is [n_frames][..]."""
        self._push_t(samples, logits, probs, argmax, filtered, likely, spotted, n_frames)


class FloatBank(_Bank):
    """Many microphones through one float32 X-CUBE-AI network -- Python handle on ``edison_float_bank_*``: ``n_mics`` continuous streams
    at one geometry on the float network loaded on the context (``Context.fnet_load``), advancing in lockstep. Microphone m behaves
    exactly as a ``FloatStream`` of its own (same geometry, flow and options) fed microphone m's samples; a push costs a number of
    launches that depends neither on ``n_mics`` nor on its frames. Outputs are time-major, [frames of the push][n_mics][..].

    A push may leave microphones out (``present``), as ``StreamBank``'s: the absent microphone's stream stays untouched."""

    _C, _P, _WHO = "edison_float_bank_", "edison_fbank_", "float_bank"

    def __init__(self, ctx, n_mics, geometry=None, q15=False, chunk_frames=1, output_filter=False, alpha=0.5, threshold=0.5, fsm=False,
                 clip_min=None, clip_max=None):
        self.ctx = ctx or default_context()
        self._L = _lib.lib()
        o = _lib.FloatBankOpts()
        self._L.edison_float_bank_default_opts(ctypes.byref(o))
        o.n_mics = int(n_mics)
        self._options(o.stream, chunk_frames, output_filter, alpha, threshold, fsm)
        geometry = _float_options(o.stream, geometry, q15, clip_min, clip_max)
        g = geometry.to_ctypes()
        h = ctypes.c_void_p()
        self.ctx._check(self._L.edison_float_bank_create(self.ctx._h, ctypes.byref(g), ctypes.byref(o), ctypes.byref(h)))
        self._h = h
        self.geometry, self.n_mics, self.hop = geometry, int(n_mics), int(geometry.frame_step)
        self.n_out = int(self.ctx.fnet_info()["n_out"])
        self.keywords = getattr(self.ctx, "fnet_keywords", None)   # the names of the loaded .ednf (Context.fnet_load)
        self._fsms = (_lib.Fsm * self.n_mics)()

    def push(self, samples, present=None):
        """samples: [n_mics, chunk_frames * hop] new int16 samples (host). Returns ``FloatStream.push``'s dict with the microphone axis
        added: logits / probs float32 [chunk][n_mics][n_out], argmax [chunk][n_mics], ``keywords`` [chunk][n_mics] (the names of the
        network's .ednf; KEYWORDS for a 10-output network without names); with the filter filtered [chunk][n_mics][n_out] fp32, likely,
        spotted [chunk][n_mics]; with the state machine fsm_states [chunk][n_mics] and fsm, a list of n_mics snapshots. ``present``:
        uint8 [n_mics] (host), nonzero = this microphone's samples count; None: everyone. It comes back as ``present``; an absent
        microphone's rows hold the fill and its keywords None."""
        x = np.ascontiguousarray(samples, dtype=np.int16)
        if x.shape != (self.n_mics, self.chunk * self.hop):
            raise ValueError("push needs [n_mics, chunk_frames*hop] = [%d, %d] samples" % (self.n_mics, self.chunk * self.hop))
        p = self._host_present(present)
        c, m, no = self.chunk, self.n_mics, self.n_out
        lo, pr, am = np.zeros((c, m, no), np.float32), np.zeros((c, m, no), np.float32), np.zeros((c, m), np.int32)
        if p is None:
            self.ctx._check(self._c("push")(self._h, x.ctypes.data, lo.ctypes.data, pr.ctypes.data, am.ctypes.data))
        else:
            self.ctx._check(self._L.edison_fbank_push_present(self._h, x.ctypes.data, p.ctypes.data, lo.ctypes.data, pr.ctypes.data, am.ctypes.data))
        out = dict(logits=lo, probs=pr, argmax=am, present=p)
        names = self.keywords or (list(KEYWORDS) if no == NET_OUT else None)
        if names is not None:
            out["keywords"] = [[None if i < 0 else names[i] if i < len(names) else str(i) for i in row] for row in am]
        return self._filter_tail(out, (c, m), self._fsms)

    def push_t(self, samples, logits=None, probs=None, argmax=None, filtered=None, likely=None, spotted=None, fsm_states=None, n_frames=None,
               present=None):
        """Device tensors (torch, int16 / fp32 / int32 on the context's GPU); asynchronous on the context's stream. samples
        [n_mics][n * hop]; every output [n][n_mics][..] with n = chunk_frames, or n_frames <= chunk_frames for a ragged push. ``present``:
        a device uint8 [n_mics] tensor, read on the context's stream (keep it unchanged until the push has run); None: everyone."""
        self._push_t(samples, logits, probs, argmax, filtered, likely, spotted, n_frames, fsm_states, present)


class Fsm:
    """edisonFSM (app.c:727-928): RESET -> IDLE -> HOT (wake word) -> LOC (location) -> SET (value) -> IDLE."""
    STATES = ("RESET", "IDLE", "HOT", "LOC", "SET")

    def __init__(self, threshold=0.5):
        self._L = _lib.lib()
        self._f = _lib.Fsm()
        self._L.edison_fsm_init(ctypes.byref(self._f))
        self.threshold = float(threshold)

    def step(self, pred_max, pred_idx, dt_us):
        r = self._L.edison_fsm_step(ctypes.byref(self._f), float(pred_max), int(pred_idx), int(dt_us), self.threshold)
        if r < 0:
            raise EdisonError(r, "edison_fsm_step")
        return self.STATES[r]

    @property
    def state(self):
        return self.STATES[self._f.state]

    @property
    def last_command(self):
        """(location, value) keyword strings of the last executed command, or None."""
        if self._f.last_loc < 0:
            return None
        return KEYWORDS[self._f.last_loc], KEYWORDS[self._f.last_val]

    @property
    def commands(self):
        return int(self._f.commands)

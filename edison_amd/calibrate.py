"""Calibrating the loaded float32 network on the GPU (``edison_fcal_*``, include/edison_hip.h) and the flow
``Context.quantize`` builds on it: audio -> the float flow's features, chunk by chunk -> the calibrator -> quantize.quantize. The
statistic lives in device memory; ``Calibrator.result()`` brings back a few hundred integers.
"""
import ctypes

import numpy as np

from . import _lib, quantize as qz


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _t_ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Calibrator:
    """edison_fcal on `ctx`, bound to the float network loaded now; loading another one invalidates it (EdisonError)."""

    def __init__(self, ctx):
        self._ctx, self._L = ctx, ctx._L
        h = ctypes.c_void_p()
        ctx._check(self._L.edison_fcal_create(ctx._h, ctypes.byref(h)))
        self._h = h
        info = self.info()
        self.n_stats, self.in_n, self.batch = info["n_stats"], info["in_n"], info["batch"]

    def close(self):
        if getattr(self, "_h", None):
            self._L.edison_fcal_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        """dict of edison_fcal_info_t: n_stats, in_n, batch, lds_bytes."""
        info = _lib.FcalInfo()
        self._ctx._check(self._L.edison_fcal_info(self._h, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in _lib.FcalInfo._fields_}

    def reset(self):
        self._ctx._check(self._L.edison_fcal_reset(self._h))

    def add(self, x):
        """Host inputs [n][in_n] float32, as Context.fnet takes them."""
        f = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, self.in_n)
        self._ctx._check(self._L.edison_fcal_add(self._h, _np_ptr(f), f.shape[0]))

    def add_t(self, x, n=None):
        """edison_fcal_add_dev on a torch device tensor (float32 [n][in_n], contiguous), enqueued on the context's stream."""
        n = int(x.shape[0] if n is None else n)
        self._ctx._check(self._L.edison_fcal_add_dev(self._h, _t_ptr(x), n))

    def result(self):
        """Synchronise and fetch dict(absmax uint32 [n_stats], hist uint64 [n_stats][256], count uint64 [n_stats]): what
        quantize.quantize takes. The calibrator goes on counting afterwards."""
        absmax = np.zeros(self.n_stats, np.uint32)
        hist = np.zeros((self.n_stats, 256), np.uint64)
        count = np.zeros(self.n_stats, np.uint64)
        self._ctx._check(self._L.edison_fcal_result(self._h, _np_ptr(absmax), _np_ptr(hist), _np_ptr(count)))
        return dict(absmax=absmax, hist=hist, count=count)


def quantize_audio(ctx, audio, geometry=None, q15=False, chunk=16384, method="max_min", saturate=0.0, n_utt=None, utt_stride=None, clip_min=None,
                   clip_max=None, return_features=False):
    """Context.quantize: calibrate the loaded float network on a set of utterances and quantise it. Per chunk the float flow's device
    form (kws_float_t) writes its features into one device buffer and the calibrator reads them behind it on the context's stream.
    audio: int16, numpy (uploaded chunk by chunk) or a torch device tensor; utterances as in kws_float. Returns (ednn_blob, report):
    quantize.quantize's, with float_argmax (the float network's class per utterance) and, with return_features, features (float32
    [n][in_n], the calibrated network inputs) added."""
    import torch
    from . import config as cfg
    from .kws.geometry import KwsGeometry
    if ctx._fnet_blob is None:
        raise ValueError("no float network loaded (fnet_load)")
    ctx._fnet_refresh()                  # a trainer may have stepped the device weights past the blob
    g = geometry if geometry is not None else KwsGeometry.from_config(net_input_scale=cfg.net_input_scale)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    on_device = isinstance(audio, torch.Tensor)
    if not on_device:
        audio = np.ascontiguousarray(audio, dtype=np.int16)
    stride = utt_stride
    if stride is None and audio.ndim == 2:
        stride = int(audio.shape[1])
    stride = int(g.n_samples if stride is None else stride)
    flat = audio.reshape(-1)
    used = (g.frame_count - 1) * g.frame_step + g.frame_len
    if n_utt is None:
        n_utt = 0 if flat.shape[0] < used else 1 + (flat.shape[0] - used) // max(stride, 1)
    n = int(n_utt)
    if n and (n - 1) * stride + used > flat.shape[0]:
        raise ValueError("audio too short for %d utterances" % n)
    dev = torch.device("cuda", ctx.device)
    in_n = g.n_features
    with Calibrator(ctx) as cal:
        m_max = min(chunk, max(n, 1))
        keep = torch.zeros((n, in_n), dtype=torch.float32, device=dev) if return_features else None
        feat = torch.zeros((m_max, in_n), dtype=torch.float32, device=dev)
        am = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        for u0 in range(0, n, chunk):
            m = min(chunk, n - u0)
            lo, hi = u0 * stride, (u0 + m - 1) * stride + used
            if on_device:
                a_d = flat[lo:hi]
            else:
                ctx.sync()                       # the previous chunk still reads the audio buffer this upload replaces
                a_d = torch.from_numpy(flat[lo:hi]).to(dev)
            torch.cuda.current_stream(dev).synchronize()   # torch's allocations and uploads, before the context's stream reads them
            f = keep[u0:u0 + m] if return_features else feat
            ctx.kws_float_t(a_d, g, m, stride, feat=f, argmax=am[u0:u0 + m], q15=q15, clip_min=clip_min, clip_max=clip_max)
            cal.add_t(f, m)
        stats = cal.result()
    from . import cube_import
    # q15 = 1 feeds the network the firmware's int16 coefficients unscaled
    blob, report = qz.quantize(cube_import.read_blob(ctx._fnet_blob), stats, method=method, saturate=saturate, scale=1.0 if q15 else g.net_input_scale)
    report["float_argmax"] = am[:n].cpu().numpy()
    if return_features:
        report["features"] = keep.cpu().numpy()
    return blob, report

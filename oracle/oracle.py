"""oracle/oracle.py -- TEST INFRASTRUCTURE: ctypes access to the CPU checker.

Two libraries, both test-only (tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg are the only allowed callers; the product never imports this):

  * ``oracle/_build/liboracle.so``  -- this repo's plain-C restatement
    (mfcc_ref.c: reference audio/edison/mfcc/mfcc_utils.py:16-323;
     kws_cnn_ref.c: NNoM 0.3.0 / CMSIS-NN portable branches)           -> kind "port"
  * ``oracle/_ref/libnnom_ref.so``  -- the reference int8 CNN itself, built from
    /root/reference by oracle/Makefile (prebuilt file on the GPU box)   -> kind "reference"

The model blob reader below is deliberately independent of edison_amd/ so that a bug in
the product's loader cannot hide behind a shared parser.
"""
import ctypes
import os
import struct
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PORT_SO = os.path.join(_HERE, "_build", "liboracle.so")
REF_SO = os.path.join(_HERE, "_ref", "libnnom_ref.so")
Q15_REF_SO = os.path.join(_HERE, "_ref", "libcmsis_q15_ref.so")   # the reference's CMSIS-DSP Q15 FFT / split / sqrt routines
F32_REF_SO = os.path.join(_HERE, "_ref", "libmfcc_f32_ref.so")    # the reference's firmware/src/audio/mfcc.c (table builders)
DEFAULT_MODEL = os.path.join(os.path.dirname(_HERE), "edison_amd", "data", "kws_nnom.ednn")

VARIANT_A, VARIANT_B = 0, 1
VARIANT_TF = 3  # mfcc_utils.mfcc_tf restated from tf.signal's definitions: PARITY UNPINNED (oracle.h)
L_CONV, L_POOL, L_DENSE, L_SOFTMAX = 1, 2, 3, 4

# audio/config.py:11-32
FS, FRAME_LEN, NUM_MEL, MEL_LO, MEL_HI, MEL_SCALE, NUM_MFCC = 16000, 1024, 32, 80.0, 7600.0, 128, 13


def build(force=False):
    """Compile the restatement (always possible: gcc only) and, when the reference is mounted, the reference."""
    if force or not os.path.exists(PORT_SO) or any(
            os.path.getmtime(os.path.join(_HERE, f)) > os.path.getmtime(PORT_SO)
            for f in ("mfcc_ref.c", "mfcc_q15_ref.c", "mfcc_f32_ref.c", "kws_cnn_ref.c", "postproc_ref.c", "ref_loader.c", "oracle.h")):
        subprocess.check_call(["make", "-C", _HERE, "-B", "port"], stdout=subprocess.DEVNULL)
    if os.path.isdir("/root/reference/firmware"):
        for so, target in ((REF_SO, "ref"), (Q15_REF_SO, "q15ref"), (F32_REF_SO, "f32ref")):
            if force or not os.path.exists(so):
                subprocess.check_call(["make", "-C", _HERE, target], stdout=subprocess.DEVNULL)


def use_native_build():
    """bench.py's cpu_baseline leg only: (re)build the restatement with -march=native ON THIS MACHINE and make port()
    load that library. Must be called before the first port() of the process."""
    global PORT_SO
    assert _port is None, "use_native_build() must come before the first use of the checker"
    subprocess.check_call(["make", "-C", _HERE, "-B", "native"], stdout=subprocess.DEVNULL)
    PORT_SO = os.path.join(_HERE, "_build", "liboracle_native.so")


class _Layer(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int32), ("out_ch", ctypes.c_int32), ("kh", ctypes.c_int32), ("kw", ctypes.c_int32),
                ("sh", ctypes.c_int32), ("sw", ctypes.c_int32), ("bias_lshift", ctypes.c_int32),
                ("out_rshift", ctypes.c_int32), ("relu", ctypes.c_int32),
                ("w", ctypes.c_void_p), ("b", ctypes.c_void_p)]


_port = None
_ref = None


def port():
    global _port
    if _port is None:
        if not os.path.exists(PORT_SO):
            build()
        L = ctypes.CDLL(PORT_SO)
        L.oracle_mfcc.restype = ctypes.c_int
        L.oracle_mfcc.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                  ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                  ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_int]
        L.oracle_mel_weight_matrix.restype = None
        L.oracle_mel_weight_matrix.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                               ctypes.c_double, ctypes.c_void_p]
        L.oracle_net_input.restype = None
        L.oracle_net_input.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                       ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
        L.oracle_cnn_run.restype = ctypes.c_int
        L.oracle_cnn_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.oracle_num_threads.restype = ctypes.c_int
        L.oracle_q15_tables_new.restype = ctypes.c_void_p
        L.oracle_q15_tables_new.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                            ctypes.c_double, ctypes.c_double, ctypes.c_int]
        L.oracle_q15_tables_free.restype = None
        L.oracle_q15_tables_free.argtypes = [ctypes.c_void_p]
        L.oracle_q15_tables_get.restype = ctypes.c_int
        L.oracle_q15_tables_get.argtypes = [ctypes.c_void_p] * 8
        L.oracle_mfcc_q15.restype = ctypes.c_int
        L.oracle_mfcc_q15.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.oracle_f32_mfcc_new.restype = ctypes.c_void_p
        L.oracle_f32_mfcc_new.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float]
        L.oracle_f32_mfcc_free.restype = None
        L.oracle_f32_mfcc_free.argtypes = [ctypes.c_void_p]
        L.oracle_f32_mfcc_n_out.argtypes = [ctypes.c_void_p]
        L.oracle_f32_mfcc_tables_get.restype = ctypes.c_int
        L.oracle_f32_mfcc_tables_get.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int]
        L.oracle_f32_mfcc_window_get.restype = ctypes.c_int
        L.oracle_f32_mfcc_window_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.oracle_f32_mfcc_run.restype = ctypes.c_int
        L.oracle_f32_mfcc_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.oracle_output_filter.restype = None
        L.oracle_output_filter.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.oracle_net_input_q15.restype = None
        L.oracle_net_input_q15.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        _port = L
    return _port


def have_ref():
    return os.path.exists(REF_SO)


def ref():
    """The reference NNoM build; raises if oracle/_ref is absent (it cannot be rebuilt on the GPU box)."""
    global _ref
    if _ref is None:
        if not os.path.exists(REF_SO):
            build()
        if not os.path.exists(REF_SO):
            raise FileNotFoundError("oracle/_ref/libnnom_ref.so is absent and /root/reference is not mounted")
        L = ctypes.CDLL(REF_SO)
        L.nnom_ref_run_batch.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]
        L.nnom_ref_run_layers.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int32]
        if L.nnom_ref_init() != 0:
            raise RuntimeError("nnom_ref_init failed")
        _ref = L
    return _ref


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _open_lazy(path, names):
    """A reference-compiled library that carries unresolved symbols of paths nobody calls: opened with lazy binding through
    oracle/ref_loader.c (ctypes itself always binds NOW). names: {symbol: (restype, argtypes)} -> {symbol: callable}."""
    L = port()
    L.oracle_dl_open_lazy.restype = ctypes.c_void_p
    L.oracle_dl_open_lazy.argtypes = [ctypes.c_char_p]
    L.oracle_dl_sym.restype = ctypes.c_void_p
    L.oracle_dl_sym.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    L.oracle_dl_error.restype = ctypes.c_char_p
    if not os.path.exists(path):
        build()
    if not os.path.exists(path):
        raise FileNotFoundError("%s is absent and /root/reference is not mounted" % os.path.relpath(path, os.path.dirname(_HERE)))
    h = L.oracle_dl_open_lazy(path.encode())
    if not h:
        raise OSError("dlopen %s: %s" % (path, (L.oracle_dl_error() or b"?").decode()))
    out = {}
    for name, (restype, argtypes) in names.items():
        addr = L.oracle_dl_sym(h, name.encode())
        if not addr:
            raise OSError("%s lacks %s" % (path, name))
        out[name] = ctypes.CFUNCTYPE(restype, *argtypes)(addr)
    return out


_q15_ref = None
_f32_ref = None


def have_q15_ref():
    return os.path.exists(Q15_REF_SO) or os.path.isdir("/root/reference/firmware")


def have_f32_ref():
    return os.path.exists(F32_REF_SO) or os.path.isdir("/root/reference/firmware")


class CmsisQ15Ref:
    """The reference's own CMSIS-DSP routines of variant C, compiled with the firmware's ARM_MATH_DSP branches
    (oracle/ref_shim/cmsis_q15_ref_shim.c). Tables are the caller's (by pointer)."""

    def __init__(self):
        vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
        self._f = _open_lazy(Q15_REF_SO, {
            "q15ref_cfft": (ci, [vp, ci, vp, cl]),
            "q15ref_split_rfft": (ci, [vp, ci, vp, vp, vp, ci, cl]),
            "q15ref_sqrt_q31": (ci, [vp, vp, cl]),
        })

    def cfft(self, x, tw):
        """arm_cfft_q15(forward, no bit reversal) on [n_frames, 2 * n] int16 (re, im interleaved); returns a new array whose
        element order is the routine's (bit-reversed)."""
        b = np.ascontiguousarray(x, dtype=np.int16).copy()
        n = b.shape[-1] // 2
        tw = np.ascontiguousarray(tw, dtype=np.int16)
        assert tw.size >= 2 * (3 * n // 4)
        if self._f["q15ref_cfft"](_p(b), n, _p(tw), b.size // (2 * n)) != 0:
            raise ValueError("arm_cfft_q15: unsupported length %d" % n)
        return b

    def split_rfft(self, z, A, B, modifier=1):
        """arm_split_rfft_q15 on [n_frames, 2 * n_cplx] int16 in natural order -> [n_frames, 4 * n_cplx]."""
        z = np.ascontiguousarray(z, dtype=np.int16).copy()
        nc = z.shape[-1] // 2
        A, B = np.ascontiguousarray(A, dtype=np.int16), np.ascontiguousarray(B, dtype=np.int16)
        out = np.zeros(z.shape[:-1] + (4 * nc,), np.int16)
        self._f["q15ref_split_rfft"](_p(z), nc, _p(A), _p(B), _p(out), int(modifier), z.size // (2 * nc))
        return out

    def sqrt_q31(self, x):
        x = np.ascontiguousarray(x, dtype=np.int32)
        out = np.zeros_like(x)
        self._f["q15ref_sqrt_q31"](_p(x), _p(out), x.size)
        return out


def cmsis_q15_ref():
    global _q15_ref
    if _q15_ref is None:
        _q15_ref = CmsisQ15Ref()
    return _q15_ref


class MfccF32Ref:
    """The reference's own table builders of variant D (firmware/src/audio/mfcc.c:101-171), oracle/ref_shim/mfcc_f32_ref_shim.c."""

    def __init__(self):
        vp, ci = ctypes.c_void_p, ctypes.c_int
        cf = ctypes.c_float
        self._f = _open_lazy(F32_REF_SO, {"f32ref_dct_matrix": (ci, [ci, ci, vp]), "f32ref_mel_fbank": (ci, [ci, vp, vp, vp, ci]),
                                          "f32ref_cfft": (None, [vp, vp, ci, ci, vp, ci]), "f32ref_rfft": (None, [vp, vp, ci, vp, ci, vp, vp]),
                                          "f32ref_compute": (ci, [ci, ci, ci, ci, cf, vp, vp, ci, vp, vp, ci, ci, vp, vp]),
                                          "f32ref_max": (None, [vp, ci, vp, vp])})
        self._tables = {}

    def dct_matrix(self, input_length, coefficient_count):
        out = np.zeros((coefficient_count, input_length), np.float32)
        if self._f["f32ref_dct_matrix"](int(input_length), int(coefficient_count), _p(out)) != 0:
            raise RuntimeError("create_dct_matrix failed")
        return out

    def mel_fbank(self, frame_len_padded):
        first, last = np.zeros(26, np.int32), np.zeros(26, np.int32)
        w = np.zeros(8192, np.float32)
        n = self._f["f32ref_mel_fbank"](int(frame_len_padded), _p(first), _p(last), _p(w), w.size)
        if n < 0:
            raise RuntimeError("create_mel_fbank failed")
        return first, last, w[:n].copy()


    def arm_max(self, v):
        """CMSIS-DSP's arm_max_f32 compiled from the reference: (maximum, index of its FIRST occurrence)."""
        v = np.ascontiguousarray(v, np.float32)
        val, idx = np.zeros(1, np.float32), np.zeros(1, np.uint32)
        self._f["f32ref_max"](_p(v), int(v.size), _p(val), _p(idx))
        return float(val[0]), int(idx[0])

    # ---- the CMSIS-DSP float transform of the reference, on tables regenerated here (arm_common_tables.c is absent from the snapshot)
    def fft_tables(self, n):
        """Tables for arm_rfft_fast_f32 of n real points (n / 2 complex): (twiddle [n/2][2] f32, bit-reversal list u16, rfft twiddle f32).
        Twiddle VALUES by their formula (float64 cos / sin rounded to float32). The bit-reversal PERMUTATION is read off the
        reference's own routine: arm_cfft_f32 without bit reversal is run on the n / 2 complex exponentials and the bin each one
        lands in is where the reversal has to fetch it from. Both, and the layout of the real-transform twiddles, are then
        checked against numpy's FFT through the reference's compiled arm_cfft_f32 / arm_rfft_fast_f32 (float32 tolerance)."""
        if n in self._tables:
            return self._tables[n]
        m = n // 2
        k = np.arange(m)
        tw = np.stack([np.cos(2 * np.pi * k / m), np.sin(2 * np.pi * k / m)], axis=1).astype(np.float32)
        none = np.zeros(2, np.uint16)
        perm = np.zeros(m, np.int64)
        for q in range(m):
            z = np.exp(2j * np.pi * q * k / m)
            d = np.stack([z.real, z.imag], axis=1).astype(np.float32).copy()
            self._f["f32ref_cfft"](_p(tw), _p(none), 0, m, _p(d), 0)
            mag = d[:, 0].astype(np.float64) ** 2 + d[:, 1].astype(np.float64) ** 2
            perm[q] = int(np.argmax(mag))
            assert mag[perm[q]] > 0.99 * m * m and np.delete(mag, perm[q]).max() < 1e-3 * m * m, "the transform's output is not a permutation of the DFT"
        assert np.array_equal(np.sort(perm), k), "the transform's output is not a permutation of the DFT"
        # X[q] sits at position perm[q]. arm_bitreversal_32 applies a LIST OF SWAPS (word index = entry >> 2, two words per complex
        # value); a mixed-radix digit reversal (4 x 8 x 8 for 256 points) is not its own inverse, so the list walks the cycles:
        # swapping (q0, q1), (q1, q2), ... along q -> perm[q] leaves d[perm[q]] at q. ARM's table orders its swaps differently; pure
        # data movement, the same result.
        pairs, seen = [], np.zeros(m, bool)
        for q0 in range(m):
            q = q0
            while not seen[q]:
                seen[q] = True
                nxt = int(perm[q])
                if nxt != q0 and not seen[nxt]:
                    pairs.append((q, nxt))
                q = nxt
        rev = np.array([v for a, b in pairs for v in (8 * a, 8 * b)], np.uint16)
        rng = np.random.default_rng(5)
        z = rng.normal(size=m) + 1j * rng.normal(size=m)
        d = np.stack([z.real, z.imag], axis=1).astype(np.float32).copy()
        self._f["f32ref_cfft"](_p(tw), _p(rev), rev.size, m, _p(d), 1)
        want = np.fft.fft(z)
        assert np.abs((d[:, 0] + 1j * d[:, 1]) - want).max() < 1e-4 * np.abs(want).max(), "arm_cfft_f32 on the regenerated tables is not the DFT"
        # the real-transform stage: CMSIS stores (sin, cos) of 2 pi i / n -- both layouts are tried, the DFT decides
        x = rng.normal(size=n).astype(np.float32)
        wantr = np.fft.rfft(x.astype(np.float64))
        rt = None
        for cand in (np.stack([np.sin(2 * np.pi * k / n), np.cos(2 * np.pi * k / n)], axis=1), np.stack([np.cos(2 * np.pi * k / n), np.sin(2 * np.pi * k / n)], axis=1)):
            cand = cand.astype(np.float32)
            xin, out = x.copy(), np.zeros(n, np.float32)
            self._f["f32ref_rfft"](_p(tw), _p(rev), rev.size, _p(cand), n, _p(xin), _p(out))
            got = out[0::2].astype(np.float64) + 1j * out[1::2].astype(np.float64)   # [X0.re + i X(n/2).re, X1, X2, ...]
            ok = abs(got[0].real - wantr[0].real) < 1e-3 and abs(got[0].imag - wantr[m].real) < 1e-3 and np.abs(got[1:] - wantr[1:m]).max() < 1e-4 * np.abs(wantr).max()
            if ok:
                rt = cand
                break
        assert rt is not None, "arm_rfft_fast_f32 on the regenerated tables is not the real DFT"
        self._tables[n] = (tw, rev, rt)
        return self._tables[n]

    def compute(self, x, n_frames=None, frame_step=None, num_mfcc_features=13, feature_offset=1, frame_len=512, mfcc_dec_bits=8, preempha=0.97):
        """The reference's own mfcc_compute (mfcc.c:174-255) with the CMSIS transform compiled from the reference under it:
        -> (int8 [n][num_mfcc_features - feature_offset], float32 log-mel [n][26])."""
        x = np.ascontiguousarray(x, dtype=np.int16).ravel()
        step = frame_len if frame_step is None else frame_step
        if n_frames is None:
            n_frames = 1 + (x.shape[0] - frame_len) // step if x.shape[0] >= frame_len else 0
        n = max(int(n_frames), 0)
        padded = 1 << int(np.ceil(np.log2(frame_len)))
        tw, rev, rt = self.fft_tables(padded)
        out = np.zeros((n, num_mfcc_features - feature_offset), np.int8)
        lm = np.zeros((n, 26), np.float32)
        if n:
            assert (n - 1) * step + frame_len <= x.shape[0]
            r = self._f["f32ref_compute"](num_mfcc_features, feature_offset, frame_len, mfcc_dec_bits, float(preempha), _p(tw), _p(rev), rev.size, _p(rt),
                                          _p(x), n, step, _p(out), _p(lm))
            if r != 0:
                raise RuntimeError("f32ref_compute failed")
        return out, lm


def mfcc_f32_ref():
    global _f32_ref
    if _f32_ref is None:
        _f32_ref = MfccF32Ref()
    return _f32_ref


# ------------------------------------------------------------------------------------------- MFCC

def mel_weight_matrix(num_mel_bins=NUM_MEL, num_spectrogram_bins=FRAME_LEN // 2 + 1, sample_rate=FS,
                      lower_edge_hertz=MEL_LO, upper_edge_hertz=MEL_HI):
    W = np.zeros((num_spectrogram_bins, num_mel_bins), np.float64)
    port().oracle_mel_weight_matrix(num_mel_bins, num_spectrogram_bins, float(sample_rate), float(lower_edge_hertz),
                                    float(upper_edge_hertz), _p(W))
    return W


def mfcc(x, variant, n_frames=None, frame_len=FRAME_LEN, frame_step=FRAME_LEN, use_log=False, stages=False,
         n_threads=1, num_mel_bins=NUM_MEL, sample_rate=FS, lower_edge_hertz=MEL_LO, upper_edge_hertz=MEL_HI,
         mel_mtx_scale=MEL_SCALE):
    """x: 1-D int16 stream. Returns mfcc [n_frames, num_mel_bins] float64 (plus stage arrays if stages)."""
    x = np.ascontiguousarray(x, dtype=np.int16).ravel()
    if n_frames is None:
        n_frames = 1 + (x.shape[0] - frame_len) // frame_step  # mfcc_utils.py:154-155
    if n_frames <= 0:
        return np.zeros((0, num_mel_bins))
    assert (n_frames - 1) * frame_step + frame_len <= x.shape[0]
    nspec = frame_len // 2 if variant == VARIANT_A else frame_len // 2 + 1 if variant == VARIANT_TF else frame_len
    out = np.zeros((n_frames, num_mel_bins), np.float64)
    sp = np.zeros((n_frames, nspec), np.float64) if stages else None
    me = np.zeros((n_frames, num_mel_bins), np.float64) if stages else None
    lm = np.zeros((n_frames, num_mel_bins), np.float64) if stages else None
    r = port().oracle_mfcc(_p(x), n_frames, frame_len, frame_step, variant, num_mel_bins, float(sample_rate),
                           float(lower_edge_hertz), float(upper_edge_hertz), float(mel_mtx_scale), int(bool(use_log)),
                           _p(sp), _p(me), _p(lm), _p(out), int(n_threads))
    if r != 0:
        raise RuntimeError("oracle_mfcc failed: %d" % r)
    if stages:
        return out, dict(spectrogram=sp, mel_spectrogram=me, log_mel_spectrogram=lm)
    return out


def mfcc_numpy(x, variant, frame_len, frame_step, n_frames=None, num_mel_bins=NUM_MEL, sample_rate=FS, lower_edge_hertz=MEL_LO,
               upper_edge_hertz=MEL_HI, mel_mtx_scale=MEL_SCALE, use_log=False):
    """Variants A / B (and TF: unpinned) for ANY frame length (numpy's FFT, like the reference: mfcc_utils.py:160-197, 287-322) -- the checker of the
    generality kernel where the C restatement's radix-2 FFT does not go (lengths that are no power of two). Pinned on the reference's own
    outputs for six geometries (tests/golden/mfcc_geom_golden.npz, tests/test_oracle.py). The mel matrix is the C restatement's
    (oracle_mel_weight_matrix, itself pinned on the reference's gen_mel_weight_matrix)."""
    x = np.ascontiguousarray(x, dtype=np.int16).ravel()
    N = int(frame_len)
    if n_frames is None:
        n_frames = 1 + (x.shape[0] - N) // frame_step
    nb = N // 2 if variant == VARIANT_A else N // 2 + 1
    if variant == VARIANT_TF:
        # mfcc_utils.py:201-253 (fft_len == frame_len): float32 samples times tf.signal.hann_window(N, periodic=True) in float32, rfft, |.|, the
        # (N/2+1)-bin matrix, ln(x + 1e-6), mfccs_from_log_mel_spectrograms = DCT-II * rsqrt(2 num_mel_bins). PARITY UNPINNED (no TensorFlow here).
        win = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(np.float32)
    W = mel_weight_matrix(num_mel_bins, nb, sample_rate, lower_edge_hertz, upper_edge_hertz)
    k = np.arange(num_mel_bins)
    D = 2.0 * np.cos(np.pi * np.outer(k, 2 * np.arange(num_mel_bins) + 1) / (2.0 * num_mel_bins))   # scipy.fftpack.dct type 2, unnormalised
    out = np.zeros((max(n_frames, 0), num_mel_bins))
    for f in range(n_frames):
        if variant == VARIANT_TF:
            xw = (x[f * frame_step:f * frame_step + N].astype(np.float32) * win).astype(np.float64)
            out[f] = D @ np.log(np.abs(np.fft.rfft(xw)) @ W + 1e-6) / np.sqrt(2.0 * num_mel_bins)
            continue
        X = np.fft.fft(x[f * frame_step:f * frame_step + N].astype(np.float64))
        if variant == VARIANT_A:
            out[f] = D @ np.log(np.abs(X[:nb]) @ W + 1e-6) / np.sqrt(2.0 * num_mel_bins)
        else:
            e = ((np.abs(X / 1024.0) / np.sqrt(2.0))[:nb] @ (mel_mtx_scale * W)) / mel_mtx_scale
            out[f] = D @ (np.log(e + 1e-6) if use_log else e) / 64.0
    return out


def net_input(mfcc_rows, n_coef=NUM_MFCC, scale=1.0, clip_lo=-128.0, clip_hi=127.0):
    m = np.ascontiguousarray(mfcc_rows, dtype=np.float64)
    n, stride = m.shape
    out = np.zeros((n, n_coef), np.int8)
    port().oracle_net_input(_p(m), n, stride, n_coef, float(scale), float(clip_lo), float(clip_hi), _p(out))
    return out


# ------------------------------------------------------------------ MFCC variant C (firmware Q15)

# Float -> Q15 conversion of the regenerated CMSIS tables that reproduces the reference's published
# host-vs-board statistics (README.md:121-139; tests/golden/gen_fixtures_q15.py): twiddles floor, split tables round.
Q15_TW_MODE, Q15_RC_MODE = 0, 1


class Q15Tables:
    def __init__(self, tw_mode=Q15_TW_MODE, rc_mode=Q15_RC_MODE, sample_rate=FS, lower_edge_hertz=MEL_LO,
                 upper_edge_hertz=MEL_HI, mel_mtx_scale=MEL_SCALE):
        self.scale = int(mel_mtx_scale)
        self.h = port().oracle_q15_tables_new(tw_mode, rc_mode, NUM_MEL, float(sample_rate), float(lower_edge_hertz),
                                              float(upper_edge_hertz), self.scale)
        if not self.h:
            raise RuntimeError("oracle_q15_tables_new failed")

    def arrays(self):
        tw1024, tw16 = np.zeros(1536, np.int16), np.zeros(24, np.int16)
        rfa, rfb = np.zeros(32, np.int16), np.zeros(32, np.int16)
        coef, start, count = np.zeros(2048, np.int16), np.zeros(32, np.int16), np.zeros(32, np.int16)
        n = port().oracle_q15_tables_get(self.h, _p(tw1024), _p(tw16), _p(rfa), _p(rfb), _p(coef), _p(start), _p(count))
        return dict(tw1024=tw1024, tw16=tw16, rfa=rfa, rfb=rfb, mel_coef=coef[:n].copy(), mel_start=start,
                    mel_count=count)

    def __del__(self):
        if getattr(self, "h", None):
            port().oracle_q15_tables_free(self.h)
            self.h = None


_q15_default = None


def mfcc_q15(x, n_frames=None, frame_step=FRAME_LEN, stages=False, n_threads=1, tables=None):
    """audioCalcMFCCs on every frame of the int16 stream x -> int16 [n_frames, 32] (plus stage arrays)."""
    global _q15_default
    if tables is None:
        if _q15_default is None:
            _q15_default = Q15Tables()
        tables = _q15_default
    x = np.ascontiguousarray(x, dtype=np.int16).ravel()
    if n_frames is None:
        n_frames = 1 + (x.shape[0] - FRAME_LEN) // frame_step if x.shape[0] >= FRAME_LEN else 0
    out = np.zeros((max(n_frames, 0), NUM_MEL), np.int16)
    if n_frames <= 0:
        return (out, dict(fft=np.zeros((0, 1024, 2), np.int16), spectrogram=np.zeros((0, 513), np.int16),
                          mel_spectrogram=np.zeros((0, 32), np.int16))) if stages else out
    assert (n_frames - 1) * frame_step + FRAME_LEN <= x.shape[0]
    fft = np.zeros((n_frames, 1024, 2), np.int16) if stages else None
    sp = np.zeros((n_frames, 513), np.int16) if stages else None
    me = np.zeros((n_frames, NUM_MEL), np.int16) if stages else None
    r = port().oracle_mfcc_q15(tables.h, _p(x), n_frames, frame_step, tables.scale, _p(fft), _p(sp), _p(me), _p(out),
                               int(n_threads))
    if r != 0:
        raise RuntimeError("oracle_mfcc_q15 failed: %d" % r)
    if stages:
        return out, dict(fft=fft, spectrogram=sp, mel_spectrogram=me)
    return out


def net_input_q15(mfcc_rows, n_coef=NUM_MFCC, scale=1, clip_lo=-128, clip_hi=127):
    m = np.ascontiguousarray(mfcc_rows, dtype=np.int16)
    n, stride = m.shape
    out = np.zeros((n, n_coef), np.int8)
    port().oracle_net_input_q15(_p(m), n, stride, n_coef, scale, clip_lo, clip_hi, _p(out))
    return out


class MfccF32:
    """Variant D: mfcc_create / mfcc_compute of firmware/src/audio/mfcc.c (defaults = app.c:540)."""

    def __init__(self, num_mfcc_features=13, feature_offset=1, frame_len=512, mfcc_dec_bits=8, preempha=0.97):
        self.h = port().oracle_f32_mfcc_new(num_mfcc_features, feature_offset, frame_len, mfcc_dec_bits, preempha)
        if not self.h:
            raise ValueError("bad mfcc_create arguments")
        self.frame_len, self.n_out, self.feature_offset = frame_len, port().oracle_f32_mfcc_n_out(self.h), feature_offset

    def __call__(self, x, n_frames=None, frame_step=None, n_threads=1):
        """-> (int8 [n, n_out], float32 [n, n_out] before round/saturate, float32 log-mel [n, 26])"""
        x = np.ascontiguousarray(x, dtype=np.int16).ravel()
        step = self.frame_len if frame_step is None else frame_step
        if n_frames is None:
            n_frames = 1 + (x.shape[0] - self.frame_len) // step if x.shape[0] >= self.frame_len else 0
        n = max(n_frames, 0)
        out = np.zeros((n, self.n_out), np.int8)
        f32 = np.zeros((n, self.n_out), np.float32)
        lm = np.zeros((n, 26), np.float32)
        if n:
            assert (n - 1) * step + self.frame_len <= x.shape[0]
            port().oracle_f32_mfcc_run(self.h, _p(x), n, step, _p(out), _p(f32), _p(lm), int(n_threads))
        return out, f32, lm

    def tables(self):
        """The restated tables: dct [n_features, 26] f32, first [26], last [26], weights (rows back to back) f32."""
        nf = port().oracle_f32_mfcc_n_out(self.h) + self.feature_offset
        dct = np.zeros((nf, 26), np.float32)
        first, last, w = np.zeros(26, np.int32), np.zeros(26, np.int32), np.zeros(8192, np.float32)
        n = port().oracle_f32_mfcc_tables_get(self.h, _p(dct), _p(first), _p(last), _p(w), w.size)
        assert n >= 0
        return dct, first, last, w[:n].copy()

    def window(self):
        """The Hann window as mfcc_create holds it: [frame_len] f32."""
        w = np.zeros(self.frame_len, np.float32)
        assert port().oracle_f32_mfcc_window_get(self.h, _p(w), w.size) == self.frame_len
        return w

    def __del__(self):
        if getattr(self, "h", None):
            port().oracle_f32_mfcc_free(self.h)
            self.h = None


def output_filter(softmax, state=None, alpha=0.9, threshold=0.5):
    """app.c:332-356 over consecutive int8 softmax rows; returns (filt [n,10] f32, likely [n], spotted [n], state [10])."""
    s = np.ascontiguousarray(softmax, dtype=np.int8).reshape(-1, 10)
    n = s.shape[0]
    st = np.zeros(10, np.float32) if state is None else np.array(state, dtype=np.float32)
    filt = np.zeros((n, 10), np.float32)
    likely, spotted = np.zeros(n, np.int32), np.zeros(n, np.int32)
    port().oracle_output_filter(_p(s), n, float(alpha), float(threshold), _p(st), _p(filt), _p(likely), _p(spotted))
    return filt, likely, spotted, st


# -------------------------------------------------------------------------------------------- CNN

class Model:
    """Independent reader of the .ednn blob written by tools/import_weights_h.py."""

    def __init__(self, path=DEFAULT_MODEL):
        raw = open(path, "rb").read()
        if raw[:8] != b"EDNNOM1\0":
            raise ValueError("bad model magic")
        self.in_h, self.in_w, self.in_c, n_layers, payload_bytes, flags, _, _ = struct.unpack("<8i", raw[8:40])
        recs = [struct.unpack("<12i", raw[40 + 48 * i:88 + 48 * i]) for i in range(n_layers)]
        payload = np.frombuffer(raw[40 + 48 * n_layers:40 + 48 * n_layers + payload_bytes], dtype=np.int8)
        self.layers, self._keep = [], []
        h, w, c = self.in_h, self.in_w, self.in_c
        self.act_sizes = []
        arr = (_Layer * n_layers)()
        for i, r in enumerate(recs):
            L = dict(type=r[0])
            if r[0] == L_CONV:
                L.update(out_ch=r[1], kh=r[2], kw=r[3], sh=r[4], sw=r[5], bias_lshift=r[6], out_rshift=r[7],
                         relu=r[8], in_ch=r[11])
                L["w"] = np.ascontiguousarray(payload[r[9]:r[9] + r[1] * r[2] * r[3] * c]).reshape(r[1], r[2], r[3], c)
                L["b"] = np.ascontiguousarray(payload[r[10]:r[10] + r[1]])
                h, w, c = (h - r[2]) // r[4] + 1, (w - r[3]) // r[5] + 1, r[1]
            elif r[0] == L_POOL:
                L.update(kh=r[2], kw=r[3], sh=r[4], sw=r[5])
                h, w = (h - r[2]) // r[4] + 1, (w - r[3]) // r[5] + 1
            elif r[0] == L_DENSE:
                n_in = h * w * c
                L.update(out_ch=r[1], bias_lshift=r[6], out_rshift=r[7])
                L["w"] = np.ascontiguousarray(payload[r[9]:r[9] + r[1] * n_in]).reshape(r[1], n_in)
                L["b"] = np.ascontiguousarray(payload[r[10]:r[10] + r[1]])
                h, w, c = 1, 1, r[1]
                self.n_logits = r[1]
            elif r[0] == L_SOFTMAX:
                pass
            else:
                raise ValueError("unknown layer type %d" % r[0])
            self.layers.append(L)
            self.act_sizes.append(h * w * c)
            a = arr[i]
            a.type = r[0]
            a.out_ch, a.kh, a.kw, a.sh, a.sw = L.get("out_ch", 0), L.get("kh", 0), L.get("kw", 0), L.get("sh", 0), L.get("sw", 0)
            a.bias_lshift, a.out_rshift, a.relu = L.get("bias_lshift", 0), L.get("out_rshift", 0), L.get("relu", 0)
            a.w = L["w"].ctypes.data if "w" in L else None
            a.b = L["b"].ctypes.data if "b" in L else None
        self._arr = arr
        self.n_out = h * w * c
        self.in_size = self.in_h * self.in_w * self.in_c


def cnn(model, feats, want_acts=False, n_threads=1):
    """feats: [n, 403] int8. Returns dict(logits, softmax, argmax[, acts = list of per-layer arrays])."""
    f = np.ascontiguousarray(feats, dtype=np.int8).reshape(-1, model.in_size)
    n = f.shape[0]
    logits = np.zeros((n, model.n_logits), np.int8)
    soft = np.zeros((n, model.n_out), np.int8)
    am = np.zeros(n, np.int32)
    stride = int(sum(model.act_sizes))
    acts = np.zeros((n, stride), np.int8) if want_acts else None
    r = port().oracle_cnn_run(ctypes.cast(model._arr, ctypes.c_void_p), len(model.layers), model.in_h, model.in_w,
                              model.in_c, _p(f), n, _p(acts), stride, _p(logits), _p(soft), _p(am), int(n_threads))
    if r != 0:
        raise RuntimeError("oracle_cnn_run failed: %d" % r)
    out = dict(logits=logits, softmax=soft, argmax=am)
    if want_acts:
        offs = np.concatenate([[0], np.cumsum(model.act_sizes)])
        out["acts"] = [acts[:, offs[i]:offs[i + 1]] for i in range(len(model.act_sizes))]
    return out


def nnom_ref_batch(feats):
    """The reference itself (NNoM + CMSIS-NN + weights.h): logits, softmax, argmax for [n, 403] int8."""
    f = np.ascontiguousarray(feats, dtype=np.int8).reshape(-1, 403)
    n = f.shape[0]
    logits = np.zeros((n, 10), np.int8)
    soft = np.zeros((n, 10), np.int8)
    am = np.zeros(n, np.int32)
    r = ref().nnom_ref_run_batch(_p(f), n, _p(logits), _p(soft), _p(am))
    if r != 0:
        raise RuntimeError("nnom_ref_run_batch failed: %d" % r)
    return dict(logits=logits, softmax=soft, argmax=am)


def nnom_ref_layers(feat):
    """Per-layer activations of ONE utterance from the reference: list of int8 arrays in execution order
    (input, conv1, pool1, conv2, pool2, conv3, conv4, dense, softmax, output)."""
    f = np.ascontiguousarray(feat, dtype=np.int8).reshape(403)
    dump = np.zeros(16384, np.int8)
    sizes = np.zeros(16, np.int32)
    types = np.zeros(16, np.int32)
    n = ref().nnom_ref_run_layers(_p(f), _p(dump), dump.size, _p(sizes), _p(types), 16)
    if n < 0:
        raise RuntimeError("nnom_ref_run_layers failed: %d" % n)
    offs = np.concatenate([[0], np.cumsum(sizes[:n])])
    return [dump[offs[i]:offs[i + 1]].copy() for i in range(n)]

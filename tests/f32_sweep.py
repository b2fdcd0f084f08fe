"""The sweep of MFCC variant D, the firmware's float32 mfcc_create / mfcc_compute (csrc/mfcc_f32_kernels.hip, csrc/edison_f32.hip,
csrc/tables_f32.c): named configurations, the launch code restated, the frame counts that reach every case of the two kernels' work
splits, seeded inputs, a float64 reference and the bars.

Test infrastructure, not a test: tests/test_f32_sweep_cpu.py checks that the rows cover the table of DESIGN.md section 4.6a, that every
note names the kernel the restated dispatch gives its row, that counts() reaches every split case, that reference64 agrees with the
reference-made fixture and with both references, and that BARS are what the two references measure; tests/test_gpu_f32_sweep.py runs
every row on the GPU. Run as a program it is the child process of that file (see main()).

Variant D is two kernels behind edison_mfcc_f32_batch_dev:
    generic  ed_mfcc_f32_kernel: radix-2 in LDS, EF_WPB waves per workgroup, one frame per wave, padded sizes 128 .. 1024
    fast     ed_mfcc_f32_fast_kernel: padded 512 only (frame lengths 257 .. 512); two frames in the halves of packed fp32 registers,
             EF2_WPB waves per workgroup, a pair range per workgroup and a queue counter in LDS
EDISON_F32_GENERIC=1 (read once per process) sends padded 512 to the generic kernel too.

A row is a dict: n_features, offset, frame_len, dec_bits, preemph (the arguments of mfcc_create), hop (frame_step; 0: every frame is
the first one, n_frames given explicitly) and note = "<fast|generic> <padded>; why".
"""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edison_amd", "csrc")
N_BASE = 64
N_FBANK = 26
CU_LDS_BYTES = 160 * 1024
FLT_MIN = float(np.finfo(np.float32).tiny)
CLEAR = 1e-3          # a band is clear of the frame's float32 rounding floor when it holds more than this share of the largest bin

# ---- the bars: derived from the two references alone (tests/test_f32_sweep_cpu.py recomputes them), never from GPU output -----------
# Largest error against reference64 over the frames the sweep runs (measure(): every row's 64 base frames and, where the hop cuts across
# them, the stream of the row's largest count), measured 2026-10-17:
#                                                                   compiled mfcc_compute + CMSIS transform   oracle.MfccF32 (FFT in double)
#   lin   |band energy - ref| / the frame's largest bin                          1.63e-5 (g1000)                  1.63e-5 (g1000)
#   log   |log-mel - ref| on clear bands                                         6.68e-5 (g65)                    1.57e-5 (g65)
#   coef  |coefficient - ref| / 2^dec_bits on frames of clear bands              2.24e-5 (f512_sat, g128, ...)    1.48e-5 (f257_hop1)
#   dct   |pre-rounding float - float64 DCT of its OWN float32 log-mel| / 2^dec_bits, EVERY frame:   (returns no floats)   1.69e-5 (silence, c0)
# Each bar is the larger maximum x MARGIN, rounded up to one significant digit (tests/test_f32_sweep_cpu.py holds them to that).
# The linear figure is read back from the float32 log-mel output, so it carries that value's rounding: |lm| ulp(lm) / 2 of the band, and
# a band of a flat spectrum (one quiet sample inside a cut frame) holds several times the largest bin -- which is why both references
# share the largest figure. On the base frames alone the maxima are 4.06e-6 / 2.44e-5 / 2.24e-5.
MARGIN = 2
BARS = dict(lin=4e-5, log=2e-4, coef=5e-5, dct=4e-5)
INT8_CAP = 0.10       # share of the held int8 values that may lie within the coefficient bar of a rounding boundary: a condition on the rows

# ---- the rows -------------------------------------------------------------------------------------------------------------------------
ROWS = {}


def _row(name, n_features, offset, frame_len, dec_bits, preemph, hop, note):
    ROWS[name] = dict(name=name, n_features=n_features, offset=offset, frame_len=frame_len, dec_bits=dec_bits, preemph=preemph, hop=hop, note=note)


# the fast kernel: frame lengths 257 .. 512
_row("firmware", 13, 1, 512, 8, 0.97, 256, "fast 512; mfcc_create(13, 1, 512, 8, 0.97f) at the NNoM example's hop, frame_len / 2")
_row("firmware_whole", 13, 1, 512, 8, 0.97, 512, "fast 512; the firmware's configuration at hop = frame_len: position independence bit for bit")
_row("firmware_hop0", 13, 1, 512, 8, 0.97, 0, "fast 512; hop 0: every frame is the first one")
_row("f257_hop1", 26, 0, 257, 2, 0.0, 1, "fast 512; the shortest frame: 255 clamped lanes, all 26 features, no pre-emphasis, hop 1")
_row("f400_over", 20, 7, 400, 0, 0.97, 401, "fast 512; an odd hop one above the frame length, features 7 .. 19, dec_bits 0")
_row("f511_one", 26, 25, 511, 30, 1.0, 511, "fast 512; one lane short of full, one output (feature 25), dec_bits 30, pre-emphasis 1.0")
_row("f512_sat", 1, 0, 512, 24, 0.97, 512, "fast 512; coefficient 0 alone at a dec_bits where every value saturates")
# the generic kernel: every other padded size
_row("g65", 13, 1, 65, 8, 0.97, 32, "generic 128; the shortest frame of the smallest padded size, hop frame_len / 2")
_row("g128", 26, 0, 128, 0, 0.0, 128, "generic 128; a full frame, all 26 features")
_row("g129_hop1", 20, 7, 129, 2, 1.0, 1, "generic 256; one sample over 128, pre-emphasis 1.0, hop 1")
_row("g256", 13, 1, 256, 8, 0.97, 257, "generic 256; a full frame, an odd hop above the frame length")
_row("g513_one", 26, 25, 513, 30, 0.97, 513, "generic 1024; one sample over the fast kernel's range, one output, dec_bits 30")
_row("g1000", 13, 1, 1000, 8, 0.97, 333, "generic 1024; an odd hop below the frame length")
_row("g1024_sat", 1, 0, 1024, 24, 0.0, 1024, "generic 1024; the largest frame, every value saturates")

TABLE = dict(
    fast_frame_len=(257, 400, 511, 512), generic_frame_len=(65, 128, 129, 256, 513, 1000, 1024),
    features=((13, 1), (26, 0), (26, 25), (1, 0), (20, 7)), dec_bits=(0, 2, 8, "saturating", 30), preemph=(0.0, 0.97, 1.0),
    hop=("1", "odd", "half", "whole", "over", "0"))
SATURATING = ("f512_sat", "g1024_sat", "f511_one", "g513_one")     # rows in which every held value must lie beyond both saturation bounds


def row_items(row):
    """What a row covers of TABLE"""
    N, hop = row["frame_len"], row["hop"]
    out = {("fast_frame_len" if kernel(row) == "fast" else "generic_frame_len", N), ("features", (row["n_features"], row["offset"])),
           ("dec_bits", "saturating" if row["dec_bits"] == 24 else row["dec_bits"]), ("preemph", row["preemph"])}
    if hop == 0:
        out.add(("hop", "0"))
    if hop == 1:
        out.add(("hop", "1"))
    if hop > 1 and hop % 2:
        out.add(("hop", "odd"))
    if hop == N // 2:
        out.add(("hop", "half"))
    if hop == N:
        out.add(("hop", "whole"))
    if hop > N:
        out.add(("hop", "over"))
    return out


def full_items():
    return {(k, v) for k, vs in TABLE.items() for v in vs}


def create_args(row):
    return dict(num_mfcc_features=row["n_features"], feature_offset=row["offset"], frame_len=row["frame_len"], mfcc_dec_bits=row["dec_bits"],
                preemph=row["preemph"])


# ---- the launch code, restated --------------------------------------------------------------------------------------------------------
def _src():
    return open(os.path.join(CSRC, "mfcc_f32_kernels.hip")).read()


def ef_wpb():
    """EF_WPB: waves (= frames) per workgroup of the generic kernel"""
    return int(re.search(r"^#define EF_WPB (\d+)", _src(), re.M).group(1))


def ef2_wpb():
    """EF2_WPB of the product build: waves per workgroup of the fast kernel"""
    return int(re.search(r"#ifndef EF2_WPB\s*\n#define EF2_WPB (\d+)", _src()).group(1))


def padded(frame_len):
    p = 1
    while p < frame_len:
        p <<= 1
    return p


def kernel(row, generic_env=False):
    """edison_mfcc_f32_batch_dev's choice"""
    return "fast" if padded(row["frame_len"]) == 512 and not generic_env else "generic"


def note_kernel(note):
    k, p = note.split(";")[0].split()
    return k, int(p)


def fast_split(n, n_cu):
    """[(s0, cnt)] per workgroup of ed_mfcc_f32_fast_kernel: its slice of the frame pairs (grid as ed_launch_mfcc_f32_fast sizes it)"""
    w = ef2_wpb()
    n_pairs = (n + 1) // 2
    blocks = min((n_pairs + w - 1) // w, n_cu)
    return [(b * n_pairs // blocks, (b + 1) * n_pairs // blocks - b * n_pairs // blocks) for b in range(blocks)]


def fast_draws(n, n_cu):
    """Pairs per wave that come out of the LDS queue, in the workgroup with the fewest: a wave's first two pairs are its number and its
    number + EF2_WPB, every further pair of the slice is a queue draw (the counter starts at 2 EF2_WPB)"""
    w = ef2_wpb()
    return min(max(0, c - 2 * w) for _, c in fast_split(n, n_cu)) / w


def generic_per_cu(p):
    lds = ef_wpb() * p * 8
    return max(1, min(8, CU_LDS_BYTES // (lds + 12 * 1024)))


def generic_cap(p, n_cu):
    return n_cu * generic_per_cu(p)


def generic_blocks(n, p, n_cu):
    return min((n + ef_wpb() - 1) // ef_wpb(), generic_cap(p, n_cu))


def cases(row, n, n_cu, generic_env=False):
    """What a frame count does to the row's kernel, as tags"""
    out = set()
    if kernel(row, generic_env) == "fast":
        w, s = ef2_wpb(), fast_split(n, n_cu)
        cnts = [c for _, c in s]
        if n % 2:
            out.add("fast: odd, the last pair has no frame B")
        if n == 1:
            out.add("fast: one frame")
        if len(s) == 1 and cnts[0] < w:
            out.add("fast: one workgroup, fewer pairs than waves")
        if len(s) == 1 and cnts[0] == w:
            out.add("fast: one workgroup, one pair per wave")
        if len(s) > 1 and min(cnts) < w:
            out.add("fast: several workgroups, waves without a pair")
        if len(set(cnts)) > 1:
            out.add("fast: uneven slices")
        if len(s) == n_cu and set(cnts) == {w}:
            out.add("fast: one workgroup per CU, one pair per wave")
        if len(s) == n_cu and sorted(set(cnts)) == [w, w + 1]:
            out.add("fast: one workgroup per CU and one pair over")
        if fast_draws(n, n_cu) >= 3:
            out.add("fast: at least three queue draws per wave")
    else:
        w, p = ef_wpb(), padded(row["frame_len"])
        cap, blocks = generic_cap(p, n_cu), generic_blocks(n, p, n_cu)
        if n < w:
            out.add("generic: one workgroup, waves without a frame")
        if n == w:
            out.add("generic: one full workgroup")
        if 1 < blocks and n <= w * cap and n % w:
            out.add("generic: ragged last workgroup, no grid stride")
        if blocks == cap and w * cap < n <= 2 * w * cap:
            out.add("generic: grid stride, second round ragged")
        if blocks == cap and n > 2 * w * cap and n % w:
            out.add("generic: several rounds of the grid stride, ragged end")
        if blocks == cap and n == w * cap - 1:
            out.add("generic: the grid exactly at its cap")
    return out


FAST_CASES = ("fast: odd, the last pair has no frame B", "fast: one frame", "fast: one workgroup, fewer pairs than waves",
              "fast: one workgroup, one pair per wave", "fast: several workgroups, waves without a pair", "fast: uneven slices",
              "fast: one workgroup per CU, one pair per wave", "fast: one workgroup per CU and one pair over",
              "fast: at least three queue draws per wave")
GENERIC_CASES = ("generic: one workgroup, waves without a frame", "generic: one full workgroup", "generic: ragged last workgroup, no grid stride",
                 "generic: grid stride, second round ragged", "generic: several rounds of the grid stride, ragged end",
                 "generic: the grid exactly at its cap")


def counts(row, n_cu, generic_env=False):
    """The frame counts row `row` runs on a device of n_cu compute units: every case of cases()"""
    if kernel(row, generic_env) == "fast":
        w = ef2_wpb()
        full = 2 * w * n_cu
        return sorted({1, 2, 3, 2 * w - 1, 2 * w, 2 * w + 1, 2 * (3 * w + 5), full - 1, full, full + 1, 5 * full + 7})
    w, cap = ef_wpb(), generic_cap(padded(row["frame_len"]), n_cu)
    return sorted({1, 3, 4, 5, w * cap - 1, w * cap + 1, 2 * w * cap + 3})


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
KINDS = dict(zero=0, rail_pos=1, rail_neg=2, square=3, impulse=4, hop0=50)     # hop0: a speech-like frame at about 3 % of full scale


def _speechlike(rng, n, N):
    """noise with the long-term tilt of speech: white noise through y[i] = 0.9 y[i-1] + x[i], unit rms"""
    x = rng.normal(0, 1, (n, N + 64))
    y = np.zeros_like(x)
    for i in range(1, N + 64):
        y[:, i] = 0.9 * y[:, i - 1] + x[:, i]
    y = y[:, 64:]
    return y / np.sqrt((y * y).mean(axis=1, keepdims=True))


def base_frames(row):
    """([64, frame_len] int16, position of every special frame): 0 silence, 1 / 2 the rails +32767 / -32768, 3 a square wave at fs / 2
    between the rails, 4 one full-scale impulse in mid-frame, 5 .. 8 tones on bin centres of the padded transform (two pure, two over a
    noise floor), 9 .. 63 speech-like noise with rms from 0.3 LSB to full scale, five decades; then shuffled."""
    N, P = row["frame_len"], padded(row["frame_len"])
    rng = np.random.default_rng(4000 + N)
    t = np.arange(N)
    f = np.zeros((N_BASE, N))
    f[1], f[2] = 32767, -32768
    f[3] = np.where(t & 1, -32768, 32767)
    f[4, N // 2] = 32767
    floor = _speechlike(rng, 2, N)
    for j, (k, amp) in enumerate(((P // 16, 30000.0), (P // 8 + 1, 300.0), (P // 5, 8000.0), (P // 4 - 2, 1000.0))):
        f[5 + j] = amp * np.cos(2 * np.pi * k * t / P + rng.uniform(0, 2 * np.pi))
        if j >= 2:
            f[5 + j] += 0.05 * amp * floor[j - 2]
    n = N_BASE - 9
    f[9:] = _speechlike(rng, n, N) * (0.3 * 10.0 ** (5.0 * np.arange(n) / (n - 1)))[:, None]
    x = np.clip(np.rint(f), -32768, 32767).astype(np.int16)
    perm = rng.permutation(N_BASE)
    where = {k: int(np.nonzero(perm == v)[0][0]) for k, v in KINDS.items()}
    return x[perm], where


def tile_index(n):
    """Base frame of frame slot i: partners and positions vary from one repetition of the set to the next"""
    i = np.arange(n)
    return (i + i // N_BASE) % N_BASE


def audio(row, n, base=None):
    """(int16 stream, idx): n frames at the row's hop. hop >= frame_len: frame slot i is exactly base[idx[i]] (idx from tile_index), the
    gaps hold filler; 0 < hop < frame_len: the base frames idx[0], idx[1], ... back to back, cut every hop samples (idx[i] is then
    only the frame the cut starts in); hop 0: the base frame KINDS calls hop0, alone."""
    N, hop = row["frame_len"], row["hop"]
    where = base_frames(row)[1]
    if base is None:
        base = base_frames(row)[0]
    if hop == 0:
        return base[where["hop0"]].copy(), np.full(n, where["hop0"])
    idx = tile_index(n)
    if hop >= N:
        x = np.full(((n - 1) * hop + N,), 12345, np.int16) if hop > N else np.empty(n * N, np.int16)
        pos = (np.arange(n) * hop)[:, None] + np.arange(N)[None, :]
        x[pos.reshape(-1)] = base[idx].reshape(-1)
        return x, idx
    total = (n - 1) * hop + N
    k = -(-total // N)
    return base[tile_index(k)].reshape(-1)[:total].copy(), tile_index(k)[(np.arange(n) * hop) // N]



class F32Tables(ctypes.Structure):
    """ed_f32_tables_t (edison_amd/csrc/edison_internal.h), for the tests that read what ed_build_f32_tables hands the kernels"""
    _fields_ = [("n_features", ctypes.c_int32), ("offset", ctypes.c_int32), ("frame_len", ctypes.c_int32), ("padded", ctypes.c_int32),
                ("log2p", ctypes.c_int32), ("dec_bits", ctypes.c_int32), ("preempha", ctypes.c_float), ("scale", ctypes.c_float),
                ("window", ctypes.c_float * 1024), ("tw", ctypes.c_float * 1024),
                ("mel_first", ctypes.c_int32 * 26), ("mel_last", ctypes.c_int32 * 26), ("mel_off", ctypes.c_int32 * 26),
                ("mel_w", ctypes.c_float * 1100), ("dct", ctypes.c_float * (26 * 26))]


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------
_TABLES = {}


def tables(row):
    """(window [N], mel weights [26, P / 2 + 1], DCT rows offset .. n_features - 1 [n_out, 26]) as float64: the float32 values of
    tables_f32.c, from the oracle's builders (pinned on the reference's object code: tests/test_oracle_refpins.py), widened"""
    key = (row["n_features"], row["offset"], row["frame_len"])
    if key not in _TABLES:
        from oracle import oracle
        o = oracle.MfccF32(row["n_features"], row["offset"], row["frame_len"], row["dec_bits"], row["preemph"])
        dct, first, last, w = o.tables()
        W = np.zeros((N_FBANK, padded(row["frame_len"]) // 2 + 1))
        pos = 0
        for b in range(N_FBANK):
            if first[b] >= 0:
                k = last[b] - first[b] + 1
                W[b, first[b]:last[b] + 1] = w[pos:pos + k]
                pos += k
        assert pos == w.size
        _TABLES[key] = (o.window().astype(np.float64), W, dct[row["offset"]:].astype(np.float64))
    return _TABLES[key]


def reference64(row, x, n, hop):
    """mfcc.c:174-255 in float64 on the float32 tables: (scaled coefficients before rounding [n, n_out], log-mel [n, 26], the largest
    |X[k]| of every frame [n])"""
    N, P = row["frame_len"], padded(row["frame_len"])
    win, W, D = tables(row)
    pre = float(np.float32(row["preemph"]))
    scale = float(1 << row["dec_bits"])
    x = np.ascontiguousarray(x, dtype=np.int16)
    assert n == 0 or (n - 1) * hop + N <= x.size
    C, LM, SM = np.zeros((n, D.shape[0])), np.zeros((n, N_FBANK)), np.zeros(n)
    for lo in range(0, n, 4096):
        hi = min(n, lo + 4096)
        fr = x[(np.arange(lo, hi) * hop)[:, None] + np.arange(N)[None, :]].astype(np.float64)
        v = np.empty_like(fr)
        v[:, 0] = fr[:, 0]                                              # sample 0 is neither pre-emphasised nor scaled (mfcc.c:178-181)
        v[:, 1:] = (fr[:, 1:] - pre * fr[:, :-1]) / 32768.0
        mag = np.abs(np.fft.rfft(v * win, P, axis=1))
        e = mag @ W.T
        e[e == 0.0] = FLT_MIN
        LM[lo:hi] = np.log(e)
        SM[lo:hi] = mag.max(axis=1)
        C[lo:hi] = (LM[lo:hi] @ D.T) * scale
    return C, LM, SM


def round_half_away(c):
    """int8 of mfcc.c:249-254: round half away from zero, saturate"""
    r = np.sign(c) * np.floor(np.abs(c) + 0.5)
    return np.clip(r, -128, 127).astype(np.int8)


def clear_bands(lm64, spec_max):
    """Bands that stand clear of the frame's float32 rounding floor (or are exactly empty: FLT_MIN in every implementation)"""
    e = np.exp(lm64)
    return (e > CLEAR * spec_max[:, None]) | (lm64 == np.log(FLT_MIN))


def errors(row, ref, lm, coef=None):
    """The three figures of BARS for log-mel energies lm [n, 26] (and pre-rounding scaled coefficients coef [n, n_out]) against
    ref = reference64(...): (lin, log, coef), each the maximum over the frames; plus the mask of the frames held to the coefficient
    and int8 bars (every band clear)"""
    C, LM, SM = ref
    lm = lm.astype(np.float64)
    lin = np.abs(np.exp(lm) - np.exp(LM)) / np.maximum(SM, 1e-300)[:, None]
    lin[SM == 0] = np.where(np.abs(lm[SM == 0] - LM[SM == 0]) < 1e-5, 0.0, np.inf)      # silence: FLT_MIN, whatever the largest bin
    clear = clear_bands(LM, SM)
    held = clear.all(axis=1)
    dlog = np.where(clear, np.abs(lm - LM), 0.0)
    dco = None if coef is None else np.abs(coef.astype(np.float64) - C) / float(1 << row["dec_bits"]) * held[:, None]
    return lin, dlog, dco, held


def dct_stage(row, lm, f32):
    """The last stage alone, on EVERY frame, whatever its conditioning: |pre-rounding float - float64 DCT of the SAME implementation's
    float32 log-mel energies x 2^dec_bits| / 2^dec_bits, [n, n_out]"""
    scale = float(1 << row["dec_bits"])
    return np.abs(f32.astype(np.float64) - (lm.astype(np.float64) @ tables(row)[2].T) * scale) / scale


def boundary_band(row, C, bar=None):
    """Values whose reference lies within the coefficient bar of a rounding boundary (.5 between integers inside the int8 range, the
    two saturation bounds 127.5 / -128.5 beyond it)"""
    tol = (BARS["coef"] if bar is None else bar) * float(1 << row["dec_bits"])
    inside = (C > -128.5 - tol) & (C < 127.5 + tol)
    frac = np.abs(C - np.trunc(C))
    return inside & ((np.abs(frac - 0.5) <= tol) | (np.abs(C - 127.5) <= tol) | (np.abs(C + 128.5) <= tol))


def ceil1(v):
    """v rounded up to one significant digit"""
    e = 10.0 ** np.floor(np.log10(v))
    return float(np.ceil(v / e - 1e-9) * e)


def oracle_outputs(row, x, n, hop):
    """oracle.MfccF32 (float32 in the firmware's order, FFT in double): (int8, scaled floats, log-mel)"""
    from oracle import oracle
    o = oracle.MfccF32(row["n_features"], row["offset"], row["frame_len"], row["dec_bits"], row["preemph"])
    return o(x, n_frames=n, frame_step=hop, n_threads=4)


def ref_outputs(row, x, n, hop):
    """The reference's compiled mfcc_compute + CMSIS transform: (int8, None, log-mel). It returns no pre-rounding floats: its
    coefficient figure is the float64 DCT of ITS log-mel energies (the float32 DCT's own rounding is in oracle.MfccF32's figure)."""
    from oracle import oracle
    i8, lm = oracle.mfcc_f32_ref().compute(x, n_frames=n, frame_step=hop, num_mfcc_features=row["n_features"], feature_offset=row["offset"],
                                           frame_len=row["frame_len"], mfcc_dec_bits=row["dec_bits"], preempha=row["preemph"])
    return i8, None, lm


MEASURE_N_CU = 304    # the bars do not depend on the device the tests run on: the overlapping rows are measured on the stream of the largest
                      # count of a device this size; a smaller device's streams are prefixes of it (tests/test_gpu_f32_sweep.py asserts n_cu <= this)


def measure(row, outputs):
    """(lin, log, coef, dct) maxima of a reference (oracle_outputs / ref_outputs) over the frames the sweep runs -- the row's 64 base frames
    and, where the hop cuts across them (0 < hop < frame_len), the stream of the row's largest count -- then its int8, the reference64
    tuple and the held mask, all three of the base frames"""
    base, _ = base_frames(row)
    N, hop = row["frame_len"], row["hop"]
    runs = [(base.reshape(-1), N_BASE, N)]
    if 0 < hop < N:
        n = counts(row, MEASURE_N_CU)[-1]
        runs.append((audio(row, n, base)[0], n, hop))
    worst, first = [0.0, 0.0, 0.0, 0.0], None
    for x, n, h in runs:
        ref = reference64(row, x, n, h)
        i8, f32, lm = outputs(row, x, n, h)
        own = f32 is not None
        if not own:
            f32 = (lm.astype(np.float64) @ tables(row)[2].T) * float(1 << row["dec_bits"])
        lin, dlog, dco, held = errors(row, ref, lm, f32)
        dd = dct_stage(row, lm, f32) if own else np.zeros(1)
        worst = [max(a, float(b.max())) for a, b in zip(worst, (lin, dlog, dco, dd))]
        first = first or (i8, ref, held)
    return (tuple(worst),) + first


# ---- the child process ----------------------------------------------------------------------------------------------------------------
def main(argv):
    """python f32_sweep.py OUT.npz ROW[,ROW...] [COUNT,COUNT...]: run the rows through the host entry point in THIS process (whatever
    EDISON_F32_GENERIC says here) at the given frame counts, or at counts(row, n_cu, generic_env) where none are given, and write
    int8 / float32 / log-mel of every (row, count) as "<row>/<count>/i8|f32|lm"."""
    sys.path.insert(0, ROOT)
    from edison_amd.context import default_context
    from edison_amd.mfcc.mfcc_f32 import MfccF32
    out_path, names = argv[0], argv[1].split(",")
    ctx = default_context()
    n_cu = ctx.device_info()["n_cu"]
    generic_env = os.environ.get("EDISON_F32_GENERIC", "0") not in ("", "0")
    res = {"n_cu": np.array(n_cu)}
    for name in names:
        row = ROWS[name]
        m = MfccF32(ctx=ctx, **create_args(row))
        base, _ = base_frames(row)
        for n in ([int(v) for v in argv[2].split(",")] if len(argv) > 2 else counts(row, n_cu, generic_env)):
            x, _ = audio(row, n, base)
            i8, f32, lm = m.compute(x, n_frames=n, frame_step=row["hop"], want_float=True)
            res["%s/%d/i8" % (name, n)], res["%s/%d/f32" % (name, n)], res["%s/%d/lm" % (name, n)] = i8, f32, lm
        m.close()
    np.savez(out_path, **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

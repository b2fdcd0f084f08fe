"""The sweep of MFCC variant C, the firmware's fixed-point audioCalcMFCCs (csrc/mfcc_q15_kernels.hip, csrc/edison_q15.hip,
csrc/tables_q15.c): named configurations, the launch code restated, the frame counts that reach every case of the kernel's work split
and of its deferred DCT batches, seeded inputs and the oracle calls.

Test infrastructure, not a test: tests/test_q15_sweep_cpu.py checks that the rows cover the table of DESIGN.md section 4.6b, that every
note names the kernel instance the restated dispatch gives its row, that counts() reaches every case, that the host library's tables
have the shape, Nyquist flag and scale every row claims, and that the inputs make a wrong Nyquist bin, a wrong division or a wrong
sign visible in the oracle's own output; tests/test_gpu_q15_sweep.py runs every row on the GPU. Everything is integer: every
comparison is equality, there is no tolerance.

Variant C is one kernel template, ed_mfcc_q15_kernel<STAGES, ALIGNED, NLO, NHI>, eight instances behind ed_launch_mfcc_q15:
    STAGES   the diagnostic entries (edison_mfcc_q15_stages*): FFT, spectrum and mel rows are written out, bin 512 always computed
    ALIGNED  4-byte loads of sample pairs: device pointer, frame_step and group_stride all even in samples (pointer: 4-byte aligned)
    NLO+NHI  taps per lane of the compact mel matrix: 6+18 (the shipped filterbank) or 8+24, chosen by tables_q15.c
and in the product instances the Nyquist bin is computed only when tables_q15.c found a non-zero tap on bin 512 (need_nyquist).
One workgroup of EQ_WPB waves per CU owns a contiguous slice of the frames; a wave takes frames w and w + EQ_WPB of the slice by
position, every further one from a counter in LDS, parks each frame's mel row and runs the DCT stage for EQ_NB parked rows at once, or
for what it holds when it has no frame left.

A row is a dict: fb = (sample rate, lower edge, upper edge, mel_mtx_scale), shape = (NLO, NHI) and nyquist as the tables give them
(claimed here, checked against ed_build_q15_tables on the CPU), hop (frame_step; 0: every frame is the first one), n_coef, entry and
note = "stages=<0|1> aligned=<0|1> <NLO>+<NHI> nyquist=<0|1>; why". big: the row also runs the largest count (one per shape x Nyquist).

Entries:
    host         edison_mfcc_q15_batch         host pointers (staged: the device pointer is aligned)     int16 + int8
    dev          edison_mfcc_q15_batch_dev     device tensor at an even sample offset                    int16 + int8
    dev_odd      the same at an odd sample offset into the tensor                                        int16 + int8
    float        edison_mfcc_batch_dev, EDISON_MFCC_C   the int16 values as float                        float32 + int8
    stages       edison_mfcc_q15_stages        host pointers                                             fft, spectrum, mel, int16 [32]
    dev_stages, dev_stages_odd   edison_mfcc_q15_stages_dev at an even / odd sample offset
The KWS entry (edison_kws_batch_q15*: 31 frames per group, group_stride = utt_stride) has no row: tests/test_gpu_q15_sweep.py runs it
on the shipped filterbank, the only one the shipped graph was trained on, at the strides KWS_STRIDES.

The wrapped 32-bit band sum is negative in the scale-32767 row (a chirp between the rails across the top band: C's division
truncates towards zero there). At a power-of-two scale, where the kernel divides by an add and a shift, it cannot be made negative with these
inputs: taps and magnitudes are non-negative, so the sum has to pass 2^31, and at scale 16384 the same chirp reaches 1.1e9
(tests/test_q15_sweep_cpu.py holds that figure below 2^31); the sign fix of that branch is unreachable here and is not forced.
"""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edison_amd", "csrc")
N_BASE = 64
FRAME_LEN = 1024
NUM_MEL = 32
UTT_FRAMES = 31
CU_LDS_BYTES = 160 * 1024
ZERO_CAP = 0.10       # share of the base frames whose oracle output may be all zero: a condition on the inputs
MIN_SENSITIVE = 8     # base frames in which a wrong Nyquist bin / a wrong division shows
KWS_STRIDES = (31 * 1024 + 1, 1001)     # odd and clear of the utterance; odd and overlapping

SHIPPED = (16000, 80.0, 7600.0, 128)
WIDE = (16000, 20.0, 8000.0, 128)
NYQ = (16000, 80.0, 8100.0, 128)
NYQ_64 = (16000, 300.0, 8200.0, 64)
NYQ_WIDE = (16000, 80.0, 9000.0, 128)
NYQ_WIDE_1000 = (16000, 80.0, 9000.0, 1000)
NYQ_WIDE_LO = (16000, 20.0, 8400.0, 128)
S1000 = (16000, 80.0, 7600.0, 1000)
S32767 = (16000, 80.0, 7600.0, 32767)

# ---- the rows -------------------------------------------------------------------------------------------------------------------------
ROWS = {}
ENTRIES = ("host", "dev", "dev_odd", "float", "stages", "dev_stages", "dev_stages_odd")
STAGE_ENTRIES = ("stages", "dev_stages", "dev_stages_odd")
DEVICE_ENTRIES = ("dev", "dev_odd", "float", "dev_stages", "dev_stages_odd")


def _row(name, fb, shape, nyquist, hop, n_coef, entry, note, big=False):
    ROWS[name] = dict(name=name, fb=fb, shape=shape, nyquist=nyquist, hop=hop, n_coef=n_coef, entry=entry, note=note, big=big)


# 6+18, no tap on bin 512: the shipped filterbank
_row("shipped", SHIPPED, (6, 18), 0, 1024, 13, "host", "stages=0 aligned=1 6+18 nyquist=0; the firmware's configuration, host entry, 13 coefficients")
_row("shipped_dev", SHIPPED, (6, 18), 0, 1024, 32, "dev", "stages=0 aligned=1 6+18 nyquist=0; device entry, all 32 coefficients, the largest count", big=True)
_row("shipped_odd_ptr", SHIPPED, (6, 18), 0, 1024, 13, "dev_odd", "stages=0 aligned=0 6+18 nyquist=0; an odd device pointer alone makes the loads unaligned")
_row("hop0", SHIPPED, (6, 18), 0, 0, 31, "dev", "stages=0 aligned=1 6+18 nyquist=0; hop 0: every frame is the first one")
_row("hop1", SHIPPED, (6, 18), 0, 1, 1, "host", "stages=0 aligned=0 6+18 nyquist=0; hop 1, coefficient 0 alone")
_row("hop512_float", SHIPPED, (6, 18), 0, 512, 13, "float", "stages=0 aligned=1 6+18 nyquist=0; the float output of edison_mfcc_batch_dev, half-overlapping frames")
_row("hop1025_float", SHIPPED, (6, 18), 0, 1025, 31, "float", "stages=0 aligned=0 6+18 nyquist=0; an odd hop above the frame: every frame unaligned, position-independent")
_row("stages_hop333", SHIPPED, (6, 18), 0, 333, 32, "stages", "stages=1 aligned=0 6+18 nyquist=0; host stages at an odd hop below the frame")
_row("stages_dev", SHIPPED, (6, 18), 0, 1024, 32, "dev_stages", "stages=1 aligned=1 6+18 nyquist=0; device stages")
# non-power-of-two scales on the shipped edges
_row("scale1000", S1000, (6, 18), 0, 512, 13, "host", "stages=0 aligned=1 6+18 nyquist=0; scale 1000: the compiler's division")
_row("scale32767", S32767, (6, 18), 0, 1024, 32, "dev", "stages=0 aligned=1 6+18 nyquist=0; the largest scale: band sums wrap, a negative sum is divided")
# 8+24, no tap on bin 512
_row("wide", WIDE, (8, 24), 0, 1024, 13, "dev", "stages=0 aligned=1 8+24 nyquist=0; the wide shape, the largest count", big=True)
_row("wide_odd_hop", WIDE, (8, 24), 0, 1025, 32, "host", "stages=0 aligned=0 8+24 nyquist=0; the wide shape unaligned")
_row("wide_stages", WIDE, (8, 24), 0, 1024, 32, "dev_stages", "stages=1 aligned=1 8+24 nyquist=0; the wide shape with stages")
_row("wide_stages_odd", WIDE, (8, 24), 0, 333, 32, "dev_stages_odd", "stages=1 aligned=0 8+24 nyquist=0; the wide shape with stages, odd pointer and odd hop")
# 6+18 with a tap on bin 512
_row("nyq", NYQ, (6, 18), 1, 1024, 32, "dev", "stages=0 aligned=1 6+18 nyquist=1; the Nyquist bin in the product instance, the largest count", big=True)
_row("nyq_64", NYQ_64, (6, 18), 1, 333, 13, "host", "stages=0 aligned=0 6+18 nyquist=1; the Nyquist bin with scale 64 at an odd hop")
_row("nyq_stages", NYQ, (6, 18), 1, 512, 32, "dev_stages_odd", "stages=1 aligned=0 6+18 nyquist=1; stages with a non-zero tap on bin 512, odd pointer")
_row("nyq_stages_host", NYQ_64, (6, 18), 1, 1024, 32, "stages", "stages=1 aligned=1 6+18 nyquist=1; host stages with a non-zero tap on bin 512")
# 8+24 with a tap on bin 512
_row("nyq_wide", NYQ_WIDE, (8, 24), 1, 1024, 32, "dev_odd", "stages=0 aligned=0 8+24 nyquist=1; the wide shape with the Nyquist bin from an odd pointer, the largest count", big=True)
_row("nyq_wide_1000", NYQ_WIDE_1000, (8, 24), 1, 1025, 31, "dev", "stages=0 aligned=0 8+24 nyquist=1; a non-power-of-two scale with the wide shape and the Nyquist bin")
_row("nyq_wide_lo", NYQ_WIDE_LO, (8, 24), 1, 1024, 1, "float", "stages=0 aligned=1 8+24 nyquist=1; the other wide filterbank that reaches bin 512, float output, one coefficient")
_row("nyq_wide_stages", NYQ_WIDE_LO, (8, 24), 1, 1024, 32, "stages", "stages=1 aligned=1 8+24 nyquist=1; host stages, wide shape, non-zero tap on bin 512")

TABLE = dict(shape_nyquist=((6, 18, 0), (8, 24, 0), (6, 18, 1), (8, 24, 1)), scale=(128, 64, 1000, 32767), nyquist_scale=("not a power of two",),
             wide_scale=("not a power of two",), hop=("0", "1", "odd below", "half", "whole", "odd above"), n_coef=(1, 13, 31, 32), entry=ENTRIES,
             instance=tuple((s, a, nlo, nhi) for s in (0, 1) for a in (0, 1) for nlo, nhi in ((6, 18), (8, 24))))


def pow2(v):
    return v > 0 and v & (v - 1) == 0


def row_items(row):
    """What a row covers of TABLE"""
    hop, scale = row["hop"], row["fb"][3]
    out = {("shape_nyquist", row["shape"] + (row["nyquist"],)), ("scale", scale), ("n_coef", row["n_coef"]), ("entry", row["entry"]),
           ("instance", instance(row))}
    if row["nyquist"] and not pow2(scale):
        out.add(("nyquist_scale", "not a power of two"))
    if row["shape"] == (8, 24) and not pow2(scale):
        out.add(("wide_scale", "not a power of two"))
    for tag, hit in (("0", hop == 0), ("1", hop == 1), ("odd below", 1 < hop < FRAME_LEN and hop % 2), ("half", hop == FRAME_LEN // 2),
                     ("whole", hop == FRAME_LEN), ("odd above", hop > FRAME_LEN and hop % 2)):
        if hit:
            out.add(("hop", tag))
    return out


def full_items():
    return {(k, v) for k, vs in TABLE.items() for v in vs}


# ---- the launch code, restated --------------------------------------------------------------------------------------------------------
def _src():
    return open(os.path.join(CSRC, "mfcc_q15_kernels.hip")).read()


def eq_wpb():
    """EQ_WPB of the product build: waves per workgroup"""
    return int(re.search(r"#ifndef EQ_WPB\s*\n#define EQ_WPB (\d+)", _src()).group(1))


def eq_nb():
    """EQ_NB: mel rows a wave parks before it runs their DCT stage"""
    return int(re.search(r"^#define EQ_NB (\d+)", _src(), re.M).group(1))


def eq_buf():
    return int(re.search(r"^#define EQ_BUF (\d+)", _src(), re.M).group(1))


def pairs(n):
    """ED_Q15_PAIRS"""
    return (n + 2) // 2


def lds_bytes(shape):
    """sizeof(u32) * EQ_LDS_DWORDS(ED_Q15_PAIRS(NLO), ED_Q15_PAIRS(NHI))"""
    w, nb = eq_wpb(), eq_nb()
    tw = (2 * 4 + 1) * 6 * 64
    return 4 * ((pairs(shape[0]) + pairs(shape[1])) * 64 + 1024 + tw + w * (eq_buf() + nb * 32 + nb * 16 + nb) + 4)


def blocks_per_cu(shape):
    """Resident workgroups per CU. The source asks the runtime's occupancy calculator (ed_kernel_prepare) and lets the integer in the
    environment variable ED_Q15_BLOCKS_PER_CU only LOWER the answer (a value outside 1 .. computed is ignored); with more than half of
    a CU's LDS per workgroup the answer is 1, which nothing can lower, so the grid is blocks() whatever the environment says."""
    return max(1, CU_LDS_BYTES // lds_bytes(shape))


def blocks(n, n_cu, shape=(6, 18)):
    return min((n + eq_wpb() - 1) // eq_wpb(), n_cu * blocks_per_cu(shape))


def split(n, n_cu, shape=(6, 18)):
    """[(s0, cnt)] per workgroup: its slice of the launch's frames"""
    g = blocks(n, n_cu, shape)
    return [(b * n // g, (b + 1) * n // g - b * n // g) for b in range(g)]


def aligned(ptr_offset, hop, group_stride=0):
    """ed_launch_q15_shape's choice; ptr_offset in samples from a 4-byte aligned address"""
    return (2 * ptr_offset) % 4 == 0 and hop % 2 == 0 and group_stride % 2 == 0


def ptr_offset(row):
    """Sample offset of the first frame from the start of its (aligned) allocation"""
    return 1 if row["entry"].endswith("_odd") else 0


def instance(row):
    """(STAGES, ALIGNED, NLO, NHI) of the kernel that runs the row"""
    return (int(row["entry"] in STAGE_ENTRIES), int(aligned(ptr_offset(row), row["hop"])),) + tuple(row["shape"])


def note_instance(note):
    m = re.match(r"stages=([01]) aligned=([01]) (\d+)\+(\d+) nyquist=([01]); ", note)
    return tuple(int(v) for v in m.groups())


CASES = ("one frame", "one workgroup, waves without a frame", "one workgroup, one frame per wave", "several workgroups, uneven slices",
         "second frame by position", "first queue draws", "at least three draws per wave", "a wave parks 16 frames and goes on",
         "last batch partial")
BIG_CASE = "a wave parks 16 frames and goes on"


def cases(row, n, n_cu):
    """What a frame count does to the kernel, as tags"""
    w, nb = eq_wpb(), eq_nb()
    s = split(n, n_cu, row["shape"])
    cnts = [c for _, c in s]
    out = set()
    if n == 1:
        out.add("one frame")
    if len(s) == 1 and n < w:
        out.add("one workgroup, waves without a frame")
    if len(s) == 1 and n == w:
        out.add("one workgroup, one frame per wave")
    if len(s) > 1 and len(set(cnts)) > 1:
        out.add("several workgroups, uneven slices")
    if any(w < c <= 2 * w for c in cnts):
        out.add("second frame by position")
    if any(c > 2 * w for c in cnts):
        out.add("first queue draws")                    # the counter starts at 2 EQ_WPB
    if min(cnts) >= 5 * w:
        out.add("at least three draws per wave")        # on average: which wave draws is the queue's business
    if min(cnts) >= w * nb + 1:
        out.add(BIG_CASE)                               # pigeonhole: some wave of EVERY workgroup holds EQ_NB + 1 frames or more
    if any(c % (w * nb) for c in cnts):
        out.add("last batch partial")                   # some wave's frame count is no multiple of EQ_NB
    return out


def counts(row, n_cu):
    """The frame counts row `row` runs on a device of n_cu compute units. Every row reaches every case but BIG_CASE; the rows marked big
    (one per shape x Nyquist, device entry, hop 0 or >= 1024) add the count that reaches it."""
    w, nb = eq_wpb(), eq_nb()
    out = {1, 2, w - 1, w, w + 1, 2 * w + 1, w * n_cu - 1, w * n_cu + 1, 2 * w * n_cu + 1, 5 * w * n_cu + 7}
    if row["big"]:
        out.add((w * nb + 1) * n_cu + 3)
    return sorted(out)


def whole(row):
    """Frames do not overlap: every frame of a call is a base frame, compared with the bits of the 64-frame call"""
    return row["hop"] >= FRAME_LEN or row["hop"] == 0


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
KINDS = dict(zero=0, rail_pos=1, rail_neg=2, square=3, impulse=4, nyq0=5, chirp0=20, hop0=50)
N_NYQ, N_TONE, N_CHIRP, N_QUIET = 10, 5, 3, 4


def top_band_bins(fb):
    """(first, last) bin the chirps sweep: the top band of the filterbank (mel edges 31 .. 33 of 34, mfcc_utils.py:43-60), a few bins
    inside it, where the sum of its magnitudes is largest"""
    mel = lambda f: 1127.0 * np.log1p(f / 700.0)
    lo = 700.0 * np.expm1((mel(fb[1]) + (mel(fb[2]) - mel(fb[1])) * 31.0 / 33.0) / 1127.0)
    first, last = int(np.ceil(lo / fb[0] * FRAME_LEN)), min(FRAME_LEN // 2, int(fb[2] / fb[0] * FRAME_LEN))
    return first + 8, last - 4


def _speechlike(rng, n, N):
    """noise with the long-term tilt of speech: white noise through y[i] = 0.9 y[i-1] + x[i], unit rms"""
    x = rng.normal(0, 1, (n, N + 64))
    y = np.zeros_like(x)
    for i in range(1, N + 64):
        y[:, i] = 0.9 * y[:, i - 1] + x[:, i]
    y = y[:, 64:]
    return y / np.sqrt((y * y).mean(axis=1, keepdims=True))


_BASE = {}


def base_frames(row):
    """([64, 1024] int16, position of every special frame): 0 silence, 1 / 2 the rails, 3 a square wave at fs / 2 between the rails, 4 one
    full-scale impulse in mid-frame, 5 .. 14 a tone exactly on bin 512 (30000 down to 3000) with weaker tones on bins 509 .. 511,
    15 .. 19 tones on bin centres (two over a noise floor), 20 .. 22 constant-envelope chirps across the top band (between the rails, a
    full-scale cosine, a weaker one),
    23 .. 26 speech-like noise of 0.3 .. 30 LSB rms -- below the transform's 1 / 1024: the output is zero or nearly so --, 27 .. 63
    speech-like noise from 100 LSB rms to clipping; then shuffled. Seeded per filterbank."""
    if row["fb"] in _BASE:
        return _BASE[row["fb"]]
    N = FRAME_LEN
    rng = np.random.default_rng(5000 + int(row["fb"][1]) + int(row["fb"][2]) + row["fb"][3])
    t = np.arange(N)
    f = np.zeros((N_BASE, N))
    f[1], f[2] = 32767, -32768
    f[3] = np.where(t & 1, -32768, 32767)
    f[4, N // 2] = 32767
    at = 5
    for j, amp in enumerate((30000.0, 25000.0, 20000.0, 16000.0, 12000.0, 10000.0, 8000.0, 6000.0, 4000.0, 3000.0)):
        f[at + j] = amp * np.cos(np.pi * t)
        for k in (509, 510, 511):
            f[at + j] += rng.uniform(0.02, 0.1) * amp * np.cos(2 * np.pi * k * t / N + rng.uniform(0, 2 * np.pi))
    at += N_NYQ
    floor = _speechlike(rng, 2, N)
    for j, (k, amp) in enumerate(((64, 30000.0), (129, 300.0), (204, 8000.0), (254, 1000.0), (400, 20000.0))):
        f[at + j] = amp * np.cos(2 * np.pi * k * t / N + rng.uniform(0, 2 * np.pi))
        if j in (2, 3):
            f[at + j] += 0.05 * amp * floor[j - 2]
    at += N_TONE
    k0, k1 = top_band_bins(row["fb"])
    for j, amp in enumerate((1e9, 32767.0, 20000.0)):                  # 1e9: clipped to a chirp between the rails
        phase = 2 * np.pi * (k0 * t + (k1 - k0) * t * t / (2.0 * N)) / N
        f[at + j] = amp * np.cos(phase + rng.uniform(0, 2 * np.pi))
    at += N_CHIRP
    f[at:at + N_QUIET] = _speechlike(rng, N_QUIET, N) * (0.3 * 10.0 ** (2.0 * np.arange(N_QUIET) / (N_QUIET - 1)))[:, None]
    at += N_QUIET
    n = N_BASE - at
    f[at:] = _speechlike(rng, n, N) * (100.0 * 10.0 ** (2.5 * np.arange(n) / (n - 1)))[:, None]
    x = np.clip(np.rint(f), -32768, 32767).astype(np.int16)
    perm = rng.permutation(N_BASE)
    where = {k: int(np.nonzero(perm == v)[0][0]) for k, v in KINDS.items()}
    _BASE[row["fb"]] = (x[perm], where)
    return _BASE[row["fb"]]


def tile_index(n):
    """Base frame of frame slot i: neighbours and positions vary from one repetition of the set to the next"""
    i = np.arange(n)
    return (i + i // N_BASE) % N_BASE


def audio(row, n, base=None):
    """(int16 stream, idx): n frames at the row's hop. hop >= 1024: frame slot i is exactly base[idx[i]] (idx from tile_index), the gaps
    hold filler; 0 < hop < 1024: the base frames idx[0], idx[1], ... back to back, cut every hop samples (idx[i] is then only the frame
    the cut starts in); hop 0: the base frame KINDS calls hop0, alone."""
    N, hop = FRAME_LEN, row["hop"]
    where = base_frames(row)[1]
    if base is None:
        base = base_frames(row)[0]
    if hop == 0:
        return base[where["hop0"]].copy(), np.full(n, where["hop0"])
    idx = tile_index(n)
    if hop >= N:
        x = np.full((n, hop), 12345, np.int16)
        x[:, :N] = base[idx]
        return x.reshape(-1)[:(n - 1) * hop + N].copy(), idx
    total = (n - 1) * hop + N
    k = -(-total // N)
    return base[tile_index(k)].reshape(-1)[:total].copy(), tile_index(k)[(np.arange(n) * hop) // N]


def kws_n_utt(n_cu):
    """Utterance counts of the KWS test: 31 n frames in one group per utterance"""
    w = eq_wpb()
    return sorted({1, 3, -(-(w * n_cu + 1) // UTT_FRAMES), -(-(2 * w * n_cu + 1) // UTT_FRAMES)})


# ---- the tables the host library builds ----------------------------------------------------------------------------------------------
_PAIRS_MAX = pairs(8) + pairs(24)


class Q15Tables(ctypes.Structure):
    """ed_q15_tables_t (edison_amd/csrc/edison_internal.h), for the tests that read what ed_build_q15_tables hands the kernel"""
    _fields_ = [("tw1024", ctypes.c_uint32 * 768), ("tw1024x", ctypes.c_uint32 * 768), ("tw16", ctypes.c_uint32 * 12), ("tw16x", ctypes.c_uint32 * 12),
                ("rfa", ctypes.c_uint32 * 16), ("rfb", ctypes.c_uint32 * 16), ("mel_tap", (ctypes.c_int32 * 64) * 32),
                ("mel_lo_bin", ctypes.c_int32 * 64), ("mel_hi_bin", ctypes.c_int32 * 64), ("mel_tap2", (ctypes.c_uint32 * 64) * _PAIRS_MAX),
                ("mel_lo_pair", ctypes.c_int32 * 64), ("mel_hi_pair", ctypes.c_int32 * 64), ("mel_nlo", ctypes.c_int32), ("mel_nhi", ctypes.c_int32),
                ("mel_scale", ctypes.c_int32), ("n_mel_coef", ctypes.c_int32), ("need_nyquist", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("sqbit", ctypes.c_uint32 * 1024)]


def host_tables(lib, fb):
    """(return code, Q15Tables, message) of ed_build_q15_tables for filterbank fb"""
    lib.ed_build_q15_tables.restype = ctypes.c_int
    lib.ed_build_q15_tables.argtypes = [ctypes.c_double] * 4 + [ctypes.POINTER(Q15Tables), ctypes.c_char_p, ctypes.c_size_t]
    t = Q15Tables()
    err = ctypes.create_string_buffer(200)
    r = lib.ed_build_q15_tables(float(fb[0]), float(fb[1]), float(fb[2]), float(fb[3]), ctypes.byref(t), err, 200)
    return r, t, err.value.decode()


def host_weights(t):
    """The compact mel matrix as the kernel's lanes hold it, summed back to [32 bands, 513 bins]"""
    W = np.zeros((NUM_MEL, FRAME_LEN // 2 + 1), np.int64)
    tap = np.array(t.mel_tap)
    lo, hi = np.array(t.mel_lo_bin), np.array(t.mel_hi_bin)
    for l in range(64):
        b = l & 15
        for part, (m, first, n, row0) in enumerate(((b, lo[l], t.mel_nlo, 0), (31 - b, hi[l], t.mel_nhi, t.mel_nlo))):
            for k in range(n):
                W[m, first + k] += tap[row0 + k, l]
    return W


def packed_weights(t):
    """The same matrix from the form the kernel reads: mel_tap2 (two taps per dword against the int16 spectrum pairs from
    mel_lo_pair / mel_hi_pair on); [32 bands, 514]: column 513 is the pad halfword of the last pair, which must stay 0"""
    W = np.zeros((NUM_MEL, FRAME_LEN // 2 + 2), np.int64)
    tap2 = np.array(t.mel_tap2, dtype=np.uint32)
    lo, hi = np.array(t.mel_lo_pair), np.array(t.mel_hi_pair)
    nlop = pairs(t.mel_nlo)
    for l in range(64):
        b = l & 15
        for m, first, n, row0 in ((b, lo[l], nlop, 0), (31 - b, hi[l], pairs(t.mel_nhi), nlop)):
            for k in range(n):
                v = int(tap2[row0 + k, l])
                for h in (0, 1):
                    c = (v >> (16 * h)) & 0xffff
                    W[m, 2 * (first + k) + h] += c - 65536 if c >= 32768 else c
    return W


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
_ORACLE_TABLES = {}


def oracle_tables(fb):
    if fb not in _ORACLE_TABLES:
        from oracle import oracle
        _ORACLE_TABLES[fb] = oracle.Q15Tables(sample_rate=fb[0], lower_edge_hertz=fb[1], upper_edge_hertz=fb[2], mel_mtx_scale=fb[3])
    return _ORACLE_TABLES[fb]


def oracle_weights(fb):
    """melMtxCompact of the oracle as [32 bands, 513 bins] int64"""
    a = oracle_tables(fb).arrays()
    W = np.zeros((NUM_MEL, FRAME_LEN // 2 + 1), np.int64)
    pos = 0
    for m in range(NUM_MEL):
        s, c = int(a["mel_start"][m]), int(a["mel_count"][m])
        W[m, s:s + c] = a["mel_coef"][pos:pos + c]
        pos += c
    assert pos == a["mel_coef"].size
    return W


def oracle_outputs(row, x, n, stages=False, hop=None, n_threads=8):
    """oracle.mfcc_q15 on the row's filterbank: int16 [n, 32], and with stages dict(fft [n, 513, 2], spectrogram, mel_spectrogram)"""
    from oracle import oracle
    r = oracle.mfcc_q15(x, n_frames=n, frame_step=row["hop"] if hop is None else hop, stages=stages, n_threads=n_threads, tables=oracle_tables(row["fb"]))
    if stages:
        r[1]["fft"] = np.ascontiguousarray(r[1]["fft"][:, :513])
    return r


def net_input(mfcc, n_coef):
    from oracle import oracle
    return oracle.net_input_q15(mfcc, n_coef=n_coef)


def band_sums(fb, spec):
    """The 32-bit band sums of audioprocessing.c:158-172 from a spectrogram [n, 513] and the oracle's compact matrix: (exact int64 sums,
    the same wrapped to int32 as the MCU's accumulator holds them)"""
    acc = spec.astype(np.int64) @ oracle_weights(fb).T
    return acc, ((acc + 2 ** 31) % 2 ** 32 - 2 ** 31)


def trunc_div(acc, scale):
    """C's division of the wrapped sum, cast to q15"""
    q = np.sign(acc) * (np.abs(acc) // scale)
    return ((q + 2 ** 15) % 2 ** 16 - 2 ** 15).astype(np.int16)

"""What tests/test_lds_layout.py and tests/golden/gen_fixtures_mel_terms.py share: the fast MFCC kernel's mel tables read the way
its loop reads them (ed_mfcc2_body, stage 5), as the list of (bin, weight) terms every accumulator takes, in order."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMS_FIXTURE = os.path.join(ROOT, "tests", "golden", "mel_terms_parent.json")
SHAPES = {"2+5": False, "3+6": True}  # table shape -> EDISON_FORCE_WIDE_MEL


def layout_constants():
    """the ED2_* layout constants of edison_internal.h"""
    text = open(os.path.join(ROOT, "edison_amd", "csrc", "edison_internal.h")).read()
    out = {}
    for name in ("ED2_T2_STRIDE", "ED2_S_OFF", "ED2_L_OFF", "ED2_XBUF_FLOATS"):
        out[name] = int(re.search(r"#define %s (\d+)" % name, text).group(1))
    return out


def build_tables(lib, variant, wide, sample_rate=16000.0, lower_edge_hertz=80.0, upper_edge_hertz=7600.0):
    """(slo4, shi4, band, half, w4[nlo + nhi][64][4] as uint32 bit patterns, nlo, nhi) of one variant and table shape (wide: the 3+6
    shape forced; a filterbank that needs it gets it either way), for the shipped filterbank or the one given"""
    lib.ed_build_mfcc_tables.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    buf, err = (ctypes.c_char * 65536)(), ctypes.create_string_buffer(256)
    old = os.environ.pop("EDISON_FORCE_WIDE_MEL", None)
    if wide:
        os.environ["EDISON_FORCE_WIDE_MEL"] = "1"
    try:
        assert lib.ed_build_mfcc_tables(variant, float(sample_rate), float(lower_edge_hertz), float(upper_edge_hertz), 128.0, buf, err, 256) == 0, err.value
    finally:
        os.environ.pop("EDISON_FORCE_WIDE_MEL", None)
        if old is not None:
            os.environ["EDISON_FORCE_WIDE_MEL"] = old
    i32 = np.frombuffer(buf, dtype=np.int32).copy()
    u32 = np.frombuffer(buf, dtype=np.uint32).copy()
    o = 2 * 8 * 64 * 2                                            # tw1, tw2
    slo, shi, band, half = (i32[o + 64 * k:o + 64 * (k + 1)] for k in range(4))
    o += 4 * 64 + 2 * 64 * 4 + 4 * 64 * 2                         # + dct4, twp
    nlo, nhi = int(i32[o + 9 * 64 * 4]), int(i32[o + 9 * 64 * 4 + 1])
    w4 = u32[o:o + 9 * 64 * 4].reshape(9, 64, 4)[:nlo + nhi]
    return slo, shi, band, half, w4, nlo, nhi, buf


def mel_terms(slo, shi, band, half, w4, nlo, nhi):
    """{"b<band>r<row>": {"lo0": [[bin, weight bits], ...], "lo1", "hi0", "hi1"}}: the products each of the loop's four accumulators
    adds, in the loop's order, for the lane that serves quarter `row` of band pair (band, 31 - band); products with a zero weight
    (+0.0 exactly: magnitudes are finite and non-negative) are left out. Per t the lane reads slot 2 q + half, then slot
    2 q + 1 - half (a slot = bins 2 s, 2 s + 1 of both frames); a slot's first bin goes to accumulator 0, its second to 1."""
    out = {}
    for lane in range(64):
        acc = {"lo0": [], "lo1": [], "hi0": [], "hi1": []}
        for part, first, n, base in (("lo", int(slo[lane]), nlo, 0), ("hi", int(shi[lane]), nhi, nlo)):
            for t in range(n):
                for slot_half in (int(half[lane]), 1 - int(half[lane])):
                    for c in range(2):
                        k = 4 * (first + t) + 2 * slot_half + c
                        w = int(w4[base + t, lane, 2 * slot_half + c])
                        if w & 0x7fffffff:
                            acc[part + str(c)].append([k, w])
        key = "b%dr%d" % (int(band[lane]), lane >> 4)
        assert key not in out
        out[key] = acc
    return out

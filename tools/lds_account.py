#!/usr/bin/env python3
"""The account of the fast MFCC loop's LDS accesses (ed_mfcc2_body, one frame pair): per instruction group, the conflict-free
passes and the extra ones (bank conflicts), from the model in edison_amd/csrc/tables.c (ed_mfcc2_lds_account) on the tables the
library builds. No GPU needed.  usage: tools/lds_account.py > profiles/r06_mfcc_lds_account.txt"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edison_amd import _lib

ROWS_MAX = 16
T2_STRIDE_BEFORE, T2_STRIDE = 66, 65  # transpose 2's slot stride up to round 5 / ED2_T2_STRIDE (edison_internal.h)


class Row(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("kind", ctypes.c_int32), ("instructions", ctypes.c_int32),
                ("free_passes", ctypes.c_int32), ("extra_passes", ctypes.c_int32)]


def account(lib, wide, t2_stride, wave=0, variant=_lib.MFCC_B):
    """[(name, instructions, free passes, extra passes)] of one loop iteration; wide: the 3+6 table shape (EDISON_FORCE_WIDE_MEL=1)"""
    lib.ed_build_mfcc_tables.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    lib.ed_mfcc2_lds_account.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Row), ctypes.c_int]
    buf, err = (ctypes.c_char * 65536)(), ctypes.create_string_buffer(256)
    old = os.environ.pop("EDISON_FORCE_WIDE_MEL", None)
    if wide:
        os.environ["EDISON_FORCE_WIDE_MEL"] = "1"
    try:
        assert lib.ed_build_mfcc_tables(variant, 16000.0, 80.0, 7600.0, 128.0, buf, err, 256) == _lib.OK, err.value
    finally:
        os.environ.pop("EDISON_FORCE_WIDE_MEL", None)
        if old is not None:
            os.environ["EDISON_FORCE_WIDE_MEL"] = old
    rows = (Row * ROWS_MAX)()
    n = lib.ed_mfcc2_lds_account(buf, t2_stride, wave, rows, ROWS_MAX)
    assert n > 0, n
    return [(r.name.decode(), r.instructions, r.free_passes, r.extra_passes) for r in rows[:n]]


def main():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    print("# LDS accesses of one iteration (one frame pair, one wave) of ed_mfcc2_body, modelled on the host: tools/lds_account.py")
    print("# (ed_mfcc2_lds_account in edison_amd/csrc/tables.c; 16 kHz, 80-7600 Hz filterbank). passes = LDS-array cycles; extra = bank conflicts")
    print("# (what SQ_LDS_BANK_CONFLICT counts). ds_bpermute_b32 (16 per pair) uses the crossbar, not the banks, and is not modelled.")
    print("# The round-3 counters (profiles/r03_mfcc_sq_counters.txt) give 3 997 696 conflict cycles per launch of 32 768 pairs = 122.0 per pair.")
    for wide in (False, True):
        for stride in (T2_STRIDE_BEFORE, T2_STRIDE):
            rows = account(lib, wide, stride)
            assert all(account(lib, wide, stride, w) == rows for w in range(1, 12)), "the account is the same for every wave of the workgroup"
            print("\n## table shape %s, transpose-2 stride %d slots%s" % ("3+6 (EDISON_FORCE_WIDE_MEL=1)" if wide else "2+5 (shipped)", stride,
                                                                  " (rounds 1-5)" if stride == T2_STRIDE_BEFORE else " (ED2_T2_STRIDE, this kernel)"))
            print("%-92s %5s %6s %6s" % ("instruction group", "insts", "free", "extra"))
            for name, insts, free, extra in rows:
                print("%-92s %5d %6d %6d" % (name, insts, free, extra))
            print("%-92s %5d %6d %6d" % ("total", sum(r[1] for r in rows), sum(r[2] for r in rows), sum(r[3] for r in rows)))


if __name__ == "__main__":
    main()

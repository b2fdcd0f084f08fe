#!/usr/bin/env python3
"""mel_terms_parent.json: the (bin, weight) products every accumulator of the fast MFCC kernel's mel stage adds, in order, read
from the tables of the library this is run against -- run it on the commit whose sums a later table layout has to reproduce bit
for bit (tests/test_lds_layout.py compares the current tables' terms with these). Generated at the commit before the LDS layout
work of round 6 (transpose-2 stride 65).  usage: EDISON_LIB=<that commit's libedison_hip.so> tests/golden/gen_fixtures_mel_terms.py"""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from edison_amd import _lib
import lds_layout as L  # noqa: E402

lib = ctypes.CDLL(_lib.LIB_PATH)
out = {}
for vname, variant in (("A", _lib.MFCC_A), ("B", _lib.MFCC_B)):
    for shape, wide in L.SHAPES.items():
        out["%s %s" % (vname, shape)] = L.mel_terms(*L.build_tables(lib, variant, wide)[:7])
json.dump(out, open(L.TERMS_FIXTURE, "w"), separators=(",", ":"), sort_keys=True)
print(L.TERMS_FIXTURE, os.path.getsize(L.TERMS_FIXTURE), "bytes")

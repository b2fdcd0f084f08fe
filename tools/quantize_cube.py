#!/usr/bin/env python3
"""Command-line front end of edison_amd/kws/kws_quantize.py: a float32 network (.ednf) and a calibration set -> an int8 NNoM graph.

Usage:  tools/quantize_cube.py <net.ednf> <audio.npy> <out.ednn> [--weights-h <out.h>] [--saturate <share>] [--geometry k=v,...] [--chunk N]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edison_amd.kws.kws_quantize import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main(["quantize"] + sys.argv[1:]))

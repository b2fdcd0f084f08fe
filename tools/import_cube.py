#!/usr/bin/env python3
"""Command-line front end of edison_amd/cube_import.py: X-CUBE-AI <net>.c + <net>_data.c -> .ednf float network blob.

Usage:  tools/import_cube.py <net>.c <net>_data.c out.ednf [keywords.txt]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edison_amd.cube_import import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main(sys.argv))

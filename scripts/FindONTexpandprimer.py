#!/usr/bin/env python3
"""Which expanded primer produced each read end of an amplicon sequencing run, on the GPU: the reference's FindONTexpandprimer.py with the
same flags and defaults (-p 1, -m 0.8, the full "ID | j" label as the name) — see multiprime_amd/ontprimer.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiprime_amd.ontprimer import expand_main  # noqa: E402

if __name__ == "__main__":
    expand_main()

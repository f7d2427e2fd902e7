#!/usr/bin/env python3
"""Trimming an alignment for run_dege.py with the flags and the output bytes of DEGEPRIME-1.1.0/TrimAlignment.pl — see
multiprime_amd/degeprime.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiprime_amd.degeprime import trim_main  # noqa: E402

if __name__ == "__main__":
    trim_main()

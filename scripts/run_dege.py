#!/usr/bin/env python3
"""DegePrime on the GPU with the reference wrapper's name and flags (scripts/run_dege.py, which calls DEGEPRIME-1.1.0/DegePrime.pl) — see
multiprime_amd/degeprime.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiprime_amd.degeprime import main  # noqa: E402

if __name__ == "__main__":
    main()

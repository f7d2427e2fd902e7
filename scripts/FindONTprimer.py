#!/usr/bin/env python3
"""Which primer pair produced each read of an amplicon sequencing run, on the GPU: the reference's FindONTprimerV3.py with the same flags
and defaults — see multiprime_amd/ontprimer.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiprime_amd.ontprimer import main  # noqa: E402

if __name__ == "__main__":
    main()

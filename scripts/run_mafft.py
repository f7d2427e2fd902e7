#!/usr/bin/env python3
"""Star alignment: align the unaligned sequences of a cluster from nothing on the GPU, every base kept (the `mafft --auto` step of
the workflow's rule alignment_and_info_extraction: -i X.tfa -o X.tmsa) — see multiprime_amd/starmsa.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiprime_amd.starmsa import main  # noqa: E402

if __name__ == "__main__":
    main()

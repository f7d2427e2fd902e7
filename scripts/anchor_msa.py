#!/usr/bin/env python3
"""Anchored alignment: add the unaligned sequences of a cluster to its seed alignment on the GPU, keeping the seed's width (the
`mafft --addfragments --keeplength` step) — see multiprime_amd/anchor.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiprime_amd.anchor import main  # noqa: E402

if __name__ == "__main__":
    main()

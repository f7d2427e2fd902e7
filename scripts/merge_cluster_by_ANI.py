#!/usr/bin/env python3
"""Merging rare clusters by average nucleotide identity on the GPU: the pipeline's merge_cluster_by_ANI.py step without fastANI, on the
tree extract_cluster.py leaves — see multiprime_amd/animerge.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiprime_amd.animerge import main  # noqa: E402

if __name__ == "__main__":
    main()

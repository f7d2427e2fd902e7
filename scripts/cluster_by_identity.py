#!/usr/bin/env python3
"""Clustering by identity on the GPU: the pipeline's `cd-hit -c 1` and `cd-hit -c <identity>` steps, with cd-hit's .clstr layout for
extract_cluster.py — see multiprime_amd/cluster.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiprime_amd.cluster import main  # noqa: E402

if __name__ == "__main__":
    main()

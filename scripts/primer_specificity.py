#!/usr/bin/env python3
"""Drop-in entry point with the reference script's name and flags (scripts/primer_specificity.py): the bowtie2 + samtools mapping
step and the pairing of the sites are one GPU pass that returns PCR products — see multiprime_amd/specificity.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiprime_amd.specificity import main  # noqa: E402

if __name__ == "__main__":
    main()

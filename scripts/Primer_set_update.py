#!/usr/bin/env python3
"""Drop-in for the reference's scripts/Primer_set_update.py (same flags -c -n -r -s -l -m -p -f -o, same four output files): new primers
against a core set — the cross-set 3'-end dimer search and the three off-target joins run on an MI355X (multiprime_amd/panel.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    from multiprime_amd.panel import main as panel_main
    panel_main(argv)


if __name__ == "__main__":
    main()

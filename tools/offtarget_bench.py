#!/usr/bin/env python3
"""The off-target screen (scripts/primer_specificity.py) at scale: the device path (mp_offtarget_resident: scan, site reduction and
join on the GPU) against the host path (validate.py's scan with its hits copied back, sorted and put into dicts, then amplicons() per
sequence), on synthetic backgrounds of --bases bases (multiprime_amd.synth.offtarget_case) with 3' terms of --terms bases.  Per size
and term length: the device stages (event times), the whole run() of each path, hits / sites / products, and whether the two paths
wrote the same three files.  One JSON line per measurement on stdout.

    python tools/offtarget_bench.py --bases 1e8 1e9 --terms 9 18

--gaps: every device run is followed by one under the gapped rule (validate.py: `--gaps`) on the same input, alternating; the record
then carries both (`device`, `device_gaps`), the scan time of every run (`scan_ms`, `scan_ms_gaps`) and, with the host path, whether
the gapped files agree too (`equal_gaps`).
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def files(out):
    return [open(out + s, "rb").read() for s in ("", ".pair.num", ".total.acc.num")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, nargs="+", default=[1e8, 1e9])
    ap.add_argument("--terms", type=int, nargs="+", default=[9, 18])
    ap.add_argument("--row-len", type=int, default=1_000_000)
    ap.add_argument("--primers", type=int, default=8)
    ap.add_argument("--degenerate", type=int, default=2, help="N per primer term (besides one R): 2 * 4^n reads per primer")
    ap.add_argument("--size", default="100,1500")
    ap.add_argument("--repeat", type=int, default=2, help="device runs per point (the first warms the process up)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--gaps", action="store_true", help="measure the gapped rule beside the ungapped one, alternating runs")
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process: torch's, as in the GPU suite)
    from multiprime_amd._abi import Library
    from multiprime_amd.specificity import off_targets
    from multiprime_amd.synth import offtarget_case
    lib = Library()
    import io
    import contextlib
    for bases in a.bases:
        n_rows = max(1, int(bases) // a.row_len)
        with tempfile.TemporaryDirectory() as td:
            t0 = time.time()
            pf, bf = offtarget_case(td, n_rows, a.row_len, a.primers, 3, n_degenerate=a.degenerate)
            made = time.time() - t0
            for term in a.terms:
                rec = {"bases": n_rows * a.row_len, "rows": n_rows, "term": term, "size": a.size, "primers": a.primers, "make_input_s": round(made, 2)}
                scan_ms = {False: [], True: []}
                for rep in range(a.repeat):
                    for gaps in (False, True) if a.gaps else (False,):
                        app = off_targets(primer_file=pf, term_length=term, reference_file=bf, PCR_product_size=a.size,
                                          outfile=os.path.join(td, "gap.out" if gaps else "dev.out"), library=lib, join="device", gaps=gaps)
                        with contextlib.redirect_stdout(io.StringIO()):
                            app.run()
                        scan_ms[gaps].append(round(app.stats["scan_ms"], 3))
                        rec["device_gaps" if gaps else "device"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in app.stats.items()}
                rec["scan_ms"] = scan_ms[False]
                if a.gaps:
                    rec["scan_ms_gaps"] = scan_ms[True]
                if not a.no_host:
                    host = off_targets(primer_file=pf, term_length=term, reference_file=bf, PCR_product_size=a.size, outfile=os.path.join(td, "host.out"),
                                       library=lib, join="host")
                    with contextlib.redirect_stdout(io.StringIO()):
                        host.run()
                    rec["host"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in host.stats.items()}
                    rec["equal"] = files(os.path.join(td, "dev.out")) == files(os.path.join(td, "host.out"))
                    if a.gaps:
                        host = off_targets(primer_file=pf, term_length=term, reference_file=bf, PCR_product_size=a.size,
                                           outfile=os.path.join(td, "hostgap.out"), library=lib, join="host", gaps=True)
                        with contextlib.redirect_stdout(io.StringIO()):
                            host.run()
                        rec["equal_gaps"] = files(os.path.join(td, "gap.out")) == files(os.path.join(td, "hostgap.out"))
                print(json.dumps(rec), flush=True)
                if not (rec.get("equal", True) and rec.get("equal_gaps", True)):
                    sys.exit(1)


if __name__ == "__main__":
    main()

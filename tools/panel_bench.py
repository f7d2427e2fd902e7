#!/usr/bin/env python3
"""The panel update (scripts/Primer_set_update.py) measured: the dimer step on a synthetic core set x new set and the off-target step on a
synthetic background, device path against host path on identical files, one JSON line per measurement on stdout.

    python tools/panel_bench.py                                   # on the GPU box: both steps, device and host path
    python tools/panel_bench.py --device-only --core 20000 --new 2000 --skip-offtarget      # the kernel's rate on a larger rectangle
    python tools/panel_bench.py --reference /path/to/reference/scripts/Primer_set_update.py --ref-sample 120,30
                                                                  # the unmodified reference's -f D on a small sample (needs no GPU)

The reference line reports the sample's wall time and the pairs it visited; `scaled_s` is that time scaled linearly by pairs to the
--core x --new rectangle and is labelled as scaled.  Its `-p` is left at the default 10 processes.
"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def primer_files(directory, n_core, n_new, n_common, seed):
    """Random 18..24-base primers without degenerate letters; the last n_common new primers repeat core sequences."""
    rng = np.random.default_rng(seed)

    def make(n):
        return ["".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(18, 25)))) for _ in range(n)]
    core = make(n_core)
    new = make(n_new - n_common) + core[:n_common]
    paths = []
    for name, seqs in (("core", core), ("new", new)):
        paths.append(os.path.join(directory, name + ".fa"))
        with open(paths[-1], "w") as f:
            f.writelines(f">{name}{i}\n{s}\n" for i, s in enumerate(seqs))
    return paths


def pairs_visited(n_core, n_new, n_common):
    return n_core * (n_new - n_common) + n_new * (n_core + n_new - n_common)


def rounded(stats):
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in stats.items()}


def quiet(app):
    with contextlib.redirect_stdout(io.StringIO()):
        app.run()
    return rounded(app.stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--core", type=int, default=1000)
    ap.add_argument("--new", type=int, default=250)
    ap.add_argument("--common", type=int, default=10)
    ap.add_argument("--bases", type=float, default=1e8, help="background size of the off-target step (profiles/offtarget_scale.txt: 1e8)")
    ap.add_argument("--row-len", type=int, default=1_000_000)
    ap.add_argument("--mismatch", type=int, default=1)
    ap.add_argument("--term", type=int, default=9)
    ap.add_argument("--size", default="150,2000")
    ap.add_argument("--repeat", type=int, default=2, help="device runs per step (the first warms the process up)")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--skip-offtarget", action="store_true")
    ap.add_argument("--reference", help="path of the unmodified Primer_set_update.py: time its -f D on --ref-sample and stop")
    ap.add_argument("--ref-sample", default="120,30", help="core,new primers of the reference's sample")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        if a.reference:
            n_core, n_new = (int(x) for x in a.ref_sample.split(","))
            core, new = primer_files(td, n_core, n_new, min(a.common, n_new // 2), 7)
            t0 = time.time()
            subprocess.run([sys.executable, a.reference, "-c", core, "-n", new, "-f", "D", "-o", os.path.join(td, "ref")], check=True,
                           stdout=subprocess.DEVNULL, cwd=td)
            wall = time.time() - t0
            sample = pairs_visited(n_core, n_new, min(a.common, n_new // 2))
            full = pairs_visited(a.core, a.new, a.common)
            print(json.dumps({"step": "dimer", "path": "reference -f D (unmodified, -p 10), CPU", "core": n_core, "new": n_new, "pairs": sample,
                              "wall_s": round(wall, 2), "lines": sum(1 for _ in open(os.path.join(td, "ref.dimer"))) - 1,
                              "scaled_to": {"core": a.core, "new": a.new, "pairs": full}, "scaled_s": round(wall * full / sample, 1),
                              "note": "scaled linearly by pairs from the sample; includes interpreter and pool start-up"}), flush=True)
            return
        import torch  # noqa: F401  (one HIP runtime per process: torch's, as in the GPU suite)
        from multiprime_amd import panel
        from multiprime_amd._abi import Library
        from multiprime_amd.synth import offtarget_case
        lib = Library()
        core, new = primer_files(td, a.core, a.new, a.common, 7)
        rec = {"step": "dimer", "core": a.core, "new": a.new, "common": a.common, "pairs": pairs_visited(a.core, a.new, a.common), "device": []}
        for _ in range(a.repeat):
            rec["device"].append(quiet(panel.Dimer(core, new, os.path.join(td, "dev.dimer"), library=lib)))
        if not a.device_only:
            t0 = time.time()
            rec["host"] = quiet(panel.Dimer(core, new, os.path.join(td, "host.dimer"), search="host"))
            rec["host"]["run_s"] = round(time.time() - t0, 3)
            rec["equal"] = all(open(os.path.join(td, "dev.dimer" + s)).read() == open(os.path.join(td, "host.dimer" + s)).read()
                               for s in ("", ".dimer_num"))
        print(json.dumps(rec), flush=True)
        if rec.get("equal") is False:
            sys.exit(1)
        if a.skip_offtarget:
            return
        n_rows = max(1, int(a.bases) // a.row_len)
        t0 = time.time()
        pf, bf = offtarget_case(td, n_rows, a.row_len, 8, 3, n_degenerate=0)
        records = open(pf).read().split(">")[1:]
        for name, part in (("oc", records[:4]), ("on", records[4:])):          # four primers each: one R in every 3' term, two reads per primer
            with open(os.path.join(td, name + ".fa"), "w") as f:
                f.writelines(">" + r for r in part)
        core, new = os.path.join(td, "oc.fa"), os.path.join(td, "on.fa")
        rec = {"step": "offtargets", "bases": n_rows * a.row_len, "rows": n_rows, "term": a.term, "mismatch": a.mismatch, "size": a.size,
               "make_input_s": round(time.time() - t0, 2), "device": []}
        for _ in range(a.repeat):
            rec["device"].append(quiet(panel.off_targets(core, new, a.mismatch, a.term, bf, a.size, os.path.join(td, "dev.offtargets"), library=lib)))
        if not a.device_only:
            rec["host"] = quiet(panel.off_targets(core, new, a.mismatch, a.term, bf, a.size, os.path.join(td, "host.offtargets"), library=lib,
                                                  join="host"))
            rec["equal"] = all(open(os.path.join(td, "dev.offtargets" + s)).read() == open(os.path.join(td, "host.offtargets" + s)).read()
                               for s in ("", ".num"))
        print(json.dumps(rec), flush=True)
        if rec.get("equal") is False:
            sys.exit(1)


if __name__ == "__main__":
    main()

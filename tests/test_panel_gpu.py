"""The panel update on the GPU: mp_dimer_cross, mp_amplicon_join_classes and mp_offtarget_classes against tests/panel_ref.py in exact
order (hit records sorted by (job, partner)), and scripts/Primer_set_update.py end to end against the host path byte for byte."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

import panel_cases as cases
import panel_ref as R
from conftest import GOLDEN, REPO
from multiprime_amd import iupac, panel
from multiprime_amd.dimer import cached_loss_table, dg_limit, encode_primers
from multiprime_amd.dimer import dg_params as fd_dg_params

pytestmark = pytest.mark.gpu
PANEL = os.path.join(GOLDEN, "panel")


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.context(0)
    yield c
    c.close()


def cross(ctx, seqs, jobs, **kw):
    codes, off = encode_primers(seqs)
    loss, dg, limit = panel.tables()
    return [tuple(r) for r in ctx.dimer_cross(codes, off, np.array(jobs, np.int32).reshape(-1, 3), loss, dg, limit, **kw).tolist()]


# ---- mp_dimer_cross ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long", [False, True])
def test_end_lengths_both_plane_widths(ctx, long):
    seqs, jobs = cases.length_set(long)
    assert max(map(len, seqs)) == (64 if long else 32) and {len(s) for s in seqs} >= set(n for n in cases.LENGTHS if long or n <= 32)
    want = R.cross_records(seqs, jobs)
    got = cross(ctx, seqs, jobs)
    assert got == want
    x_len = {len(seqs[jobs[j][0]]) for j, *_ in want}
    assert x_len >= {n for n in cases.LENGTHS if n >= 4 and (long or n <= 32)}          # every length hits as the job's primer
    assert {l for _, _, l, *_ in want} >= {3, 4, 5, 9, 17, 18}


def test_delta_g_counts_at_any_distance(ctx, monkeypatch):
    seqs, jobs = cases.dg_only_pair()
    want = R.cross_records(seqs, jobs)
    assert want == [(0, 1, 7, 0, 0, 0)]
    assert R.loss(7, 4, 0, 23) <= 3 and R.delta_g("GCGCATT") < -5 and len(seqs[1]) - 7 - 0 >= 21
    assert cross(ctx, seqs, jobs) == want
    # the same pair, the same tables, finDimer's search (pair_search with the d2 == 0 condition): no hit for 0 -> 1
    codes, off = encode_primers(seqs)
    loss, dg, limit = panel.tables()
    for lanes in ("1", "64"):
        monkeypatch.setenv("MP_DIMER_LANES", lanes)
        hits = ctx.dimer_scan(codes, off, 0, 0, loss, dg, limit).tolist()
        assert not any(h[0] == 0 and h[1] == 1 for h in hits), (lanes, hits)
    # and finDimer's own tables leave mode 0 what it was
    monkeypatch.delenv("MP_DIMER_LANES")
    assert not any(h[0] == 0 and h[1] == 1 for h in ctx.dimer_scan(codes, off, 0, 0, cached_loss_table(3.96), fd_dg_params(), dg_limit()).tolist())


def test_degenerate_primers_first_passing_combination(ctx):
    seqs, jobs = cases.degenerate_set()
    want = R.cross_records(seqs, jobs)
    assert cross(ctx, seqs, jobs) == want
    by_pair = {(jobs[j][0], y): (l, ei, pi, idx) for j, y, l, ei, pi, idx in want}
    l, ei, pi, idx = by_pair[(1, 0)]                   # both expansions of the end occur in the host: the first in expansion order
    assert ei == 0 and iupac.expand(seqs[1][-l:])[0] in ("ACTAATGC"[-l:],) and len(iupac.expand(seqs[1][-l:])) == 2
    assert by_pair[(1, 2)][1:3] == (0, 1) or by_pair[(1, 2)][1:3] == (0, 0)
    assert any(pi > 0 for _, _, _, _, pi, _ in want) and any(ei > 0 for _, _, _, ei, _, _ in want)


def test_job_ranges(ctx):
    seqs, jobs = cases.range_set()
    want = R.cross_records(seqs, jobs)
    got = cross(ctx, seqs, jobs)
    assert got == want
    per_job = [sum(1 for r in want if r[0] == j) for j in range(len(jobs))]
    assert per_job[0] >= 199 and per_job[1] == 0 and per_job[-1] == 0 and per_job[3] >= 85 and per_job[5] in (0, 1)
    # no jobs at all, and no primers
    codes, off = encode_primers(seqs)
    loss, dg, limit = panel.tables()
    assert len(ctx.dimer_cross(codes, off, np.zeros((0, 3), np.int32), loss, dg, limit)) == 0


@pytest.mark.parametrize("layout", ["no_core", "no_new", "all_common"])
def test_panel_layouts(tmp_path, hip_lib, layout):
    text = open(os.path.join(PANEL, "plain", "new.fa")).read()
    core, new = tmp_path / "core.fa", tmp_path / "new.fa"
    core.write_text("" if layout == "no_core" else text)
    new.write_text("" if layout == "no_new" else text)
    outs = []
    for search in ("device", "host"):
        out = str(tmp_path / (search + ".dimer"))
        panel.Dimer(str(core), str(new), out, search=search, library=hip_lib).run()
        outs.append((open(out).read(), open(out + ".dimer_num").read()))
    assert outs[0] == outs[1]
    n_lines = outs[0][0].count("\n") - 1
    assert n_lines == (0 if layout == "no_new" else 4), outs[0][0]          # shared <-> n5, n4 -> n3, tiny -> tiny


@pytest.mark.parametrize("every", [1, 5])
def test_queue_and_hit_buffer_drains(ctx, every):
    seqs, jobs = cases.drain_set(every)
    want = R.cross_records(seqs, jobs)
    assert len(want) == (1300 if every == 1 else 260)
    assert cross(ctx, seqs, jobs) == want


def test_cap_smaller_than_the_hit_count(ctx):
    seqs, jobs = cases.drain_set(1)
    want = set(R.cross_records(seqs, jobs))
    codes, off = encode_primers(seqs)
    loss, dg, limit = panel.tables()
    for cap in (0, 1, 700, 1299):
        recs, n = ctx.dimer_cross_raw(codes, off, jobs, loss, dg, limit, cap)
        recs = [tuple(r) for r in recs.tolist()]
        assert n == 1300 and len(recs) == cap and len(set(recs)) == cap and set(recs) <= want


# ---- mp_amplicon_join_classes -------------------------------------------------------------------------------------------------------------
def resolved(sites):
    """One read per (class, strand, row, position), the last entry wins; ascending as the call wants them."""
    at = {}
    for cls, strand, row, pos, read in sites:
        at[(cls, strand, row, pos)] = read
    return [k + (v,) for k, v in sorted(at.items())]


def join_cases():
    F, Rv, CORE, NEW = 0, 1, 0, 1
    return {
        "empty": [],
        "one_site": [(CORE, F, 0, 10, 1)],
        "empty_classes": [(CORE, F, 0, 10, 1), (CORE, Rv, 0, 200, 2)],                        # core x core is never joined
        "last_wins_and_both_keep": [(CORE, F, 0, 100, 1), (CORE, F, 0, 100, 2), (NEW, F, 0, 100, 7), (NEW, Rv, 0, 300, 8), (NEW, Rv, 0, 300, 9),
                                    (CORE, Rv, 0, 320, 3)],
        "early_out_far": [(CORE, F, 0, 10, 1), (CORE, F, 0, 20, 2), (NEW, Rv, 0, 5000, 7)],
        "early_out_close": [(NEW, F, 1, 500, 7), (CORE, Rv, 1, 530, 1), (CORE, Rv, 1, 400, 2)],
        "dead_start": [(NEW, F, 2, 100, 7), (NEW, F, 2, 3000, 8), (NEW, F, 2, 5000, 9), (NEW, Rv, 2, 400, 7), (NEW, Rv, 2, 5300, 8)],
        "bounds": [(CORE, F, 0, 1000, 1)] + [(NEW, Rv, 0, 1000 + n - 1, 7) for n in (99, 100, 101, 1499, 1500, 1501)],
        "three_classes_one_row": [(CORE, F, 3, 1000, 1), (NEW, F, 3, 1010, 7), (NEW, Rv, 3, 1300, 8), (CORE, Rv, 3, 1400, 2),
                                  (CORE, F, 5, 50, 1), (NEW, Rv, 5, 400, 9), (NEW, F, 4, 10, 7), (CORE, Rv, 4, 300, 2)],
    }


@pytest.mark.parametrize("name", list(join_cases()))
def test_join_classes(ctx, name):
    sites = join_cases()[name]
    want = R.join_classes(sites, 100, 1500)
    got = [tuple(r) for r in ctx.amplicon_join_classes(np.array(resolved(sites), np.int32).reshape(-1, 5), 100, 1500).tolist()]
    assert got == want
    n = {"empty": 0, "one_site": 0, "empty_classes": 0, "last_wins_and_both_keep": 3, "early_out_far": 0, "early_out_close": 0, "dead_start": 1,
         "bounds": 2, "three_classes_one_row": 5}[name]
    assert len(want) == n, want
    if name == "last_wins_and_both_keep":
        assert [(r[3], r[4], r[6]) for r in want] == [(2, 9, 0), (7, 3, 1), (7, 9, 2)]
    if name == "three_classes_one_row":
        assert sorted({r[6] for r in want if r[0] == 3}) == [0, 1, 2]
    if name == "bounds":
        assert [r[5] for r in want] == [101, 1499]
    _, counts = ctx.offtarget_stats()
    assert counts["products"] == len(want)


def test_join_classes_cap_and_order_check(ctx, hip_lib):
    sites = np.array(resolved(join_cases()["three_classes_one_row"]), np.int32)
    import ctypes as C
    out = np.zeros((2, 7), np.int32)
    n = C.c_int64(0)
    rc = hip_lib.dll.mp_amplicon_join_classes(ctx.h, len(sites), sites.ctypes.data_as(C.c_void_p), 100, 1500, 2, out.ctypes.data_as(C.c_void_p), C.byref(n))
    assert rc == 0 and n.value == 5 and [tuple(r) for r in out.tolist()] == R.join_classes(sites.tolist(), 100, 1500)[:2]
    from multiprime_amd._abi import MprimeError
    with pytest.raises(MprimeError, match="ascend"):
        ctx.amplicon_join_classes(sites[::-1].copy(), 100, 1500)


# ---- mp_offtarget_classes ---------------------------------------------------------------------------------------------------------------
def store_of(rows):
    data = np.frombuffer("".join(rows).encode(), np.uint8)
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return data, off


@pytest.mark.parametrize("mm", [0, 1])
@pytest.mark.parametrize("term_len", [9, 0])
def test_offtarget_classes_against_scan_and_join(hip_lib, mm, term_len):
    rows, core, new = cases.background_case()
    reads = []                                         # (sequence, class): the expanded terms, core first
    for cls, prim in enumerate((core, new)):
        for seq in dict.fromkeys(s[-term_len:] for _, s in prim):
            reads.append((seq, cls))
    codes, off = encode_primers([s for s, _ in reads])
    cls = np.array([c for _, c in reads], np.int32)
    c = hip_lib.context(0)
    try:
        c.seq_load(*store_of(rows))
        hits = c.kmm_scan_resident(codes, off, mm, 5)
        got = [tuple(r) for r in c.offtarget_classes(codes, off, np.arange(len(reads), dtype=np.int32), cls, mm, 5, 30, 250).tolist()]
        _, counts = c.offtarget_stats()
        again = [tuple(r) for r in c.offtarget_classes(codes, off, np.arange(len(reads), dtype=np.int32), cls, mm, 5, 30, 250, cap=1).tolist()]
        hits = hits[np.lexsort((hits[:, 1], hits[:, 0], hits[:, 2]))]
        sites = [(int(cls[read]), strand, row, pos, read) for row, pos, read, strand in hits.tolist()]
        joined = [tuple(r) for r in c.amplicon_join_classes(np.array(resolved(sites), np.int32).reshape(-1, 5), 30, 250).tolist()]
    finally:
        c.close()
    want = R.join_classes(sites, 30, 250)
    assert got == want == joined == again
    assert counts["hits"] == len(hits) and counts["products"] == len(want)
    assert {r[6] for r in want} == {0, 1, 2}
    if term_len == 0:
        assert (mm == 1) == any(r[0] == 1 and r[1] == 5 for r in want)      # the one-mismatch copy of nF on row 1
    else:
        assert (mm == 1) == any(r[0] == 2 and r[2] == 200 for r in want)    # the reverse site on row 2 whose term needs its mismatch


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def script_main():
    spec = importlib.util.spec_from_file_location("primer_set_update_script", os.path.join(REPO, "scripts", "Primer_set_update.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.main


def four_files(prefix):
    return [open(prefix + s).read() for s in (".dimer", ".dimer.dimer_num", ".offtargets", ".offtargets.num")]


def test_script_on_the_sam_fixture(tmp_path, capsys):
    for name in os.listdir(os.path.join(PANEL, "sam")):
        if not name.startswith("out."):
            shutil.copy(os.path.join(PANEL, "sam", name), tmp_path)
    core, new = str(tmp_path / "core.fa"), str(tmp_path / "new.fa")
    script_main()(["-c", core, "-n", new, "-s", "100,1500", "-o", str(tmp_path / "dev")])
    said = capsys.readouterr().out
    assert "INFO: Start finDimer ..." in said and "off-targets prediction ..." in said and "Total time" in said
    panel.Dimer(core, new, str(tmp_path / "host.dimer"), search="host").run()
    panel.off_targets(core, new, 1, 9, "", "100,1500", str(tmp_path / "host.offtargets"), join="host").run()
    assert four_files(str(tmp_path / "dev")) == four_files(str(tmp_path / "host"))
    assert four_files(str(tmp_path / "dev"))[2].split("\n")[1:-1] == R.offtarget_lines(core, new, 100, 1500)


@pytest.mark.parametrize("case", ["plain", "degenerate"])
def test_script_on_the_dimer_fixtures(tmp_path, case):
    for name in ("core.fa", "new.fa"):
        shutil.copy(os.path.join(PANEL, case, name), tmp_path)
    core, new = str(tmp_path / "core.fa"), str(tmp_path / "new.fa")
    script_main()(["-c", core, "-n", new, "-f", "D", "-o", str(tmp_path / "dev")])
    got = open(tmp_path / "dev.dimer").read().split("\n")[1:-1]
    assert got == R.dimer_lines(core, new)
    assert sorted(got) == sorted(open(os.path.join(PANEL, case, "out.dimer")).read().split("\n")[1:-1])      # the reference's own lines


def test_script_with_the_scan(tmp_path, hip_lib):
    rows, core, new = cases.background_case()
    (tmp_path / "core.fa").write_text("".join(f">{n}\n{s}\n" for n, s in core))
    (tmp_path / "new.fa").write_text("".join(f">{n}\n{s}\n" for n, s in new))
    (tmp_path / "bg.fa").write_text("".join(f">row{i} background\n{r}\n" for i, r in enumerate(rows)))
    core, new, bg = str(tmp_path / "core.fa"), str(tmp_path / "new.fa"), str(tmp_path / "bg.fa")
    script_main()(["-c", core, "-n", new, "-r", bg, "-s", "30,250", "-l", "9", "-m", "1", "-f", "O", "-o", str(tmp_path / "dev")])
    panel.off_targets(core, new, 1, 9, bg, "30,250", str(tmp_path / "host.offtargets"), join="host", library=hip_lib).run()
    dev, host = open(tmp_path / "dev.offtargets").read(), open(tmp_path / "host.offtargets").read()
    assert dev == host and dev.count("\n") > 6 and "row0\t" in dev
    assert open(tmp_path / "dev.offtargets.num").read() == open(tmp_path / "host.offtargets.num").read()
    assert "cF|>nF2_0" not in dev and "nF2_0" in dev          # each file has its own reads: the shared term is a read of either class

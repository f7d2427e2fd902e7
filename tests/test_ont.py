"""The host side of the read-to-primer assignment (multiprime_amd/ontprimer.py) and its yardstick (tests/ont_ref.py) without a GPU: the
yardstick against the reference's recorded outputs, the integer rule against difflib, the device's pair routine built for the CPU
(tools/ont_emul.cpp) against difflib, key order and labels, pieces, the rank table, the strict threshold, the refusals, the scripts' exits.
The class runs here on a stand-in context that answers ont_assign with the yardstick's integer rule."""
import gzip
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import ont_cases as cases
import ont_ref as ref
from conftest import REPO, load_gz_json
from multiprime_amd import ontprimer as op

SCRIPTS = {"FindONTprimerV3.py": os.path.join(REPO, "scripts", "FindONTprimer.py"),
           "FindONTexpandprimer.py": os.path.join(REPO, "scripts", "FindONTexpandprimer.py")}


@pytest.fixture(scope="module")
def golden():
    return load_gz_json("ont_small.json.gz")


def plant(root, golden):
    """The golden run's files in root: the primer file, reads.fq / reads.fa and their .gz."""
    with open(os.path.join(root, golden["primer_file"]), "w") as f:
        f.write(golden["primers"])
    for name, text in golden["inputs"].items():
        with open(os.path.join(root, name), "w") as f:
            f.write(text)
        with gzip.open(os.path.join(root, name + ".gz"), "wb") as f:
            f.write(text.encode())


def flag(flags, name):
    return flags[flags.index(name) + 1]


class YardstickContext:
    """ont_set_keys / ont_assign / ont_stats answered by tests/ont_ref.py's integer rule."""

    def __init__(self):
        self.n = 0

    def ont_set_keys(self, data, off):
        raw = bytes(data)
        self.keys = [raw[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]

    def ont_assign(self, data, off, q):
        raw = bytes(data)
        got = [ref.winner(raw[off[i]:off[i + 1]].decode(), self.keys, q.tolist()) for i in range(len(off) - 1)]
        self.n += len(got)
        return np.array([g[0] for g in got], np.int32), np.array([g[1] for g in got], np.int32)

    def ont_stats(self):
        return {"assign_ms": 0.0}, {"keys": len(self.keys), "pieces": self.n}

    def close(self):
        pass


class YardstickLibrary:
    def context(self, device=0):
        return YardstickContext()


def test_golden_run_has_what_it_should(golden):
    reads = cases.golden_reads()
    assert golden["inputs"]["reads.fq"] == cases.fastq_text(reads) and golden["inputs"]["reads.fa"] == cases.fasta_text(reads)
    assert golden["primers"] == cases.PRIMERS and 38 <= len(reads) <= 42
    assert any(len(r) < cases.LENGTH for r in reads) and not golden["inputs"]["reads.fa"].endswith("\n")
    lines = golden["cases"]["v3_fq"]["lines"]
    assert any("NA" in x for x in lines) and len(lines) > 4
    assert any(r.startswith("ACGTTGCAAGCTTGACCA") for r in reads) and any(r.endswith(ref.rc("ACGTTGCAAGCTTGACCA")) for r in reads)   # both strands


@pytest.mark.parametrize("case", ["v3_fq", "v3_fq_gz", "v3_fa", "v3_fa_gz", "expand_fq"])
def test_yardstick_and_class_reproduce_the_reference(case, golden, tmp_path, monkeypatch):
    """The recorded .num lines (ties ordered) from the yardstick's difflib pipeline and from ONTprimer on the stand-in context, in three
    batches; the expand file byte for byte under the reference's name."""
    rec = golden["cases"][case]
    plant(str(tmp_path), golden)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("MP_ONT_BATCH", "15")
    expand = rec["script"] == "FindONTexpandprimer.py"
    fmt, reads = flag(rec["flags"], "-f"), flag(rec["flags"], "-i")
    min_ident = 0.8 if expand else 0.6
    want = ref.order_lines(rec["lines"])
    assert ref.pipeline(reads, golden["primers"], fmt, golden["length"], min_ident, expand) == want
    app = op.ONTprimer(reads, golden["primer_file"], outfile="out", primer_len=golden["length"], min_ident=min_ident, Input_format=fmt,
                       nproc=3, expand=expand, library=YardstickLibrary())
    app.run()
    assert open("out.num").readlines() == want
    assert open(rec["expand_file"]).read() == rec["expand_text"] and rec["expand_file"] == "_panel.expand.fa"
    assert app.stats[1]["pieces"] == 2 * len(cases.golden_reads())


def random_pairs(n, seed):
    rng = random.Random(seed)
    out = [("ACACACAC", "CACACA"), ("CACACA", "ACACACAC"), ("A" * 64, "A" * 64), ("A" * 64, "A" * 37), ("", ""), ("", "ACGT"), ("ACGT", ""),
           ("AC" * 32, "CA" * 32), ("ACGT" * 16, "TGCA" * 16), ("AAAACCCC", "CCCCAAAA"), ("ACGTACGTAC\n", "ACGTACGTAC")]
    while len(out) < n:
        alpha = rng.choice(["ACGT", "ACGT", "ACGTN\n", "AC", "A"])
        a = "".join(rng.choice(alpha) for _ in range(rng.randint(0, 64)))
        if rng.random() < 0.5 and a:
            b = cases._damage(rng, a, rng.randint(0, 5))
            if rng.random() < 0.4:
                b = b[rng.randint(0, 6):] + "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 6)))
            b = "".join(ch if ch in "ACGT" else "G" for ch in b)[:64]
        else:
            b = "".join(rng.choice(alpha.replace("N\n", "")) for _ in range(rng.randint(0, 64)))
        out.append((a, b))
    return out


def test_integer_rule_equals_difflib():
    for a, b in random_pairs(3000, 11):
        m = ref.match_count(a, b)
        assert m == ref.difflib_count(a, b), (a, b)
        t = len(a) + len(b)
        assert ref.ratio(a, b) == (round(2.0 * m / t, 2) if t else 1.0), (a, b)


def test_device_pair_routine_equals_difflib_on_the_cpu(tmp_path):
    """csrc/ontcore.hpp — the very routine a lane runs — built with g++ behind tools/ont_emul.cpp: 64-bit masks, and 32-bit masks
    where both strings have at most 32 bytes (the program stops if the two disagree)."""
    exe = str(tmp_path / "ont_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(REPO, "tools", "ont_emul.cpp")])
    edge_pieces, edge_keys = cases.word_edge()
    pairs = random_pairs(6000, 12) + [(p, k) for p in edge_pieces for k in edge_keys]
    text = "".join("%s\t%s\n" % (a.replace("\n", "n"), b) for a, b in pairs)         # (any byte outside ACGT is "no base")
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=120).stdout.split()
    assert len(got) == len(pairs)
    for (a, b), m in zip(pairs, got):
        assert int(m) == ref.difflib_count(a, b), (a, b)


def test_key_order_and_labels(tmp_path):
    """A sequence two primers produce sits where it came first and carries the later label; so does a palindromic expansion."""
    p = tmp_path / "set.fa"
    p.write_text(">one\nACGTTR\n>two\nACGTTG\n>pal\nACGCGT\n>three\nAYGT\n")
    keys, labels = op.key_list(str(p))
    kd, text = ref.key_dict(p.read_text())
    assert keys == list(kd) and labels == list(kd.values())
    assert keys == ["ACGTTA", "TAACGT", "ACGTTG", "CAACGT", "ACGCGT", "ACGT", "ATGT", "ACAT"]
    assert labels == [">one | 0", ">one | 0", ">two | 0", ">two | 0", ">pal | 0", ">three | 0", ">three | 1", ">three | 1"]
    assert (tmp_path / "set.expand.fa").read_text() == text == (">one | 0\nACGTTA\n>one | 1\nACGTTG\n>two | 0\nACGTTG\n>pal | 0\nACGCGT\n"
                                                                ">three | 0\nACGT\n>three | 1\nATGT\n")
    assert op.expand("ANR") == ["AAA", "AAG", "ATA", "ATG", "AGA", "AGG", "ACA", "ACG"] == ref.expand("ANR")


def test_expand_file_name_rule(tmp_path, monkeypatch):
    """str.strip("fa") takes the letters f and a from both ends of the whole name."""
    assert op.expand_name("set.fa") == "set.expand.fa"
    assert op.expand_name("fa_panel.fa") == "_panel.expand.fa"
    assert op.expand_name("panel.fasta") == "panel.fastexpand.fa"
    assert op.expand_name("dir/alfa") == "dir/alexpand.fa"
    monkeypatch.chdir(tmp_path)
    open("affa", "w").write(">x\nACGT\n")
    op.key_list("affa")
    assert open("expand.fa").read() == ">x | 0\nACGT\n"


@pytest.mark.parametrize("name,fmt", [("reads.fq", "fq"), ("reads.fq.gz", "fq"), ("reads.fa", "fa"), ("reads.fa.gz", "fa")])
def test_pieces_of_all_four_input_kinds(name, fmt, golden, tmp_path, monkeypatch):
    plant(str(tmp_path), golden)
    monkeypatch.chdir(tmp_path)
    reads = cases.golden_reads()
    want = ref.pieces(name, fmt, 18)
    assert len(want) == len(reads)
    for batch in (None, 7, 1):
        got = [p for b in op.read_pieces(name, fmt, 18, batch) for p in b]
        assert got == [p for pair in want for p in pair], batch
    assert max(len(b) for b in op.read_pieces(name, fmt, 18, 7)) == 14
    if name.endswith("gz"):
        assert all("\n" not in p for pair in want for p in pair) and want[0] == [reads[0][:18], reads[0][-18:]]
    else:
        assert want[0] == [reads[0][:18], reads[0][-17:] + "\n"]                  # the kept quirk: 17 bases and the newline
        short = reads.index("ACGTTGCAAGC")
        assert want[short] == ["ACGTTGCAAGC\n", "ACGTTGCAAGC\n"]                  # shorter than l: the whole line twice
        if fmt == "fa":
            assert want[-1][1] == reads[-1][-18:]                                 # the last line has no newline
    monkeypatch.setenv("MP_ONT_BATCH", "3")
    assert [len(b) for b in op.read_pieces(name, fmt, 18)][:2] == [6, 6]
    with pytest.raises(ValueError):
        list(op.read_pieces(name, "fastq", 18))


def test_empty_line_gives_empty_pieces(tmp_path):
    p = tmp_path / "x.fa"
    p.write_text(">a\n\n>b\nACGT")
    assert list(op.read_pieces(str(p), "fa", 18)) == [["\n", "\n", "ACGT", "ACGT"]]
    with gzip.open(str(tmp_path / "x.fa.gz"), "wb") as f:
        f.write(b">a\n\n>b\nACGT")
    assert list(op.read_pieces(str(tmp_path / "x.fa.gz"), "fa", 18)) == [["", "", "ACGT", "ACGT"]]


def test_rank_table_against_round():
    ratios, q = op.ratio_table(), op.rank_table()
    assert q.shape == (129, 65) and q.dtype == np.int32 and q.min() == 0
    cells = [(t, m) for t in range(129) for m in range(t // 2 + 1)]
    for t, m in cells:
        assert ratios[t, m] == (round(2.0 * m / t, 2) if t else 1.0)
    vals = sorted({ratios[c] for c in cells})
    assert len(vals) == 100 and 0.01 not in vals and q.max() == 99          # 2 / 128 already rounds to 0.02
    for t, m in cells:
        assert q[t, m] == vals.index(ratios[t, m])
    assert (np.diff(q, axis=1) >= 0).all()                                        # what the device's pruning bound relies on
    assert q[0, 0] == q[36, 18] == 99 and q[18, 6] == q[15, 5] and q[36, 9] == vals.index(0.5)
    # rounding cases where the float is not the decimal: 2 * 1 / 16 = 0.125 -> 0.12 (half to even on the binary value)
    assert ratios[16, 1] == 0.12 and ratios[37, 17] == round(34 / 37, 2)


def test_threshold_is_strict(tmp_path):
    """M = 9, T = 36 is ratio 0.5: -m 0.5 gives NA, anything below it the primer."""
    p = tmp_path / "set.fa"
    p.write_text(">half\nAAAAAAAAACCCCCCCCC\n")
    keys, labels = op.key_list(str(p))
    piece = "AAAAAAAAAGGGGGGGGG"
    assert ref.match_count(piece, keys[0]) == 9 and ref.ratio(piece, keys[0]) == 0.5
    assert ref.name_of(piece, keys, labels, 0.5) == "NA" and ref.name_of(piece, keys, labels, 0.49) == ">half"
    for m, want in ((0.5, "NA"), (0.49, ">half")):
        t = op.Tally(keys, labels, m)
        assert t.name(18, 0, 9) == want
        t.add([18, 18], np.array([0, 0]), np.array([9, 9]))
        assert t.lines() == ["Primer_F\tPrimer_R\tNumber\n", "%s\t%s\t1\n" % (want, want)]


def test_tally_orders_ties_by_pair_string():
    t = op.Tally(["AC", "GT", "CC"], [">b | 0", ">a | 0", ">b | 1"], 0.1)
    t.add([2] * 8, np.array([0, 1, 1, 0, 2, 2, 1, 1]), np.array([2, 2, 2, 2, 2, 0, 2, 2]))
    assert t.lines() == ["Primer_F\tPrimer_R\tNumber\n", ">a\t>b\t2\n", ">a\t>a\t1\n", ">b\tNA\t1\n"]
    t = op.Tally(["AC", "GT", "CC"], [">b | 0", ">a | 0", ">b | 1"], 0.1, full_label=True)
    t.add([2] * 4, np.array([0, 1, 2, 1]), np.array([2, 2, 2, 2]))
    assert t.lines() == ["Primer_F\tPrimer_R\tNumber\n", ">a | 0\t>b | 0\t1\n", ">a | 0\t>b | 1\t1\n"]


def test_refusals(tmp_path):
    p = tmp_path / "set.fa"
    for bad in ("ACGTacgt", "ACGIACGT", "ACG-T"):
        p.write_text(">good\nACGT\n>bad one\n%s\n" % bad)
        with pytest.raises(ValueError, match=">bad one"):
            op.key_list(str(p))
        assert not (tmp_path / "set.expand.fa").exists()
    p.write_text(">good\nACGT\n")
    with pytest.raises(ValueError, match="65"):
        op.ONTprimer("reads.fq", str(p), outfile="o", primer_len=65)
    p.write_text(">long\n%s\n" % ("ACGT" * 16 + "A"))
    with pytest.raises(ValueError, match=">long"):
        op.key_list(str(p))
    p.write_text(">k\nACGT\n")
    assert op.ONTprimer("reads.fq", str(p), outfile="o", primer_len=64).primer_len == 64


@pytest.mark.parametrize("script", sorted(SCRIPTS))
def test_scripts_exit_paths(script, tmp_path):
    def run(*args):
        return subprocess.run([sys.executable, SCRIPTS[script]] + list(args), cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    (tmp_path / "set.fa").write_text(">k\nACGT\n")
    (tmp_path / "reads.fq").write_text("@r\nACGT\n+\nIIII\n")
    res = run()
    assert res.returncode == 1 and "Usage:" in res.stdout and "--min_ident" in res.stdout
    assert ("Default: 0.8" if "expand" in script else "Default: 0.6") in res.stdout
    res = run("-s", "set.fa", "-o", "out")
    assert res.returncode == 1 and "Input file must be specified !!!" in res.stdout
    res = run("-i", "reads.fq", "-s", "set.fa")
    assert res.returncode == 1 and "No output file provided !!!" in res.stdout
    res = run("-i", "reads.fq", "-s", "set.fa", "-o", "out", "-f", "fastq")
    assert res.returncode == 1 and "-f (only fa or fq) is accepted!" in res.stdout and not (tmp_path / "out.num").exists()
    res = run("-i", "reads.fq", "-s", "set.fa", "-o", "out", "-l", "65")
    assert res.returncode == 2 and "65" in res.stderr

"""Plain restatement of the both-strand rule of include/mprime_ani.h (THE RULE, BOTH STRANDS) — the yardstick of
tests/test_ani_strand_gpu.py, checked itself by tests/test_ani_strand.py: the canonical value of a word and whether an occurrence is as
read, the canonical sketch with its orientation bits, a pair's (same, opp), two groups' (SAME, OPP) and the strand they vote, and the
file operation of a merge that turns a cluster.  Everything the forward rule already states (hash, table, pair, decision, files) is
ani_ref's.  Dictionaries, sorted lists and loops.  A helper, not a test."""
from __future__ import annotations

import os
import shutil

import ani_ref as ref

_PAIRS = "ATGCRYMKSWHBVDN", "TACGYRKMSWDVBHN"                      # the complement table of multiprime_amd/iupac.py
_COMP = str.maketrans(_PAIRS[0] + _PAIRS[0].lower(), _PAIRS[1] + _PAIRS[1].lower())


def rc(seq):
    """The reverse complement, IUPAC letters and lower case included; any other character stays."""
    return seq.translate(_COMP)[::-1]


def word_rc(v):
    """The value of the reverse-complement word of the word of value v."""
    r = 0
    for _ in range(ref.WORD):
        r = r * 4 + (3 - (v & 3))
        v >>= 2
    return r


def canonical_words(seq):
    """{canonical value: True if the record holds an as-read occurrence of it}."""
    codes = ["ACGT".find(chr(b & 0xDF)) for b in seq.encode("latin-1")]
    out = {}
    for i in range(len(codes) - ref.WORD + 1):
        w = codes[i:i + ref.WORD]
        if min(w) >= 0:
            f = 0
            for cd in w:
                f = f * 4 + cd
            cv = min(f, word_rc(f))
            out[cv] = out.get(cv, False) or f == cv
    return out


def sketch(seq, s=1024):
    """(hashes, bits): the canonical sketch at size s and the orientation bit of every element."""
    both = sorted((ref.fmix32(cv), 0 if as_read else 1) for cv, as_read in canonical_words(seq).items())[:s]
    return [h for h, _ in both], [b for _, b in both]


def bit_words(bits, s):
    """The bits as the library stores them: (s + 31) // 32 words, bit i % 32 of word i // 32 for element i."""
    out = [0] * ((s + 31) // 32)
    for i, b in enumerate(bits):
        out[i // 32] |= b << (i % 32)
    return out


def pair_strand(a, b, s):
    """(same, opp) of two (hashes, bits) sketches at size s; (w, u, ani_ppm) is ani_ref.pair on the hashes."""
    lasts = [x[0][-1] for x in (a, b) if len(x[0]) == s]
    c = min(lasts) if lasts else None
    bit_b = dict(zip(*b))
    same = opp = 0
    for h, bit in zip(*a):
        if h in bit_b and (c is None or h <= c):
            if bit == bit_b[h]:
                same += 1
            else:
                opp += 1
    return same, opp


def groups_strand(p_sketches, r_sketches, s, report_ppm):
    """(SAME, OPP) over the reported pairs of all (p, r)."""
    same = opp = 0
    for a in p_sketches:
        for b in r_sketches:
            if ref.pair(a[0], b[0], s)[2] >= report_ppm:
                x, y = pair_strand(a, b, s)
                same += x
                opp += y
    return same, opp


def strand(same, opp):
    return "-" if opp > same else "+"


# ---- the files ---------------------------------------------------------------------------------------------------------------------------
def rc_fasta(data):
    """The bytes of a FASTA file with every record turned: header lines as they are, a record's sequence lines joined, reversed and
    complemented, on one line."""
    out, seq = [], None
    for line in data.decode("latin-1").splitlines(True):
        if line.startswith(">"):
            if seq is not None:
                out.append(rc(seq) + "\n")
            seq = None
            out.append(line if line.endswith("\n") else line + "\n")
        elif line.strip():
            seq = (seq or "") + line.strip()
    if seq is not None:
        out.append(rc(seq) + "\n")
    return "".join(out).encode("latin-1")


def apply_orient(clusters, wd, md, strands):
    """ani_ref.apply in merge mode where a sub whose strands[(ref id, sub id)] is '-' arrives turned (.fa and .tfa; the .txt as is)."""
    for name, size in clusters:
        shutil.rmtree("%s/%s_%d" % (wd, name, size), ignore_errors=True)
    now = {}
    for r in sorted(md, key=lambda x: int(x.rsplit("_", 1)[1])):
        total = int(r.rsplit("_", 1)[1])
        for sub in md[r]:
            cur = now.get(sub, sub)
            total += int(cur.rsplit("_", 1)[1])
            for ext in (".fa", ".tfa", ".txt"):
                data = open(cur + ext, "rb").read()
                with open(r + ext, "ab") as fo:
                    fo.write(rc_fasta(data) if strands[(r, sub)] == "-" and ext != ".txt" else data)
                os.remove(cur + ext)
        final = "%s_%d" % (r.rsplit("_", 1)[0], total)
        for ext in (".fa", ".tfa", ".txt"):
            os.rename(r + ext, final + ext)
        now[r] = final


def strand_text(md, votes):
    """<out>.strand: votes[(ref id, sub id)] = (SAME, OPP)."""
    return "".join("%s\t%s\t%s\t%d\t%d\n" % (k, m, strand(*votes[(k, m)]), votes[(k, m)][0], votes[(k, m)][1]) for k, subs in md.items() for m in subs)

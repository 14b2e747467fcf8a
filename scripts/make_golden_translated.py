#!/usr/bin/env python3
"""Generates the fixtures of the six-frame translation (vmatch -dnavsprot)
under tests/golden/ from the REAL reference.

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`, and the product library for back-translating):

    python3 scripts/make_golden_translated.py

Writes new files only -- DATA, no program text:
  translated_codons.json     (a) per translation table the amino acid of the
                             64 plain codons in the forward and in the reverse
                             direction, (b) of the 15^3 codons over
                             TCAGNSYWRKVBDHM under tables 1 and 2, and of a
                             lower-case / U sample: read off the POSITION of
                             the F and the G line of `-dnavsprot T -l 1`
                             against an index of ACDEFGHIKLMNPQRSTVWY (no
                             line: a stop codon, '*'); (d) the error texts
  translated_q.fna.gz        (c) about 200 DNA queries from a fixed seed
  translated_complete.fna    (c) a few whose six frames all reach the prefix
                             length of the index
  translated_runs.json.gz    (c) per run the vmatch options, exit code,
                             stderr and every line of stdout behind "# args="
The protein database is the existing prot_db.fna.gz, which is not touched.
"""
import gzip
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import helpers as H  # noqa: E402
import vstree_amd as V  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
AMINO = "ACDEFGHIKLMNPQRSTVWY"
BASES = "TCAG"
LETTERS = "TCAGNSYWRKVBDHM"
L = 6          # -l of the end-to-end runs (>= the prefix length 2)
NOMATCH = 20   # -qnomatch / -dbnomatch


def codons(letters):
    return [a + b + c for a in letters for b in letters for c in letters]


def record_codons(wd, name, cods, transnum):
    """-> (forward, reverse): one amino-acid letter per codon, '*' where
    vmatch prints no line"""
    H.write_fasta(os.path.join(wd, name), [("c%d" % i, c.encode())
                                           for i, c in enumerate(cods)])
    rc, lines, err = H.run_vmatch_ref(["-dnavsprot", str(transnum), "-l", "1",
                                       "-q", name, "amino"], wd)
    assert rc == 0, err
    fwd, rev = ["*"] * len(cods), ["*"] * len(cods)
    for l in lines:
        f = l.split()
        assert f[0] == "1" and f[1] == "0" and f[4] == "3" and f[6] == "0"
        which = {"F": fwd, "G": rev}[f[3]]
        assert which[int(f[5])] == "*"      # one line per codon and strand
        which[int(f[5])] = AMINO[int(f[2])]
    return "".join(fwd), "".join(rev)


def backtranslate(rng, peptide, table):
    """random codons of the amino acids of peptide (bytes) -> str"""
    out = []
    for aa in peptide:
        out.append(table[chr(aa)][int(rng.integers(0, len(table[chr(aa)])))])
    return "".join(out)


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def make_queries(rng, db, table):
    """about 200 DNA sequences of 1 .. 400 characters"""
    def randdna(n):
        return "".join(BASES[int(b)] for b in rng.integers(0, 4, n))

    def stretch(k=None):
        s = db[int(rng.integers(0, len(db)))]
        k = int(rng.integers(8, 40)) if k is None else k
        while True:
            p = int(rng.integers(0, len(s) - k))
            if b"X" not in s[p:p + k]:
                return s[p:p + k]

    qs, repeated = [], [stretch(14) for _ in range(6)]
    for i in range(200):
        if i < 2:                                 # a whole frame is a stretch
            dna = backtranslate(rng, stretch(12), table)
            qs.append(revcomp(dna) if i else dna)
            continue
        if 100 <= i < 105:
            qs.append(randdna(i - 99))            # lengths 1 .. 5
            continue
        if i % 10 == 9:
            qs.append(randdna(int(rng.integers(6, 400))))
            continue
        pep = repeated[i % 6] if i % 7 == 3 else stretch()
        dna = backtranslate(rng, pep, table)
        if i % 9 == 4:                            # an IUPAC letter inside
            p = int(rng.integers(3, len(dna) - 3))
            dna = dna[:p] + "NSYWRKVBDHM"[i % 11] + dna[p + 1:]
        if i % 11 == 5:                           # a stop codon inside
            p = 3 * int(rng.integers(2, len(dna) // 3 - 2))
            dna = dna[:p] + ("TAA", "TAG", "TGA")[i % 3] + dna[p + 3:]
        if i % 13 == 6:                           # the stretch twice
            dna = dna + randdna(int(rng.integers(1, 9))) + \
                backtranslate(rng, pep, table)
        dna = randdna(int(rng.integers(0, 30))) + dna + \
            randdna(int(rng.integers(0, 30)))     # every frame
        if i % 2:
            dna = revcomp(dna)                    # both strands
        if i % 17 == 8:
            dna = dna.lower().replace("t", "u")
        qs.append(dna[:400])
    assert [len(q) for q in qs[100:105]] == [1, 2, 3, 4, 5]
    return qs


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    wd = tempfile.mkdtemp()
    out = {"amino": AMINO, "bases": BASES, "letters": LETTERS, "plain": {},
           "wildcards": {}, "sample": {}, "errors": {}}

    # ---- (a), (b): codons against an index of the twenty amino acids ------
    H.write_fasta(wd + "/amino.fna", [("amino", AMINO.encode())])
    H.run_mkvtree_ref(["-db", "amino.fna", "-indexname", "amino", "-protein",
                       "-pl", "1", "-allout"], wd)
    for t in V.TRANSLATION_TABLES:
        f, r = record_codons(wd, "plain.fna", codons(BASES), t)
        out["plain"][str(t)] = {"forward": f, "reverse": r}
    wild = codons(LETTERS)
    rng = np.random.default_rng(20261019)
    pick = sorted(int(x) for x in rng.choice(len(wild), 300, replace=False))
    out["sample"]["index"] = pick
    for t in (1, 2):
        f, r = record_codons(wd, "wild.fna", wild, t)
        out["wildcards"][str(t)] = {"forward": f, "reverse": r}
        lower = [wild[i].lower().replace("t", "u") if k % 2
                 else wild[i].lower() for k, i in enumerate(pick)]
        f, r = record_codons(wd, "lower.fna", lower, t)
        out["sample"][str(t)] = {"codons": lower, "forward": f, "reverse": r}
        # (what the test takes for granted: case and U do not matter)
        assert f == "".join(out["wildcards"][str(t)]["forward"][i]
                            for i in pick)

    # ---- (d): the error of an illegal table number --------------------------
    for t in (0, 7, 8, 17, 20, 24):
        rc, lines, err = H.run_vmatch_ref(["-dnavsprot", str(t), "-l", "1",
                                           "-q", "plain.fna", "amino"], wd)
        assert rc != 0 and not lines
        out["errors"][str(t)] = err.strip().replace(
            H.VMATCH_REF, os.path.basename(H.VMATCH_REF))
    with open(GOLD + "/translated_codons.json", "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)

    # ---- (c): end to end on prot_db.fna.gz ---------------------------------
    db = [s for _, s in H.read_fasta(H._golden_fasta("prot_db.fna.gz"))]
    shutil.copy(H._golden_fasta("prot_db.fna.gz"), wd + "/prot_db.fna")
    H.run_mkvtree_ref(["-db", "prot_db.fna", "-protein", "-pl", "-allout"],
                      wd)
    pl = H.read_prj(wd + "/prot_db.fna.prj")["prefixlength"]
    assert pl == H.alphabets_manifest()["prot"]["index"]["prj"][
        "prefixlength"] and L >= pl
    table = {}
    for cod, aa in zip(codons(BASES), out["plain"]["1"]["forward"]):
        table.setdefault(aa, []).append(cod)
    qs = make_queries(rng, db, table)
    H.write_fasta(wd + "/translated_q.fna", [("r%d" % i, q.encode())
                                             for i, q in enumerate(qs)])
    # the second file: every frame reaches the prefix length, two sequences
    # are whole stretches of the database in frame 0 and in a reverse frame
    small = [backtranslate(rng, db[3][20:32], table),
             revcomp(backtranslate(rng, db[7][5:14], table)),
             "".join(BASES[int(b)] for b in rng.integers(0, 4, 3 * pl + 2)),
             backtranslate(rng, db[3][20:32], table),
             "".join(BASES[int(b)] for b in rng.integers(0, 4, 50))]
    assert min(len(s) for s in small) >= 3 * pl + 2
    H.write_fasta(wd + "/translated_complete.fna",
                  [("k%d" % i, s.encode()) for i, s in enumerate(small)])
    with open(wd + "/translated_q.fna", "rb") as f, \
            gzip.GzipFile(GOLD + "/translated_q.fna.gz", "wb", mtime=0) as g:
        g.write(f.read())
    shutil.copy(wd + "/translated_complete.fna",
                GOLD + "/translated_complete.fna")

    runs = {}

    def record(key, args, least=1):
        rc, lines, err = H.run_vmatch_ref(args, wd)
        runs[key] = {"args": args, "rc": rc, "lines": lines,
                     "stderr": err.strip().replace(
                         H.VMATCH_REF, os.path.basename(H.VMATCH_REF))}
        assert len(lines) >= least, (key, len(lines), err)
        return lines

    tail = ["-q", "translated_q.fna", "prot_db.fna"]
    mem = record("mem", ["-dnavsprot", "1", "-l", str(L)] + tail, least=200)
    mum = record("mum", ["-dnavsprot", "1", "-mum", "-l", str(L)] + tail)
    cand = record("mumcand", ["-dnavsprot", "1", "-mum", "cand", "-l",
                              str(L)] + tail)
    assert len(mum) < len(cand) < len(mem)
    assert any(" F " in l for l in mem) and any(" G " in l for l in mem)
    record("mem_absolute", ["-dnavsprot", "1", "-l", str(L), "-absolute"]
           + tail)
    record("mem_qnomatch", ["-dnavsprot", "1", "-l", str(L), "-qnomatch",
                            str(NOMATCH)] + tail)
    record("mem_dbnomatch", ["-dnavsprot", "1", "-l", str(L), "-dbnomatch",
                             str(NOMATCH)] + tail)
    other = record("mem_table4", ["-dnavsprot", "4", "-l", str(L)] + tail)
    assert other != mem
    record("complete", ["-dnavsprot", "1", "-complete", "-q",
                        "translated_complete.fna", "prot_db.fna"], least=2)
    # (the first two queries match before the first frame of length 0)
    record("complete_short", ["-dnavsprot", "1", "-complete"] + tail, least=2)
    assert runs["complete_short"]["rc"] != 0
    assert "patternlength=0 must be >= %d=prefixlen" % pl in \
        runs["complete_short"]["stderr"]
    for key, run in runs.items():
        assert (run["rc"] != 0) == (key == "complete_short"), (key, run)
    shutil.rmtree(wd)
    with gzip.GzipFile(GOLD + "/translated_runs.json.gz", "wb", mtime=0) as g:
        g.write(json.dumps({"L": L, "nomatch": NOMATCH, "runs": runs},
                           indent=0, sort_keys=True).encode())
    for name in ("translated_codons.json", "translated_q.fna.gz",
                 "translated_complete.fna", "translated_runs.json.gz"):
        assert os.path.getsize(os.path.join(GOLD, name)) < 300000, name
    print({k: len(r["lines"]) for k, r in runs.items()})


if __name__ == "__main__":
    main()

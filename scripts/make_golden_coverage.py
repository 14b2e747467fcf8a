#!/usr/bin/env python3
"""Generates the coverage fixtures under tests/golden/ from the REAL
reference: what vmatch prints for -dbnomatch / -qnomatch / -dbmaskmatch /
-qmaskmatch on the golden inputs that are there already.

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_coverage.py

Writes tests/golden/coverage_manifest.json and coverage_expected.npz -- DATA
only; make_golden.py and its two files are not touched.  Every run is
described by a recipe (RUNS below) from which both the vmatch command line
and, in the tests, the calls of the engine are derived.  Stored per run:
  nomatch  the printed lines parsed into integers (seqnum, relstart, length;
           with -absolute start, length) and the md5 of the lines,
  mask     (mask character x) the masked positions of the Multiseq as
           (start, length) intervals, the md5 of the masked sequences (one
           line per sequence, no description lines) and the number of masked
           symbols the reference reports,
  and the match list of the same command without the coverage option -- as
  the name of the list in expected.npz where that file holds the very same
  list, as an array of its own otherwise (columns length, dbseq, dbrel,
  queryseq, querystart, palindromic).
"""
import gzip
import hashlib
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

GOLD = os.path.join(ROOT, "tests", "golden")


def R(key, engine, L=0, side="db", minlength=None, mask=False, keep=None,
      mum=False, strands="d", absolute=False, index="db", approx=None,
      hint=None):
    return dict(key=key, engine=engine, L=L, side=side, minlength=minlength,
                mask=mask, keep=keep, mum=mum, strands=strands,
                absolute=absolute, index=index, approx=approx, hint=hint)


# engine: query (-l L [-mum] -q), complete (-complete [-e K] -q), repeats
# (-l L IDX), supermax, tandem, selfmum (-mum -l L on an index with queries)
RUNS = {
    "micro": [
        R("q_l3_dbnomatch2", "query", 3, "db", 2, hint="mem3_sp2"),
        R("q_l3_qnomatch1", "query", 3, "q", 1, hint="mem3_sp2"),
        R("q_mum3_qnomatch1", "query", 3, "q", 1, mum=True, hint="mum3"),
        R("q_p_l3_qnomatch1", "query", 3, "q", 1, strands="p"),
        R("q_dp_l3_dbnomatch2_abs", "query", 3, "db", 2, strands="dp",
          absolute=True),
        R("q_l3_dbmask", "query", 3, "db", mask=True, hint="mem3_sp2"),
        R("q_l3_qmask", "query", 3, "q", mask=True, hint="mem3_sp2"),
        R("s_l2_dbnomatch2", "repeats", 2, "db", 2, hint="repeats2"),
        R("s_l2_dbnomatch2_keepleft", "repeats", 2, "db", 2, keep="keepleft",
          hint="repeats2"),
        R("s_l3_keepleft", "repeats", 3, "db", 2, keep="keepleft"),
        R("s_l3_keepright", "repeats", 3, "db", 2, keep="keepright"),
        R("s_l3_keepleftifsame", "repeats", 3, "db", 2,
          keep="keepleftifsamesequence"),
        R("s_l3_keeprightifsame", "repeats", 3, "db", 2,
          keep="keeprightifsamesequence"),
        R("s_supermax2_dbnomatch1", "supermax", 2, "db", 1, hint="supermax2"),
        R("s_tandem1_dbmask", "tandem", 1, "db", mask=True, hint="tandem1"),
        R("c_dbnomatch3", "complete", 0, "db", 3, hint="complete"),
        R("c_e1_dbnomatch3", "complete", 0, "db", 3, approx=[1, 1]),
        R("all_l3_dbnomatch2", "repeats", 3, "db", 2, index="all"),
        R("all_l3_qnomatch1", "repeats", 3, "q", 1, index="all"),
        R("all_mum3_dbnomatch2", "selfmum", 3, "db", 2, index="all"),
        R("all_mum3_qnomatch1", "selfmum", 3, "q", 1, index="all"),
    ],
    "grumbach": [
        R("q_l14_dbnomatch20", "query", 14, "db", 20, hint="mem14_sp2"),
        R("q_l14_qnomatch20", "query", 14, "q", 20, hint="mem14_sp2"),
        R("q_mum14_dbnomatch20", "query", 14, "db", 20, mum=True,
          hint="mum14"),
        R("q_mum14_qnomatch20", "query", 14, "q", 20, mum=True, hint="mum14"),
        R("q_dp_l14_qnomatch20", "query", 14, "q", 20, strands="dp"),
    ],
    "largepat": [
        R("s_l40_dbnomatch1000", "repeats", 40, "db", 1000, hint="repeats40"),
        R("s_l40_dbnomatch1000_keepleftifsame", "repeats", 40, "db", 1000,
          keep="keepleftifsamesequence", hint="repeats40"),
        R("s_supermax30_dbnomatch1000", "supermax", 30, "db", 1000,
          hint="supermax30"),
        R("s_tandem8_dbnomatch1000", "tandem", 8, "db", 1000, hint="tandem8"),
    ],
    "c1": [
        R("q_mum20_dbnomatch50", "query", 20, "db", 50, mum=True,
          hint="mum20"),
        R("q_mum20_qnomatch10", "query", 20, "q", 10, mum=True, hint="mum20"),
    ],
    "c5": [
        R("c_e2_dbnomatch50", "complete", 0, "db", 50, approx=[1, 2],
          hint="approx_e2"),
    ],
}


def engine_args(r):
    e = r["engine"]
    if e == "query":
        a = ["-l", str(r["L"])] + (["-mum"] if r["mum"] else [])
        a += {"d": [], "p": ["-p"], "dp": ["-d", "-p"]}[r["strands"]]
    elif e == "complete":
        a = ["-complete"]
        if r["approx"]:
            a += ["-e" if r["approx"][0] else "-h", str(r["approx"][1])]
    elif e == "repeats":
        a = ["-l", str(r["L"])]
    elif e == "supermax":
        a = ["-supermax", "-l", str(r["L"])]
    elif e == "tandem":
        a = ["-tandem", "-l", str(r["L"])]
    elif e == "selfmum":
        a = ["-mum", "-l", str(r["L"])]
    else:
        raise KeyError(e)
    return a


def coverage_args(r):
    if r["mask"]:
        a = ["-dbmaskmatch" if r["side"] == "db" else "-qmaskmatch", "x"]
    else:
        a = ["-dbnomatch" if r["side"] == "db" else "-qnomatch",
             str(r["minlength"])]
    if r["keep"]:
        a.append(r["keep"])
    if r["absolute"]:
        a.append("-absolute")
    return a


def tail_args(r, files):
    withq = r["engine"] in ("query", "complete")
    return (["-q", files["query"]] if withq else []) + [files[r["index"]]]


def parse_matches(lines, approx):
    out = np.zeros((len(lines), 6), np.uint64)
    for i, l in enumerate(lines):
        f = l.split()
        out[i] = (int(f[0]), int(f[1]), int(f[2]), int(f[5]),
                  abs(int(f[7])) if approx else int(f[6]),
                  1 if f[3] == "P" else 0)
    return out


def same_as_expected(case, hint, m):
    if hint is None:
        return False
    want = H.expected(case, hint)
    return (len(want) == len(m) and not m[:, 5].any() and
            all(np.array_equal(want[k], m[:, j]) for j, k in
                enumerate(("length", "dbseq", "dbrel", "queryseq",
                           "querystart"))))


def intervals_of(flags):
    """positions where flags is true -> (start, length) rows"""
    d = np.diff(np.concatenate(([0], flags.astype(np.int8), [0])))
    s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return np.stack([s, e - s], axis=1).astype(np.uint64)


def prepare(case, wd):
    """the files of a case in wd and their indexes -> names"""
    m = H.manifest()[case]
    if "synthetic" in m:
        g, qb, n, nq, mm = H.synth_c1()
        H.write_fasta(wd + "/db.fna", [("synthetic_genome seed=42", g)])
        H.write_fasta(wd + "/q.fna", [("q%d" % i, qb[i * mm:(i + 1) * mm])
                                      for i in range(nq)], width=1000)
    else:
        def unpack(name, dst):
            src = os.path.join(GOLD, name)
            if name.endswith(".gz"):
                with gzip.open(src, "rb") as f, open(dst, "wb") as g:
                    g.write(f.read())
            else:
                shutil.copy(src, dst)
        assert len(m["db"]) == 1
        unpack(m["db"][0], wd + "/db.fna")
        unpack(m["query"], wd + "/q.fna")
    H.run_mkvtree_ref(["-db", "db.fna", "-dna", "-pl", "-allout"], wd)
    files = {"db": "db.fna", "query": "q.fna"}
    if any(r["index"] == "all" for r in RUNS[case]):
        H.run_mkvtree_ref(["-indexname", "all", "-db", "db.fna", "-q",
                           "q.fna", "-dna", "-pl", "-allout"], wd)
        files["all"] = "all"
    return files


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    manifest, arrays = {}, {}
    for case, runs in RUNS.items():
        wd = tempfile.mkdtemp()
        files = prepare(case, wd)
        manifest[case] = {}
        for r in runs:
            name = "%s__%s" % (case, r["key"])
            args = engine_args(r) + coverage_args(r) + tail_args(r, files)
            p = H.subprocess.run([H.VMATCH_REF] + args, cwd=wd,
                                 stdout=H.subprocess.PIPE,
                                 stderr=H.subprocess.PIPE)
            assert p.returncode == 0, (args, p.stderr.decode())
            lines = [l for l in p.stdout.decode().splitlines()
                     if l and not l.startswith("#")]
            entry = dict(r)
            entry["args"] = args
            if r["mask"]:
                seqs, cur = [], None
                for l in lines:
                    if l.startswith(">"):
                        cur = []
                        seqs.append(cur)
                    else:
                        cur.append(l)
                seqs = ["".join(s) for s in seqs]
                body = "\n".join(seqs) + "\n"
                flat = np.frombuffer("\n".join(seqs).encode(), np.uint8)
                arrays[name + "__masked"] = intervals_of(flat == ord("x"))
                entry["md5_body"] = hashlib.md5(body.encode()).hexdigest()
                note = [l for l in (p.stdout + p.stderr).decode().splitlines()
                        if "number of masked symbols" in l]
                entry["masked"] = int(note[0].split("symbols:")[1].split()[0])
                entry["positions"] = int(
                    note[0].split("length:")[1].split(",")[0])
                assert entry["masked"] == int((flat == ord("x")).sum())
            else:
                arrays[name + "__intervals"] = np.array(
                    [[int(x) for x in l[1:].split()] for l in lines],
                    np.uint64).reshape(len(lines), 2 if r["absolute"] else 3)
                entry["lines"] = len(lines)
                entry["md5_lines"] = hashlib.md5(
                    ("\n".join(lines) + "\n").encode()).hexdigest()
            # the match list of the same command without the coverage option
            rc, mlines, err = H.run_vmatch_ref(
                engine_args(r) + tail_args(r, files), wd)
            assert rc == 0, err
            m = parse_matches(mlines, bool(r["approx"]))
            if same_as_expected(case, r["hint"], m):
                entry["matches"] = "expected:" + r["hint"]
            else:
                assert r["hint"] is None, (name, "differs from", r["hint"])
                mkey = "%s__matches__%s" % (case, "_".join(
                    engine_args(r) + [r["index"]]).replace("-", ""))
                arrays[mkey] = m
                entry["matches"] = mkey
            del entry["key"], entry["hint"]
            manifest[case][r["key"]] = entry
        shutil.rmtree(wd)
    np.savez_compressed(GOLD + "/coverage_expected.npz", **arrays)
    with open(GOLD + "/coverage_manifest.json", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", len(arrays), "arrays for",
          sum(len(v) for v in manifest.values()), "runs")


if __name__ == "__main__":
    main()

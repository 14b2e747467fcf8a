#!/usr/bin/env python3
"""Generates the fixtures of the Hamming extension under tests/golden/ from
the REAL reference: what vmatch prints for -l L -h K [-seedlength S] with and
without -q on the golden inputs that are there already.

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_extend.py

Writes tests/golden/extend_manifest.json and extend_expected.npz -- DATA only.
Every run is described by a recipe (tests/extend_cases.py: RUNS) from which
the vmatch command line and, in the tests, the seed lists and the calls of the
engine are derived.  Stored per run: the rows (length, seq1, rel1, seq2, rel2,
distance, palindromic) in the order of the lines, the md5 of the lines, and
the reference's error text where the run is an error.  The pure-Python model
(tests/extend_model.py), fed with the seed lists of the CPU oracle, must
reproduce every recorded list, order included, or nothing is written.
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
import extend_cases as EC  # noqa: E402
import extend_model as EM  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MAXROWS = 6000


def unpack(name, dst):
    src = os.path.join(GOLD, name)
    if name.endswith(".gz"):
        with gzip.open(src, "rb") as f, open(dst, "wb") as g:
            g.write(f.read())
    else:
        shutil.copy(src, dst)


def prepare(r, wd):
    m = (H.alphabets_manifest() if r["alphabet"] else H.manifest())[r["case"]]
    assert len(m["db"]) == 1
    unpack(m["db"][0], wd + "/db.fna")
    args = ["-indexname", "db.fna", "-db", "db.fna"]
    if m.get("indexedquery"):
        assert len(m["indexedquery"]) == 1
        unpack(m["indexedquery"][0], wd + "/iq.fna")
        args += ["-q", "iq.fna"]
    if r["q"]:
        unpack(m["query"], wd + "/q.fna")
    H.run_mkvtree_ref(args + ["-protein" if r["alphabet"] else "-dna", "-pl",
                              "-allout"], wd)
    prj = H.read_prj(wd + "/db.fna.prj")
    assert prj["prefixlength"] == m["index"]["prj"]["prefixlength"]


def model_rows(r):
    idx, _ = EC.load(r)
    ev = EM.Evalues(idx.numofchars)
    parts = []
    for pal, queries in EC.passes(r):
        seeds = EC.oracle_seeds(r, queries)
        rec = EM.extend(seeds, idx.tis, idx.numofchars, r["L"], r["K"],
                        r["S"], None if queries is None else
                        (queries.symbols, queries.start, queries.length), ev)
        parts.append(EC.rows_of(r, rec, pal))
    return np.concatenate(parts)


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    manifest, arrays = {}, {}
    for r in EC.RUNS:
        wd = tempfile.mkdtemp()
        prepare(r, wd)
        args = EC.vmatch_args(r) + (["-q", "q.fna"] if r["q"] else []) + \
            ["db.fna"]
        rc, lines, err = H.run_vmatch_ref(args, wd)
        shutil.rmtree(wd)
        entry = dict(r, args=args)
        del entry["key"]
        if r["error"]:
            assert rc != 0 and not lines, (r["key"], rc, len(lines))
            # (the message behind the name of the program)
            entry["stderr"] = err.strip().split(": ", 1)[1]
        else:
            assert rc == 0, (r["key"], err)
            assert 0 < len(lines) <= MAXROWS, (r["key"], len(lines))
            rows = EC.parse_rows(lines)
            got = model_rows(r)
            assert np.array_equal(got, rows), \
                (r["key"], len(got), len(rows))
            arrays[r["key"]] = rows.astype(np.int32)
            entry["lines"] = len(lines)
            entry["md5_lines"] = EC.md5(("\n".join(lines) + "\n").encode())
            entry["maxdistance"] = int(rows[:, 5].max())
            entry["maxlength"] = int(rows[:, 0].max())
        manifest[r["key"]] = entry
        print(r["key"], entry.get("lines"), entry.get("stderr", ""))
    np.savez_compressed(GOLD + "/extend_expected.npz", **arrays)
    with open(GOLD + "/extend_manifest.json", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", len(arrays), "lists")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates the fixtures of the edit-distance extension under tests/golden/
from the REAL reference: what vmatch prints for -l L -e K [-seedlength S] with
and without -q on the golden inputs that are there already
(scripts/make_golden_extend.py with -e).

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_extend_edist.py

Writes tests/golden/extend_edist_manifest.json and extend_edist_expected.npz
-- DATA only.  Every run is described by a recipe (tests/extend_edist_cases.py:
RUNS).  Stored per run: the rows (length1, seq1, rel1, length2, seq2, rel2,
distance, palindromic) in the order of the lines, the md5 of the lines, and
the reference's error text where the run is an error.  The pure-Python model
(tests/extend_edist_model.py), fed with the seed lists of the CPU oracle,
must reproduce every recorded list, order included, or nothing is written.
The model goes through hundreds of thousands of seeds; they are dealt out to
worker processes.
"""
import json
import multiprocessing
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import helpers as H  # noqa: E402
import extend_edist_cases as DC  # noqa: E402
import extend_edist_model as DM  # noqa: E402
import extend_model as EM  # noqa: E402
from make_golden_extend import prepare  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MAXROWS = 6000
WORKERS = min(16, os.cpu_count() or 1)

_job = None


def _piece(bounds):
    r, seeds, tis, numofchars, triple = _job
    return DM.extend(seeds[bounds[0]:bounds[1]], tis, numofchars, r["L"],
                     r["K"], r["S"], triple)


def model_rows(r):
    global _job
    idx, _ = DC.load(r)
    parts = []
    for pal, queries in DC.passes(r):
        seeds = DC.oracle_seeds(r, queries)
        triple = None if queries is None else (queries.symbols, queries.start,
                                               queries.length)
        _job = (r, seeds, idx.tis, idx.numofchars, triple)
        step = max(1, (len(seeds) + 8 * WORKERS - 1) // (8 * WORKERS))
        cuts = [(a, min(a + step, len(seeds)))
                for a in range(0, len(seeds), step)]
        # (fork: the workers see _job)
        with multiprocessing.get_context("fork").Pool(WORKERS) as pool:
            recs = pool.map(_piece, cuts)
        rec = np.concatenate(recs) if recs else np.zeros(0, EM.MATCH_DTYPE)
        parts.append(DC.rows_of(r, rec, pal))
    return np.concatenate(parts)


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    manifest, arrays = {}, {}
    for r in DC.RUNS:
        wd = tempfile.mkdtemp()
        prepare(r, wd)
        args = DC.vmatch_args(r) + (["-q", "q.fna"] if r["q"] else []) + \
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
            rows = DC.parse_rows(lines)
            got = model_rows(r)
            assert np.array_equal(got, rows), \
                (r["key"], len(got), len(rows))
            arrays[r["key"]] = rows.astype(np.int32)
            entry["lines"] = len(lines)
            entry["md5_lines"] = DC.md5(("\n".join(lines) + "\n").encode())
            entry["maxdistance"] = int(rows[:, 6].max())
            entry["maxlength"] = int(max(rows[:, 0].max(), rows[:, 3].max()))
            entry["unequal"] = int((rows[:, 0] != rows[:, 3]).sum())
        manifest[r["key"]] = entry
        print(r["key"], entry.get("lines"), entry.get("stderr", ""),
              flush=True)
    np.savez_compressed(GOLD + "/extend_edist_expected.npz", **arrays)
    with open(GOLD + "/extend_edist_manifest.json", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", len(arrays), "lists")


if __name__ == "__main__":
    main()

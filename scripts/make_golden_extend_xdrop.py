#!/usr/bin/env python3
"""Generates the fixtures of the X-drop extension under tests/golden/ from the
REAL reference: what vmatch prints for -l L -hxdrop X | -exdrop X
[-seedlength S] with and without -q on the golden inputs that are there
already (the cases of tests/extend_cases.py).

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_extend_xdrop.py

Writes tests/golden/extend_xdrop_manifest.json and extend_xdrop_expected.npz
-- DATA only.  Every run is described by a recipe (tests/extend_xdrop_cases.py:
RUNS).  Stored per run: the rows (length1, seq1, rel1, length2, seq2, rel2,
distance, palindromic) in the order of the lines, the md5 of the lines, and
the reference's error text where the run is an error.  The pure-Python model
(tests/extend_xdrop_model.py), fed with the seed lists of the CPU oracle, must
reproduce every recorded list, order included, or nothing is written; the
seeds are dealt out to worker processes.
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
import extend_xdrop_cases as XC  # noqa: E402
import extend_xdrop_model as XM  # noqa: E402
import extend_model as EM  # noqa: E402
from make_golden_extend import prepare  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MAXROWS = 6000
WORKERS = min(16, os.cpu_count() or 1)

_job = None


def _piece(bounds):
    r, seeds, tis, triple = _job
    trace = {}
    rec = XM.extend(seeds[bounds[0]:bounds[1]], tis, r["L"], r["X"],
                    r["hamming"], r["S"], triple,
                    **({} if r["hamming"] else {"trace": trace}))
    return rec, trace


def model_rows(r):
    """-> (rows, seeds, what the edit generations saw)"""
    global _job
    idx, _ = XC.load(r)
    parts, nseeds, seen = [], 0, {}
    for pal, queries in XC.passes(r):
        seeds = XC.oracle_seeds(r, queries)
        nseeds += len(seeds)
        triple = None if queries is None else (queries.symbols, queries.start,
                                               queries.length)
        _job = (r, seeds, idx.tis, triple)
        step = max(1, (len(seeds) + 8 * WORKERS - 1) // (8 * WORKERS))
        cuts = [(a, min(a + step, len(seeds)))
                for a in range(0, len(seeds), step)]
        # (fork: the workers see _job)
        with multiprocessing.get_context("fork").Pool(WORKERS) as pool:
            done = pool.map(_piece, cuts)
        recs = [d[0] for d in done]
        for _, t in done:
            for k, v in t.items():
                seen[k] = seen.get(k, 0) + v if k == "sepreads" else \
                    max(seen.get(k, 0), v)
        rec = np.concatenate(recs) if recs else np.zeros(0, EM.MATCH_DTYPE)
        parts.append(XC.rows_of(r, rec, pal))
    return np.concatenate(parts), nseeds, seen


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    manifest, arrays = {}, {}
    for r in XC.RUNS:
        wd = tempfile.mkdtemp()
        prepare(r, wd)
        args = XC.vmatch_args(r) + (["-q", "q.fna"] if r["q"] else []) + \
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
            rows = XC.parse_rows(lines)
            got, nseeds, seen = model_rows(r)
            assert np.array_equal(got, rows), \
                (r["key"], len(got), len(rows))
            arrays[r["key"]] = rows.astype(np.int32)
            entry["lines"] = len(lines)
            entry["seeds"] = nseeds
            entry["md5_lines"] = XC.md5(("\n".join(lines) + "\n").encode())
            entry["maxdistance"] = int(np.abs(rows[:, 6]).max())
            entry["maxlength"] = int(max(rows[:, 0].max(), rows[:, 3].max()))
            entry["unequal"] = int((rows[:, 0] != rows[:, 3]).sum())
            entry.update(seen)
        manifest[r["key"]] = entry
        print(r["key"], entry.get("lines"), entry.get("stderr", ""),
              flush=True)
    good = [e for e in manifest.values() if "lines" in e]
    # what the recorded runs must show between them
    assert any(not e["hamming"] and e["unequal"] > 0 for e in good)
    assert any(e["hamming"] and e["lines"] < e["seeds"] for e in good)
    assert any(not e["hamming"] and e["sepreads"] > 0 for e in good)
    np.savez_compressed(GOLD + "/extend_xdrop_expected.npz", **arrays)
    with open(GOLD + "/extend_xdrop_manifest.json", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", len(arrays), "lists")


if __name__ == "__main__":
    main()

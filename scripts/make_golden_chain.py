#!/usr/bin/env python3
"""Generates the chaining fixtures under tests/golden/ from the REAL
reference: what vmatch prints with -pp chain ... on the index of
tests/golden/at1MB.gz, on that of micro_db.fna with -q micro_q.fna, and on
that of chain_ties.fna.

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_chain.py

Writes tests/golden/chain_manifest.json and chain_expected.npz -- DATA only.
Every run is a recipe of tests/chain_cases.py (RUNS).  The lists are those of
matchcluster_expected.npz and are not stored again (the reference is asked
for each once more and must print the stored rows); only the list of
chain_ties.fna is new.  Stored per run: the chain table (problem, number
within the problem, score, start in the member array), the members as record
numbers, and the md5 of the bytes printed behind the "# args=" line.  The
pure-Python model (tests/chain_model.py) must reproduce every recorded answer
with both of its forms, the literal sweep and the rule without an order of
events, or nothing is written.  At least one grouped run must print another
text when the grouping is replaced by a stable sort: chain_ties.fna exists
for that (one motif four times in its first sequence and once in each of
four others: a run of 22 records on seqnum1 = 0 with ties on position2).
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
import cluster_cases as CC  # noqa: E402
import chain_cases as CS  # noqa: E402
import vstree_amd as V  # noqa: E402
from make_golden_cluster import run_ref, data_lines  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    wd = tempfile.mkdtemp()
    with gzip.open(GOLD + "/at1MB.gz", "rb") as f, \
            open(wd + "/at1MB", "wb") as g:
        g.write(f.read())
    for name in ("micro_db.fna", "micro_q.fna", CS.TIES_DB):
        shutil.copy(os.path.join(GOLD, name), wd)
    for db in ("at1MB", "micro_db.fna", CS.TIES_DB):
        H.run_mkvtree_ref(["-indexname", db + ".idx", "-db", db, "-pl",
                           "-dna", "-bwt", "-lcp", "-suf", "-ois", "-tis",
                           "-bck", "-sti1"], wd)
    manifest, arrays, lists = {}, {}, {}
    orderseen = []
    for r in CS.RUNS:
        key, s = r["key"], CS.source(r)
        index = s["db"].replace(".gz", "") + ".idx"
        if r["src"] not in lists:
            rows = CC.parse_rows(data_lines(run_ref(CS.list_args(r) +
                                                    [index], wd)))
            if r["src"] == "ties":
                arrays["ties__in"] = rows.astype(np.int32)
                CS._arrays = arrays
            else:
                assert np.array_equal(rows, CS.rows_of(r)), key
            lists[r["src"]] = rows
        rec, flags = CS.input_of(key)
        lines = CS.lines_of(V, r, rec, flags)
        text = run_ref(CS.list_args(r) + CS.chain_args(r) + [index], wd)
        got = {form: CS.model_of(r, rec, flags, form=form)
               for form in ("sweep", "rule")}
        arr = CS.as_arrays(got["sweep"])
        for form in got:
            assert got[form]["stats"] == got["sweep"]["stats"], (key, form)
            other = CS.as_arrays(got[form])
            for k in arr:
                assert np.array_equal(arr[k], other[k]), (key, form, k)
            assert CS.text_of(other, lines, r["silent"]) == text, (key, form)
        st = got["sweep"]["stats"]
        if st["replayed"] > 0:
            stable = CS.as_arrays(CS.model_of(r, rec, flags, stable=True))
            if CS.text_of(stable, lines, r["silent"]) != text:
                orderseen.append(key)
        print(key, st)
        for k in arr:
            arrays[key + "__" + k] = arr[k]
        manifest[key] = dict(args=CS.list_args(r) + CS.chain_args(r),
                             stats=st, md5_text=CS.md5(text))
    assert orderseen, "no run in which the order of the quicksort shows"
    print("the quicksort's order shows in", orderseen)
    shutil.rmtree(wd)
    np.savez_compressed(GOLD + "/chain_expected.npz", **arrays)
    with open(GOLD + "/chain_manifest.json", "w") as f:
        json.dump(dict(runs=manifest, order_matters=orderseen), f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print("wrote", len(arrays), "arrays for", len(manifest), "runs")


if __name__ == "__main__":
    main()

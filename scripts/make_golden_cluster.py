#!/usr/bin/env python3
"""Generates the clustering fixtures under tests/golden/ from the REAL
reference: what vmatch prints with -dbcluster percsmall perclarge on the
index of tests/golden/at1MB.gz (1952 sequences), and the order of the lines
of the per-cluster match files it writes with a file name prefix.

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_cluster.py

Writes tests/golden/cluster_manifest.json and cluster_expected.npz -- DATA
only.  Every run is a recipe of tests/cluster_cases.py (RUNS).  Stored per
run: the list the clusterer sees as rows (length, seq1, rel1, seq2, rel2,
palindromic) -- what vmatch prints for the same options without -dbcluster --,
the member lists in output numbering, the md5 of the bytes printed behind the
"# args=" line, the counts, and for the run with a prefix the rows of every
PREFIX.size.cnum.match in the order of their lines.  The pure-Python model
(tests/cluster_model.py) must reproduce every recorded answer with both of
its replays, and see the number of forest edges the recipe names, or nothing
is written.
"""
import glob
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
import cluster_model as CM  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def run_ref(args, wd):
    """-> the bytes behind the "# args=" line"""
    p = H.subprocess.run([H.VMATCH_REF] + args, cwd=wd,
                         stdout=H.subprocess.PIPE, stderr=H.subprocess.PIPE)
    assert p.returncode == 0, (args, p.stderr.decode())
    first, _, rest = p.stdout.partition(b"\n")
    assert first.startswith(b"# args="), first
    return rest


def data_lines(text):
    return [l for l in text.decode().splitlines()
            if l and not l.startswith("#")]


def parse_clusters(text):
    out = []
    for l in data_lines(text):
        num, _, mem = l.partition(":")
        assert int(num) == len(out), l
        out.append([int(x) for x in mem.split()])
    return out


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    wd = tempfile.mkdtemp()
    with gzip.open(GOLD + "/at1MB.gz", "rb") as f, \
            open(wd + "/at1MB", "wb") as g:
        g.write(f.read())
    H.run_mkvtree_ref(["-indexname", "atindex", "-db", "at1MB", "-pl", "-dna",
                       "-bwt", "-lcp", "-suf", "-ois", "-tis", "-bck",
                       "-sti1"], wd)
    lay = CC.model_layout()
    manifest, arrays = {}, {}
    for r in CC.RUNS:
        key = r["key"]
        listargs = CC.engine_args(r) + CC.select_args(r)
        rows = CC.parse_rows(data_lines(run_ref(listargs + ["atindex"], wd)))
        rec, flags = CC.records_of(rows)
        assert np.array_equal(CC.rows_of(rec, flags), rows)
        args = CC.engine_args(r) + CC.cluster_args(r) + CC.select_args(r)
        text = run_ref(args + ["atindex"], wd)
        want = parse_clusters(text)
        full = CM.cluster(lay, rec, flags, r["percsmall"], r["perclarge"])
        forest = CM.cluster(lay, rec, flags, r["percsmall"], r["perclarge"],
                            replay=CM.forest_replay)
        for got in (full, forest):
            assert got["clusters"] == want, key
            assert got["text"] == text, key
        assert full["stats"] == forest["stats"], key
        assert np.array_equal(full["edgerecord"], forest["edgerecord"])
        st = full["stats"]
        if r["forest"] is not None:
            assert st["forestedges"] == r["forest"], (key, st)
        print(key, st)
        arrays[key + "__in"] = rows.astype(np.int32)
        arrays[key + "__clusterstart"] = full["clusterstart"]
        arrays[key + "__members"] = full["members"]
        entry = dict(args=args, lines=len(rows), stats=st,
                     md5_text=CC.md5(text),
                     largest=max([len(m) for m in want] or [0]))
        if r["edgefiles"]:
            prefix = os.path.join(wd, "cl")
            text2 = run_ref(CC.engine_args(r) + CC.cluster_args(r) +
                            [prefix, "(1,0)", "atindex"], wd)
            assert parse_clusters(text2) == want
            erows, estart = [], [0]
            for c, mem in enumerate(want):
                name = "%s.%d.%d.match" % (prefix, len(mem), c)
                with open(name) as f:
                    lines = [l for l in f.read().splitlines()
                             if l and not l.startswith("#")]
                erows.append(CC.parse_rows(lines))
                estart.append(estart[-1] + len(lines))
            assert len(glob.glob(prefix + ".*.match")) == len(want)
            erows = np.concatenate(erows)
            # the model puts the same records in the same order
            assert np.array_equal(rows[full["edgerecord"].astype(np.int64)],
                                  erows), key
            assert np.array_equal(full["edgestart"], estart), key
            arrays[key + "__edgerows"] = erows.astype(np.int32)
            arrays[key + "__edgestart"] = np.array(estart, np.uint64)
            entry["edgefiles"] = len(want)
        manifest[key] = entry
    shutil.rmtree(wd)
    np.savez_compressed(GOLD + "/cluster_expected.npz", **arrays)
    with open(GOLD + "/cluster_manifest.json", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", len(arrays), "arrays for", len(manifest), "runs")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates the erate fixtures under tests/golden/ from the REAL reference:
what vmatch prints with -pp matchcluster erate E outprefix PREFIX on the index
of tests/golden/at1MB.gz, and the files PREFIX.size.cnum.match it writes.

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_matchcluster_erate.py

Writes tests/golden/matchcluster_erate_manifest.json and
matchcluster_erate_expected.npz -- DATA only.  Every run is a recipe of
tests/erate_cases.py (RUNS).  Stored per run: the member lists in output
numbering, the edges of every cluster in the order of its file with their
values (minlen << 32 | distance), the md5 of the bytes printed behind the
"# args=" line and the md5 of every cluster file behind its first line (which
holds an absolute path).  The list of -l 100 is stored as rows; the other
lists are those of matchcluster_expected.npz, and the script checks that the
reference still prints them.  The edges of the two largest runs are left out
of the archive: their counts and md5s stay.  The pure-Python model
(tests/erate_model.py) must reproduce every recorded answer with both
replays, or nothing is written.
"""
import gzip
import json
import os
import re
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
import matchcluster_cases as MC  # noqa: E402
import erate_cases as EC  # noqa: E402
import erate_model as EM  # noqa: E402
from make_golden_cluster import run_ref, data_lines  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
LINKED = re.compile(r"# linked (\d+) and (\d+) with edit distance (\d+) "
                    r"\(error rate ([0-9.]+)%\)$")


def parse_file(body):
    """the bytes behind the first line -> (ids, match lines, edges)"""
    ids, lines, edges = [], [], []
    for l in body.decode().splitlines():
        m = LINKED.match(l)
        if m:
            edges.append((int(m.group(1)), int(m.group(2)), int(m.group(3)),
                          m.group(4)))
        elif l.startswith("# id "):
            ids.append(int(l[5:]))
        else:
            lines.append(l)
    return ids, lines, edges


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    wd = tempfile.mkdtemp()
    with gzip.open(GOLD + "/at1MB.gz", "rb") as f, \
            open(wd + "/at1MB", "wb") as g:
        g.write(f.read())
    H.run_mkvtree_ref(["-indexname", "at1MB.idx", "-db", "at1MB", "-pl",
                       "-dna", "-bwt", "-lcp", "-suf", "-ois", "-tis", "-bck",
                       "-sti1"], wd)
    manifest, arrays = {}, {}
    for r in EC.RUNS:
        key, L = r["key"], r["L"]
        rows = CC.parse_rows(data_lines(run_ref(EC.list_args(r) +
                                                ["at1MB.idx"], wd)))
        if L in EC.OWNLISTS:
            arrays["l%d__in" % L] = rows.astype(np.int32)
        else:
            assert np.array_equal(rows, MC.array("l%d__in" % L)), key
        rec, flags = CC.records_of(rows)
        assert not flags.any()
        prefix = os.path.join(wd, key)
        text = run_ref(EC.list_args(r) + EC.cluster_args(r, prefix) +
                       ["at1MB.idx"], wd)
        full = EC.model_of(r, rec)
        forest = EC.model_of(r, rec, replay=CM.forest_replay)
        st = full["stats"]
        assert (st["matches"], st["edges"], st["clusters"]) == \
            (r["matches"], r["edges"], r["clusters"]), (key, st)
        assert max(int(v) & 0xFFFFFFFF for v in full["values"]) == \
            r["largest"], key
        for got in (full, forest):
            assert got["text"] == text, key
            assert got["clusters"] == full["clusters"]
            assert got["edges"] == full["edges"]
        md5_files = []
        for c, mem in enumerate(full["clusters"]):
            with open("%s.%d.%d.match" % (prefix, len(mem), c), "rb") as f:
                first, _, body = f.read().partition(b"\n")
            assert first.startswith(b"# args="), first
            ids, lines, edges = parse_file(body)
            assert ids == mem, (key, c)
            want = [(a, b, v & 0xFFFFFFFF,
                     "%.2f" % (100.00 * float(v & 0xFFFFFFFF) / (v >> 32)))
                    for a, b, v in full["edges"][c]]
            assert edges == want, (key, c)
            assert EM.format_cluster(mem, lines, full["edges"][c]) == body, \
                (key, c)
            md5_files.append(EC.md5(body))
        print(key, st)
        stored = [key + "__clusterstart", key + "__members",
                  key + "__edgestart"]
        arrays[stored[0]] = full["clusterstart"]
        arrays[stored[1]] = full["members"]
        arrays[stored[2]] = full["edgestart"]
        if key not in EC.NOEDGES:
            arrays[key + "__m0"] = full["m0"]
            arrays[key + "__m1"] = full["m1"]
            arrays[key + "__values"] = full["values"]
            stored += [key + "__m0", key + "__m1", key + "__values"]
        manifest[key] = dict(args=EC.list_args(r) +
                             EC.cluster_args(r, "PREFIX"), stats=st,
                             md5_text=EC.md5(text), md5_files=md5_files,
                             stored=stored)
    shutil.rmtree(wd)
    np.savez_compressed(GOLD + "/matchcluster_erate_expected.npz", **arrays)
    with open(GOLD + "/matchcluster_erate_manifest.json", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(arrays), "arrays for", len(manifest), "runs")


if __name__ == "__main__":
    main()

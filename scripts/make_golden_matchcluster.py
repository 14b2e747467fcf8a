#!/usr/bin/env python3
"""Generates the match clustering fixtures under tests/golden/ from the REAL
reference: what vmatch prints with -pp matchcluster gapsize G | overlap P
outprefix PREFIX on the index of tests/golden/at1MB.gz (and, with -q
micro_q.fna, on that of micro_db.fna), and the files PREFIX.size.cnum.match
it writes.

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_matchcluster.py

Writes tests/golden/matchcluster_manifest.json and matchcluster_expected.npz
-- DATA only.  Every run is a recipe of tests/matchcluster_cases.py (RUNS).
Stored per run: the list as rows (once per -l L), the member lists in output
numbering, the edges of every cluster in the order of its file with their
values (gaps as integers, overlaps as the printed strings), the md5 of the
bytes printed behind the "# args=" line and the md5 of every cluster file
behind its first line (which holds an absolute path).  The edges of
l20_overlap1 (118 628 of them) are left out of the archive: its counts and
md5s stay.  The pure-Python model (tests/matchcluster_model.py) must
reproduce every recorded answer with both of its replays, or nothing is
written.

Three runs pin the query-side view of a record (position2 a query coordinate
on the axis of position1, counted from the other end for a P record): the -q
run on micro_db.fna / micro_q.fna, the same with -d -p, and -d -p -l 30
gapsize 50 on at1MB.  The reference accepts the last one (3 033 matches).  Its
P half comes from the pass of the index against its own reverse complement,
which prints one of two mirror images only; the list as printed is clustered
under a plain layout against queries with the index's own sequences as the
query set (tests/matchcluster_cases.py), not under the selfpalindromic
layout, which vsa_matchcluster_open refuses.
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
import matchcluster_model as MM  # noqa: E402
from make_golden_cluster import run_ref, data_lines  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
LINKED = re.compile(r"# linked (\d+) and (\d+) with "
                    r"(?:gapsize (\d+)|overlap percentage ([0-9.]+))$")
NOEDGES = ("l20_overlap1",)


def parse_file(body):
    """the bytes behind the first line -> (ids, match lines, edges)"""
    ids, lines, edges = [], [], []
    for l in body.decode().splitlines():
        m = LINKED.match(l)
        if m:
            edges.append((int(m.group(1)), int(m.group(2)),
                          int(m.group(3)) if m.group(3) else m.group(4)))
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
    for name in ("micro_db.fna", "micro_q.fna"):
        shutil.copy(os.path.join(GOLD, name), wd)
    for db in ("at1MB", "micro_db.fna"):
        H.run_mkvtree_ref(["-indexname", db + ".idx", "-db", db, "-pl",
                           "-dna", "-bwt", "-lcp", "-suf", "-ois", "-tis",
                           "-bck", "-sti1"], wd)
    manifest, arrays = {}, {}
    for r in MC.RUNS:
        key, L = r["key"], r["L"]
        index = r["db"].replace(".gz", "") + ".idx"
        rows = CC.parse_rows(data_lines(run_ref(MC.list_args(r) + [index],
                                                wd)))
        rec, flags = MC.records_of(r, rows)
        prefix = os.path.join(wd, key)
        text = run_ref(MC.list_args(r) + MC.cluster_args(r, prefix) +
                       [index], wd)
        full = MC.model_of(r, rec, flags)
        forest = MC.model_of(r, rec, flags, replay=CM.forest_replay)
        st = full["stats"]
        assert (st["matches"], st["edges"], st["clusters"]) == \
            (r["matches"], r["edges"], r["clusters"]), (key, st)
        md5_files = []
        pid = MM.printed_ids([int(f) for f in flags])
        for got in (full, forest):
            assert got["text"] == text, key
            assert got["clusters"] == full["clusters"]
            assert got["edges"] == full["edges"]
        for c, mem in enumerate(full["clusters"]):
            with open("%s.%d.%d.match" % (prefix, len(mem), c), "rb") as f:
                first, _, body = f.read().partition(b"\n")
            assert first.startswith(b"# args="), first
            ids, lines, edges = parse_file(body)
            assert ids == [pid[m] for m in mem], (key, c)
            want = [(pid[a], pid[b], v if r["mode"] == MM.GAP else "%.2f" % v)
                    for a, b, v in full["edges"][c]]
            assert edges == want, (key, c)
            assert MM.format_cluster(r["mode"], mem, lines, full["edges"][c],
                                     pid) == body, (key, c)
            md5_files.append(MC.md5(body))
        print(key, st)
        arrays[MC.input_name(r)] = rows.astype(np.int32)
        stored = [key + "__clusterstart", key + "__members",
                  key + "__edgestart"]
        arrays[stored[0]] = full["clusterstart"]
        arrays[stored[1]] = full["members"]
        arrays[stored[2]] = full["edgestart"]
        if key not in NOEDGES:
            arrays[key + "__m0"] = full["m0"]
            arrays[key + "__m1"] = full["m1"]
            arrays[key + "__values"] = full["values"] \
                if r["mode"] == MM.GAP else np.array(
                    ["%.2f" % v for v in full["values"].view(np.float64)])
            stored += [key + "__m0", key + "__m1", key + "__values"]
        manifest[key] = dict(args=MC.list_args(r) +
                             MC.cluster_args(r, "PREFIX"), stats=st,
                             md5_text=MC.md5(text), md5_files=md5_files,
                             stored=stored)
    shutil.rmtree(wd)
    np.savez_compressed(GOLD + "/matchcluster_expected.npz", **arrays)
    with open(GOLD + "/matchcluster_manifest.json", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(arrays), "arrays for", len(manifest), "runs")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates the fixtures of the scan without an index under tests/golden/
from the REAL reference: what vmatch prints for -online -complete [remred]
[-e K | -h K] -q Q IDX on the golden inputs that are there already, with the
query files of the cases or with reads drawn from the texts by the fixed-seed
recipes of tests/online_cases.py.

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_online.py

Writes tests/golden/online_manifest.json and online_expected.npz -- DATA only.
Stored per run: the rows (length1, seq1, rel1, length2, seq2, rel2, distance,
palindromic) in the order of the lines, the md5 of the lines, and what the
scan showed (below).  The pure-Python model (tests/online_model.py) must
reproduce every recorded list, order included, or nothing is written; the
(run, pass, query) triples are dealt out to worker processes.
"""
import gzip
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
import helpers as H  # noqa: E402
import online_cases as OC  # noqa: E402
import online_model as OM  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MAXROWS = 6000
WORKERS = min(16, os.cpu_count() or 1)


def unpack(name, dst):
    src = os.path.join(GOLD, name)
    if name.endswith(".gz"):
        with gzip.open(src, "rb") as f, open(dst, "wb") as g:
            g.write(f.read())
    else:
        shutil.copy(src, dst)


def prepare(r, wd):
    t = OC.text_of(r)
    assert len(t.files) == 1
    unpack(t.files[0], wd + "/db.fna")
    # the scan maps the text alone; -tis -ois is all mkvtree has to write
    H.run_mkvtree_ref(["-indexname", "db.fna", "-db", "db.fna", "-dna", "-pl",
                       "-tis", "-ois"], wd)
    assert H.read_prj(wd + "/db.fna.prj")["totallength"] == t.n
    with open(wd + "/q.fna", "w") as f:
        f.write(OC.reads_fasta(OC.reads_of(r)))


def _one(job):
    key, pal, i = job
    r = OC.run_of(key)
    t = OC.text_of(r)
    q = dict(OC.passes(r))[pal]
    info = {}
    rows = OM.query_matches(t.tis, q.seq(i), r["mode"], r["K"], r["percent"],
                            r["remred"], info)
    return key, pal, i, rows, info.get("dropped", 0)


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    recorded = {}
    for r in OC.RUNS:
        wd = tempfile.mkdtemp()
        prepare(r, wd)
        args = OC.vmatch_args(r) + ["-q", "q.fna", "db.fna"]
        rc, lines, err = H.run_vmatch_ref(args, wd)
        shutil.rmtree(wd)
        assert rc == 0, (r["key"], err)
        assert (r["key"] in OC.EMPTY) == (len(lines) == 0) and \
            len(lines) <= MAXROWS, (r["key"], len(lines))
        recorded[r["key"]] = (args, lines)
        print(r["key"], len(lines), flush=True)
    jobs = [(r["key"], pal, i) for r in OC.RUNS for pal, q in OC.passes(r)
            for i in range(q.nq)]
    with multiprocessing.get_context("fork").Pool(WORKERS) as pool:
        done = pool.map(_one, jobs, chunksize=1)
    manifest, arrays = {}, {}
    for r in OC.RUNS:
        key = r["key"]
        args, lines = recorded[key]
        rows = OC.parse_rows(lines)
        t, q = OC.text_of(r), OC.reads_of(r)
        parts, dropped = [], 0
        for k, pal, i, got, d in done:
            if k != key:
                continue
            rec = np.zeros(len(got), H.MATCH_DTYPE)
            for j, (length, pos, dist) in enumerate(got):
                rec[j] = (length, pos, i, abs(dist))
            parts.append(OC.rows_of(r, rec, pal))
            dropped += d
        model = np.concatenate(parts).reshape(-1, 8)
        assert np.array_equal(model, rows), (key, len(model), len(rows))
        entry = dict(r, args=args, lines=len(lines),
                     md5_lines=OC.md5(("\n".join(lines) + "\n").encode()))
        del entry["key"]
        m = rows[:, 3]
        k = np.array([OM.threshold_of(int(x), r["K"], r["percent"])
                      for x in m])
        # what the scan showed
        entry["dropped"] = int(dropped)
        entry["cutbyend"] = int(sum(
            1 for row, kk in zip(rows, k) if r["mode"] == OC.EDIST and
            t.n - abs_pos(t, row) < int(row[3]) + int(kk)))
        entry["abovethreshold"] = int((np.abs(rows[:, 6]) > k).sum())
        entry["thresholds"] = sorted(set(int(x) for x in k))
        entry["lengths"] = sorted(set(int(x) for x in m))
        entry["wildvswild"] = int(sum(
            1 for row in rows if r["mode"] == OC.HAMMING and
            wild_faces_wild(t, q, row)))
        entry["rawhits"] = int(sum(
            1 for row in rows if r["mode"] == OC.EDIST and row[3] > 64 and
            (q.seq(int(row[4])) == OC.WILD).any() and
            (t.tis[abs_pos(t, row):abs_pos(t, row) + int(row[0])] ==
             OC.WILD).any()))
        manifest[key] = entry
        arrays[key] = rows.astype(np.int32)
    good = list(manifest.values())
    # what the recorded runs must show between them
    bestofrun = manifest["tandem_e2_remred"]
    assert bestofrun["dropped"] > 0 and \
        not same_as_best_of_run("tandem_e2_remred", "tandem_e2", arrays)
    assert any(e["cutbyend"] > 0 for e in good)
    assert any(e["wildvswild"] > 0 for e in good)
    assert any(e["rawhits"] > 0 for e in good)
    assert exact_suppressed(arrays)
    assert any(0 in e["thresholds"] and e["mode"] == OC.EDIST for e in good)
    assert {32, 33, 64, 65, 130} <= set(manifest["at1mb_e2"]["lengths"])
    np.savez_compressed(GOLD + "/online_expected.npz", **arrays)
    with open(GOLD + "/online_manifest.json", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", len(arrays), "lists")


def abs_pos(t, row):
    starts = np.concatenate(([0], t.ssp + 1)).astype(np.int64)
    return int(starts[int(row[1])]) + int(row[2])


def wild_faces_wild(t, q, row):
    a = abs_pos(t, row)
    s = q.seq(int(row[4]))
    if row[7]:
        return False
    w = t.tis[a:a + len(s)]
    return bool(((w == OC.WILD) & (s == OC.WILD)).any())


def same_as_best_of_run(remred_key, plain_key, arrays):
    """would "the best of each maximal run of adjacent start positions" give
    the list remred gave?"""
    plain, rem = arrays[plain_key], arrays[remred_key]
    r = OC.run_of(plain_key)
    t = OC.text_of(r)
    best, run = [], []

    def close():
        if run:
            # the smallest distance, the leftmost among equals
            best.append(min(run, key=lambda x: (x[1], x[0]))[0])
    for row in plain:
        p = (int(row[4]), abs_pos(t, row))
        if run and (run[-1][2] != p[0] or run[-1][0] != p[1] + 1):
            close()
            run = []
        run.append((p[1], int(row[6]), p[0]))
    close()
    return sorted(best) == sorted(abs_pos(t, row) for row in rem)


def exact_suppressed(arrays):
    """an exact run in which a wildcard of the text suppressed a match: a
    window that equals the pattern byte for byte, wildcards included, and is
    not reported"""
    for r in OC.RUNS:
        if r["mode"] != OC.EXACT:
            continue
        t, q = OC.text_of(r), OC.reads_of(r)
        rows = arrays[r["key"]]
        found = {(int(row[4]), abs_pos(t, row)) for row in rows}
        for i in range(q.nq):
            s = q.seq(i)
            if not (s == OC.WILD).any() or len(s) > t.n:
                continue
            win = np.lib.stride_tricks.sliding_window_view(t.tis, len(s))
            for a in np.flatnonzero((win == s).all(axis=1)):
                if (i, int(a)) not in found:
                    return True
    return False


if __name__ == "__main__":
    main()

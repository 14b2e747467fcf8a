#!/usr/bin/env python3
"""Records what the REAL reference prints for the repeat family on the
constructed texts of tests/repeat_cases.py: vmatch -l L IDX, -supermax -l L
and -tandem -l L on indexes its own mkvtree built.

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_repeat_edges.py

Writes tests/golden/repeat_edges_manifest.json and repeat_edges_expected.npz
-- DATA only.  Per text: its md5 (so that builder and fixture cannot drift),
the mkvtree arguments, the md5 of every table mkvtree wrote.  Per run: the
arguments, the return code, the error text without the program's path, the
number of lines and their md5, the md5 of the parsed integers; the parsed
list itself (columns length, dbseq, dbrel, queryseq, querystart) unless it
has more than MAXLINES lines.
"""
import hashlib
import io
import json
import os
import shutil
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import helpers as H  # noqa: E402
import repeat_cases as RC  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MAXLINES = 5000
ENGINE_ARGS = {"repeats": [], "supermax": ["-supermax"],
               "tandem": ["-tandem"]}
COLUMNS = ("length", "dbseq", "dbrel", "queryseq", "querystart")


def run_key(engine, L):
    return "%s%d" % (engine, L)


def as_columns(m):
    """parse_vmatch_lines / *_as_ref records -> (k, 5) uint64"""
    return np.stack([m[k].astype(np.uint64) for k in COLUMNS],
                    axis=1).reshape(len(m), 5)


def md5_parsed(cols):
    return hashlib.md5(np.ascontiguousarray(cols, "<u8").tobytes()).hexdigest()


def save_npz(path, arrays):
    """np.savez_compressed without the time of day in the archive: the same
    lists give the same file"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arrays[key], allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", (1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def prepare(case, wd):
    """FASTA files and the reference's index of a case in wd -> (mkvtree
    arguments, index name)"""
    recs = case.records()
    if case.hasqueries:
        ndb = case.numofdbsequences
        H.write_fasta(wd + "/db.fna", recs[:ndb])
        H.write_fasta(wd + "/q.fna", recs[ndb:])
        args = ["-indexname", "all", "-db", "db.fna", "-q", "q.fna", "-dna",
                "-pl", "-allout"]
        name = "all"
    else:
        H.write_fasta(wd + "/db.fna", recs)
        args = ["-db", "db.fna", "-dna", "-pl", "-allout"]
        name = "db.fna"
    H.run_mkvtree_ref(args, wd)
    return args, name


def run_reference(case, wd, name, engine, L):
    """one vmatch run -> (manifest entry, parsed columns or None)"""
    args = ENGINE_ARGS[engine] + ["-l", str(L), name]
    rc, lines, err = H.run_vmatch_ref(args, wd)
    entry = {"args": args, "rc": rc, "lines": len(lines),
             "stderr": err.split(": ", 1)[1].strip() if rc != 0 else "",
             "md5_lines": hashlib.md5(
                 ("\n".join(lines) + "\n").encode()).hexdigest()}
    if rc != 0:
        assert not lines
        return entry, None
    cols = as_columns(H.parse_vmatch_lines(lines))
    entry["md5_parsed"] = md5_parsed(cols)
    entry["stored"] = len(lines) <= MAXLINES
    return entry, cols


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    manifest, arrays = {}, {}
    for cname in RC.RECORDED:
        case = RC.case(cname)
        wd = tempfile.mkdtemp()
        mkvargs, name = prepare(case, wd)
        ref = H.load_mkvtree_index(os.path.join(wd, name))
        assert np.array_equal(ref.tis, case.tis), cname
        runs = {}
        for engine, L in case.runs():
            entry, cols = run_reference(case, wd, name, engine, L)
            runs[run_key(engine, L)] = entry
            if cols is not None and entry["stored"]:
                arrays["%s__%s" % (cname, run_key(engine, L))] = \
                    cols.astype(np.uint32)
                assert cols.max(initial=0) < 2 ** 32
        manifest[cname] = {"md5_text": case.md5(), "totallength": case.n,
                           "mkvargs": mkvargs, "indexname": name,
                           "prefixlength": ref.prefixlength,
                           "largelcpvalues": ref.nllv,
                           "md5_tables": H.table_md5(ref), "runs": runs}
        shutil.rmtree(wd)
    save_npz(GOLD + "/repeat_edges_expected.npz", arrays)
    with open(GOLD + "/repeat_edges_manifest.json", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(arrays), "lists for",
          sum(len(v["runs"]) for v in manifest.values()), "runs of",
          len(manifest), "texts")


if __name__ == "__main__":
    main()

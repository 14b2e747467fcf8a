#!/usr/bin/env python3
"""Generates the fixtures of the alignment output under tests/golden/ from the
REAL reference: what vmatch prints with -s W on inputs that are there already
(and on align_tandem.fna, a small text of tandem repeats whose self matches
overlap).

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_align.py

Writes tests/golden/align_manifest.json and align_expected.npz -- DATA only.
Every run is a recipe of tests/align_cases.py: RUNS.  Stored per run: the md5
of everything vmatch printed behind its `# args=` line, the rows of the match
lines, the text of the first matches, and the edit scripts of all matches as
the pure-Python model (tests/align_model.py) made them from the records that
the rows stand for.  The model must reproduce the whole output of the
reference byte for byte, or nothing is written: a script is trusted because
the columns it prints are the reference's.
"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import helpers as H  # noqa: E402
import align_cases as AC  # noqa: E402
import align_model as AM  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MAXROWS = 6000
FIRSTMATCHES = 40        # whose text is stored


def unpack(name, dst):
    src = os.path.join(GOLD, name)
    if name.endswith(".gz"):
        with gzip.open(src, "rb") as f, open(dst, "wb") as g:
            g.write(f.read())
    else:
        shutil.copy(src, dst)


def reference_output(r):
    """-> what vmatch printed behind the first line"""
    wd = tempfile.mkdtemp()
    try:
        db, q = AC.CASES[r["case"]]
        unpack(db, wd + "/db.fna")
        H.run_mkvtree_ref(["-indexname", "db.fna", "-db", "db.fna", "-dna",
                           "-pl", "-allout"], wd)
        args = AC.vmatch_args(r)
        if r["q"]:
            unpack(q, wd + "/q.fna")
            args += ["-q", "q.fna"]
        p = subprocess.run([H.VMATCH_REF] + args + ["db.fna"], cwd=wd,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, (r["key"], p.stderr.decode())
        head, _, body = p.stdout.partition(b"\n")
        assert head.startswith(b"# args="), head
        return body
    finally:
        shutil.rmtree(wd)


def matchlines(body):
    """the lines of the output that are match lines"""
    return [l.decode() for l in body.split(b"\n")
            if l and not l.startswith((b"Sbjct:", b"Query:", b"       "))]


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    sys.path.insert(0, ROOT)
    import vstree_amd as V
    manifest, arrays = {}, {}
    classes = dict(indel=0, palindromic=0, sametext=0, overshoot=0,
                   wildcard=0)
    for r in AC.RUNS:
        body = reference_output(r)
        lines = matchlines(body)
        assert 0 < len(lines) <= MAXROWS, (r["key"], len(lines))
        rows = AC.parse_rows(lines)
        text, scripts, first = [], [], []
        for pal, prow in AC.passes(r, rows):
            rec = AC.records_of(r, prow)
            # the match lines are the sink's; the model adds the alignments
            sink = V.Sink(**AC.sink_kwargs(V, r, pal))
            for x, pair in zip(rec, AC.pairs_of(r, rec, pal)):
                words = pair.script()
                assert words is not None, (r["key"], x)
                assert AM.consumed(words) == (len(pair.u), len(pair.v))
                one = sink.format(np.array([x])) + pair.show(words,
                                                             r["width"])
                text.append(one)
                scripts.append(words)
                if len(first) < FIRSTMATCHES:
                    first.append(one.decode())
                classes["palindromic"] += pal
                classes["indel"] += any(w in (AM.DELETIONEOP, AM.INSERTIONEOP)
                                        for w in words)
                classes["wildcard"] += bool((pair.u >= AC.WILD).any() or
                                            (pair.v >= AC.WILD).any())
                if pair.distance > 0:
                    f = AM.fronts(pair.u, pair.v, pair.distance, pair.sametext)
                    # (no matcher stores more than the real distance)
                    assert f.distance == pair.distance
                    classes["overshoot"] += AM.backtrace(f, pair.u,
                                                         pair.v)[1]
                    classes["sametext"] += (pair.sametext is not None and
                                            abs(pair.sametext) <= f.distance
                                            and f.distance > 0)
        got = b"".join(text)
        assert got == body, (r["key"], len(got), len(body),
                             next(i for i in range(min(len(got), len(body)))
                                  if got[i] != body[i]))
        offsets, words = AC.csr(scripts)
        arrays[r["key"] + "__rows"] = rows.astype(np.int32)
        arrays[r["key"] + "__offsets"] = offsets.astype(np.uint32)
        arrays[r["key"] + "__words"] = words
        manifest[r["key"]] = dict(
            case=r["case"], kind=r["kind"], args=AC.vmatch_args(r),
            matches=len(lines), bytes=len(body), md5=AC.md5(body),
            words=int(len(words)), first=first)
        print(r["key"], len(lines), len(body), flush=True)
    # every class of alignment is there, or another -l has to be picked
    assert all(v > 0 for v in classes.values()), classes
    np.savez_compressed(GOLD + "/align_expected.npz", **arrays)
    with open(GOLD + "/align_manifest.json", "w") as f:
        json.dump(dict(runs=manifest, classes=classes), f, indent=1,
                  sort_keys=True)
    for name in ("align_expected.npz", "align_manifest.json"):
        assert os.path.getsize(os.path.join(GOLD, name)) <= 400000, name
    print("wrote", len(manifest), "runs", classes)


if __name__ == "__main__":
    main()

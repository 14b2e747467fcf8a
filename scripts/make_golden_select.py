#!/usr/bin/env python3
"""Generates the selection fixtures under tests/golden/ from the REAL
reference: what vmatch prints with -best N, -sort mode, -evalue, -identity,
-leastscore and the gap bounds of -l L lo [hi] on the golden inputs that are
there already.

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_select.py

Writes tests/golden/select_manifest.json and select_expected.npz -- DATA only.
Every run is described by a recipe (tests/select_cases.py: RUNS, FILTERS) from
which both the vmatch command line and, in the tests, the calls of the engine
are derived.  Stored per run: the unselected list as rows (length, seq1, rel1,
seq2, rel2 or |distance|, palindromic); per variant of it -- two or three N
that cut the list inside a group of equal E-values, one below and one beyond
its length, six sort modes, the filters -- the selected rows in the order of
the lines, the md5 of the lines and the number of "remove %lu contained
matches".  The pure-Python model (tests/select_model.py) must reproduce every
recorded answer, order included, or nothing is written.
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
import select_cases as SC  # noqa: E402
import select_model as SM  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
# (the two -q lists of c5 are the largest: 5498 and 5933 lines)
MAXROWS = 6000


def prepare(case, wd):
    m = H.manifest()[case]

    def unpack(name, dst):
        src = os.path.join(GOLD, name)
        if name.endswith(".gz"):
            with gzip.open(src, "rb") as f, open(dst, "wb") as g:
                g.write(f.read())
        else:
            shutil.copy(src, dst)
    assert len(m["db"]) == 1
    unpack(m["db"][0], wd + "/db.fna")
    unpack(m["query"], wd + "/q.fna")
    H.run_mkvtree_ref(["-db", "db.fna", "-dna", "-pl", "-allout"], wd)


def run_ref(args, wd):
    """-> (lines, number of contained matches removed or 0)"""
    p = H.subprocess.run([H.VMATCH_REF, "-v"] + args, cwd=wd,
                         stdout=H.subprocess.PIPE, stderr=H.subprocess.PIPE)
    assert p.returncode == 0, (args, p.stderr.decode())
    lines, contained = [], 0
    for l in p.stdout.decode().splitlines():
        if l.startswith("# remove ") and l.endswith(" contained matches"):
            contained = int(l.split()[2])
        elif l and not l.startswith("#"):
            lines.append(l)
    return lines, contained


def tie_cuts(lay, rec, flags, filters):
    """N inside the two largest groups of equal E-values of the list in
    best-first order, and the length of that list"""
    order, ev, _ = SM.select(lay, rec, flags, best=len(rec) + 1, **filters)
    groups, a = [], 0
    for b in range(1, len(ev) + 1):
        if b == len(ev) or ev[b] != ev[a]:
            if b - a >= 2:
                groups.append((b - a, a))
            a = b
    groups.sort(reverse=True)
    return [a + size // 2 for size, a in groups[:2]], len(order)


def variants_of(case, i, r, lay, rec, flags):
    out = []
    cuts, total = tie_cuts(lay, rec, flags, {})
    ns = sorted(set([1] + cuts + ([total - 1] if total > 2 else []) +
                    [total + 3]))
    for n in ns:
        out.append(dict(best=n))
    nsort = cuts[0] if cuts else total
    for mode in SC.SORTSETS[i % 2]:
        out.append(dict(best=nsort, sort=mode))
    if r["approx"] and not r["approx"][0]:
        # Hamming scores are negative, the score of a match without a
        # mismatch is not: equal absolute values of different sign
        out.append(dict(best=nsort, sort="sd"))
    for mode in ("ia", SC.SORTSETS[(i + 1) % 2][i % 6]):
        out.append(dict(best=total + 3, sort=mode))
    for f in SC.FILTERS.get((case, r["key"]), []):
        out.append(dict(f))
        fcuts, ftotal = tie_cuts(lay, rec, flags,
                                 {k: v for k, v in f.items()})
        if ftotal > 1:
            out.append(dict(f, best=fcuts[0] if fcuts else ftotal - 1,
                            sort=SC.SORTSETS[i % 2][1]))
    return out


def variant_key(v):
    parts = []
    for k in ("best", "sort", "evalue", "identity", "leastscore"):
        if v.get(k) is not None:
            parts.append("%s%s" % (k, v[k]))
    if v.get("gap") is not None:
        parts.append("gap" + "_".join(str(g) for g in v["gap"]))
    return "_".join(parts).replace("-", "m")


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    manifest, arrays, nvariants = {}, {}, 0
    for case, runs in SC.RUNS.items():
        wd = tempfile.mkdtemp()
        prepare(case, wd)
        manifest[case] = {}
        for i, r in enumerate(runs):
            tail = (["-q", "q.fna"] if SC.withquery(r) else []) + ["db.fna"]
            lines, _ = run_ref(SC.engine_args(r) + tail, wd)
            assert 0 < len(lines) <= MAXROWS, (case, r["key"], len(lines))
            rows = SC.parse_rows(lines)
            rec, flags = SC.records_of(case, r, rows)
            lay = SC.model_layout(case, r)
            name = "%s__%s" % (case, r["key"])
            arrays[name + "__in"] = rows.astype(np.int32)
            entry = dict(r, lines=len(lines), variants={})
            for v in variants_of(case, i, r, lay, rec, flags):
                args = SC.engine_args(r, v.get("gap")) + SC.variant_args(v)
                vlines, contained = run_ref(args + tail, wd)
                vrows = SC.parse_rows(vlines)
                # the model reproduces the reference, order included
                sel, _, st = SM.select(lay, rec, flags, **SC.options_of(v))
                assert np.array_equal(rows[sel].reshape(-1, 6), vrows), \
                    (case, r["key"], v)
                assert st["containedremoved"] == contained, (case, r, v)
                vk = variant_key(v)
                arrays["%s__%s" % (name, vk)] = vrows.astype(np.int32)
                entry["variants"][vk] = dict(
                    v, args=args, lines=len(vlines), contained=contained,
                    md5_lines=SC.md5(("\n".join(vlines) + "\n").encode()
                                     if vlines else b""))
                nvariants += 1
            del entry["key"]
            manifest[case][r["key"]] = entry
        shutil.rmtree(wd)
    np.savez_compressed(GOLD + "/select_expected.npz", **arrays)
    with open(GOLD + "/select_manifest.json", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", len(arrays), "arrays for", nvariants, "variants")


if __name__ == "__main__":
    main()

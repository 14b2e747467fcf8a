#!/usr/bin/env python3
"""Generates the non-DNA fixtures under tests/golden/ from the REAL reference:
a protein database indexed under the 20-letter alphabet (mkvtree -protein),
under an 11-class symbol map (mkvtree -smap), and together with its queries.

Run in the build container (needs the reference programs built by
`make -f oracle/Makefile.ref`):

    python3 scripts/make_golden_alphabets.py

Writes new files only -- DATA, no program text:
  prot_db.fna.gz, prot_q.fna.gz, prot_short.fna   the inputs, from fixed seeds
  prot.al1, prot11.al1        the alphabet files the reference wrote (.al1);
                              prot11.al1 is at the same time the map handed to
                              -smap: the reference reads its own .al1 back and
                              writes the same tables (asserted below)
  alphabets_manifest.json     per case the .prj numbers, the md5 of the tables,
                              the mkvtree options; per run the vmatch options,
                              exit code, stderr and the md5 of the lines
  alphabets_expected.npz      the match lists, parsed like expected.npz
make_golden.py, make_golden_coverage.py and their files are not touched.

Every search length is chosen here and asserted: no list is empty, MEM and
maximal-repeat lists hold 100 .. 100000 matches.
"""
import gzip
import hashlib
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

GOLD = os.path.join(ROOT, "tests", "golden")
TABLES = ("tis", "suf", "lcp", "llv", "bck", "bwt", "sti1")
AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


def reference_sources():
    """where the reference's sources lie: REF of oracle/Makefile.ref, which
    built the programs used here"""
    with open(os.path.join(ROOT, "oracle", "Makefile.ref")) as f:
        for line in f:
            if line.startswith("REF") and "?=" in line:
                return os.environ.get("REF", line.split("?=")[1].strip())
    raise KeyError("REF")


# the 11-class map of the reference's own collection (Mkvtree/TRANS): read
# once, to obtain the .al1 the reference writes for it
SMAP11 = os.path.join(reference_sources(), "Mkvtree", "TRANS", "TransProt11")

# search lengths per case: (MEM / MUM, supermax x2, repeats x2, tandem x2)
LENGTHS = {"prot": dict(mem=6, mum=6, supermax=(5, 12), repeats=(6, 12),
                        tandem=(2, 5)),
           "prot11": dict(mem=8, mum=8, supermax=(8, 20), repeats=(9, 20),
                          tandem=(3, 6))}
LENGTHS_ALL = dict(selfmum=6, repeats=7)


def md5file(p):
    return hashlib.md5(open(p, "rb").read()).hexdigest()


def gzcopy(src, dst):
    with open(src, "rb") as f, gzip.GzipFile(dst, "wb", mtime=0) as g:
        g.write(f.read())


def index_case(wd, indexname, mkvargs):
    H.run_mkvtree_ref(mkvargs, wd)
    prefix = os.path.join(wd, indexname)
    prj = H.read_prj(prefix + ".prj")
    return {"prj": {k: v for k, v in prj.items()
                    if k not in ("dbfile", "queryfile")},
            "md5": {t: md5file(prefix + "." + t) for t in TABLES},
            "mkvargs": mkvargs, "indexname": indexname}


def residues(rng, n):
    return AMINO[rng.integers(0, 20, n)]


def make_database(rng):
    """about 40 sequences descending from 5 ancestors -> list of bytes"""
    anc = [residues(rng, n) for n in (180, 260, 330, 410, 480)]
    seqs = []
    for i in range(40):
        s = anc[i % 5].copy()
        rate = rng.uniform(0.05, 0.15)
        hit = np.flatnonzero(rng.random(len(s)) < rate)
        s[hit] = residues(rng, len(hit))
        for _ in range(int(rng.integers(0, 4))):      # insertions, deletions
            p, k = int(rng.integers(0, len(s) - 8)), int(rng.integers(1, 6))
            if rng.random() < 0.5:
                s = np.concatenate([s[:p], residues(rng, k), s[p:]])
            else:
                s = np.concatenate([s[:p], s[p + k:]])
        seqs.append(s)

    def plant(i, what):
        p = int(rng.integers(10, len(seqs[i]) - 10))
        seqs[i] = np.concatenate([seqs[i][:p],
                                  np.frombuffer(what, np.uint8), seqs[i][p:]])
    plant(3, b"PQ" * 12)
    plant(17, b"PQ" * 12)
    plant(8, b"GSGSG" * 6)
    plant(29, b"GSGSG" * 6)
    plant(22, b"Q" * 45)                   # a run of one residue
    for s in seqs:                         # X: the wildcard of both alphabets
        s[rng.random(len(s)) < 0.003] = ord("X")
    # a repeat copy at text position 0 and one at the very end
    seqs[0] = np.concatenate([anc[0][:60], seqs[0][60:]])
    seqs[39] = np.concatenate([seqs[39][:-60], anc[4][-60:]])
    seqs[5] = np.concatenate([seqs[5][:20], anc[0][:60], seqs[5][20:]])
    seqs[34] = np.concatenate([seqs[34][:31], anc[4][-60:], seqs[34][31:]])
    total = sum(len(s) for s in seqs)
    assert 12000 <= total <= 15000, total
    assert all(150 <= len(s) <= 640 for s in seqs)
    return [s.tobytes() for s in seqs]


def make_queries(rng, db):
    qs = []
    for i in range(400):
        m = int(rng.integers(8, 61))
        if i % 20 == 7:                    # 20 random peptides
            qs.append(residues(rng, m).tobytes())
            continue
        s = np.frombuffer(db[int(rng.integers(0, len(db)))], np.uint8)
        p = int(rng.integers(0, len(s) - m))
        q = s[p:p + m].copy()
        for _ in range(int(rng.integers(0, 3))):
            q[int(rng.integers(0, m))] = residues(rng, 1)[0]
        if i % 25 == 3:
            q[int(rng.integers(0, m))] = ord("X")
        qs.append(q.tobytes())
    assert sum(b"X" in q for q in qs) >= 10
    return qs


def main():
    if not H.have_ref():
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    rng = np.random.default_rng(20261018)
    db = make_database(rng)
    qs = make_queries(rng, db)
    # the third peptide is shorter than either prefix length: the reference's
    # hard error for -complete after the matches of the first two
    short = [db[2][40:52], db[11][7:16], b"M", db[20][100:110]]
    wd = tempfile.mkdtemp()
    H.write_fasta(wd + "/prot_db.fna", [("p%d" % i, s)
                                        for i, s in enumerate(db)])
    H.write_fasta(wd + "/prot_q.fna", [("q%d" % i, s)
                                       for i, s in enumerate(qs)])
    H.write_fasta(wd + "/prot_short.fna", [("s%d" % i, s)
                                           for i, s in enumerate(short)])
    gzcopy(wd + "/prot_db.fna", GOLD + "/prot_db.fna.gz")
    gzcopy(wd + "/prot_q.fna", GOLD + "/prot_q.fna.gz")
    shutil.copy(wd + "/prot_short.fna", GOLD + "/prot_short.fna")
    assert os.path.getsize(GOLD + "/prot_db.fna.gz") < os.path.getsize(
        GOLD + "/ychrIII.fna.gz")

    manifest, arrays = {}, {}

    def record(case, key, args, approx=False, least=1, most=None):
        rc, lines, err = H.run_vmatch_ref(args, wd)
        entry = {"args": args, "rc": rc, "lines": len(lines),
                 "md5_lines": hashlib.md5(
                     ("\n".join(lines) + "\n").encode()).hexdigest()}
        arrays["%s__%s" % (case, key)] = H.parse_vmatch_lines(lines,
                                                              approx=approx)
        if rc != 0:
            # (the program names itself by its path: keep its name only)
            entry["stderr"] = err.strip().replace(
                H.VMATCH_REF, os.path.basename(H.VMATCH_REF))
        assert len(lines) >= least, (case, key, len(lines))
        assert most is None or len(lines) <= most, (case, key, len(lines))
        manifest[case]["runs"][key] = entry
        return arrays["%s__%s" % (case, key)]

    # ---- the .al1 of the 11-class map, accepted back by -smap ------------
    H.run_mkvtree_ref(["-indexname", "first11", "-db", "prot_db.fna", "-smap",
                       SMAP11, "-pl", "-allout"], wd)
    shutil.copy(wd + "/first11.al1", wd + "/prot11.al1")

    cases = {"prot": ("prot_db.fna", ["-db", "prot_db.fna", "-protein", "-pl",
                                      "-allout"]),
             "prot11": ("p11", ["-indexname", "p11", "-db",
                                   "prot_db.fna", "-smap", "prot11.al1",
                                   "-pl", "-allout"])}
    for case, (name, mkvargs) in cases.items():
        manifest[case] = {"db": ["prot_db.fna.gz"], "query": "prot_q.fna.gz",
                          "al1": case + ".al1", "runs": {}}
        manifest[case]["index"] = index_case(wd, name, mkvargs)
        with open(wd + "/" + name + ".al1", "rb") as f:
            al1 = f.read()
        if case == "prot11":
            first = {t: hashlib.md5(open(wd + "/first11." + t, "rb").read())
                     .hexdigest() for t in manifest[case]["index"]["md5"]}
            assert first == manifest[case]["index"]["md5"]
            assert al1 == open(wd + "/first11.al1", "rb").read()
        with open(GOLD + "/" + case + ".al1", "wb") as f:
            f.write(al1)
        symmap = H.symbol_map_from_al1(GOLD + "/" + case + ".al1")
        nc = int(symmap[symmap < H.WILDCARD - 1].max()) + 1
        manifest[case]["numofchars"] = nc
        pl = manifest[case]["index"]["prj"]["prefixlength"]
        assert pl > 1, "the short peptide must be shorter than prefixlength"
        ln = LENGTHS[case]
        assert ln["mem"] >= pl
        tail = ["-q", "prot_q.fna", name]
        record(case, "complete", ["-complete", "-d"] + tail)
        record(case, "complete_short", ["-complete", "-d", "-q",
                                        "prot_short.fna", name], least=2)
        assert manifest[case]["runs"]["complete_short"]["rc"] != 0
        assert ("patternlength=1 must be >= %d=prefixlen" % pl) in \
            manifest[case]["runs"]["complete_short"]["stderr"]
        for sp in (0, 2):
            record(case, "mem%d_sp%d" % (ln["mem"], sp),
                   ["-qspeedup", str(sp), "-d", "-l", str(ln["mem"])] + tail,
                   least=100, most=100000)
        record(case, "mumcand%d" % ln["mum"],
               ["-mum", "cand", "-d", "-l", str(ln["mum"])] + tail)
        record(case, "mum%d" % ln["mum"],
               ["-mum", "-d", "-l", str(ln["mum"])] + tail)
        for L in ln["supermax"]:
            record(case, "supermax%d" % L, ["-supermax", "-d", "-l", str(L),
                                            name])
        for L in ln["repeats"]:
            rep = record(case, "repeats%d" % L, ["-d", "-l", str(L), name],
                         least=100, most=100000)
            # a repeat copy at text position 0
            assert ((rep["dbseq"] == 0) & (rep["dbrel"] == 0)).any()
        for L in ln["tandem"]:
            record(case, "tandem%d" % L, ["-tandem", "-d", "-l", str(L),
                                          name])
        record(case, "approx_e1", ["-complete", "-e", "1", "-d"] + tail,
               approx=True)
        for key, run in manifest[case]["runs"].items():
            assert (run["rc"] != 0) == (key == "complete_short"), key

    # ---- an index that holds its queries ----------------------------------
    case = "prot_all"
    manifest[case] = {"db": ["prot_db.fna.gz"],
                      "indexedquery": ["prot_q.fna.gz"], "al1": "prot.al1",
                      "numofchars": manifest["prot"]["numofchars"],
                      "runs": {}}
    manifest[case]["index"] = index_case(
        wd, "all", ["-indexname", "all", "-db", "prot_db.fna", "-q",
                    "prot_q.fna", "-protein", "-pl", "-allout"])
    assert open(wd + "/all.al1", "rb").read() == \
        open(GOLD + "/prot.al1", "rb").read()
    record(case, "selfmum%d" % LENGTHS_ALL["selfmum"],
           ["-mum", "-d", "-l", str(LENGTHS_ALL["selfmum"]), "all"])
    record(case, "repeats%d" % LENGTHS_ALL["repeats"],
           ["-d", "-l", str(LENGTHS_ALL["repeats"]), "all"], least=100,
           most=100000)
    assert manifest[case]["runs"]["selfmum6"]["rc"] == 0
    shutil.rmtree(wd)

    # np.savez_compressed stamps the archive members with the time of day:
    # fixed stamps, so that the file comes out byte for byte again
    write_npz(GOLD + "/alphabets_expected.npz", arrays)
    assert os.path.getsize(GOLD + "/alphabets_expected.npz") < 300000
    with open(GOLD + "/alphabets_manifest.json", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", len(arrays), "match lists for", len(manifest), "cases")
    for case in manifest:
        print(case, "numofchars", manifest[case]["numofchars"], "pl",
              manifest[case]["index"]["prj"]["prefixlength"],
              {k: r["lines"] for k, r in manifest[case]["runs"].items()})


def write_npz(path, arrays):
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]),
                                      allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    main()

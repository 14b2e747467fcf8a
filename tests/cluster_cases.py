"""The recorded clustering runs (tests/golden/cluster_manifest.json,
cluster_expected.npz, written by scripts/make_golden_cluster.py): the recipes
from which both the vmatch command line and the calls of the engine are
derived, and the conversions between the rows vmatch prints and the records
of the engine.  All runs are on the index of tests/golden/at1MB.gz (1952
sequences).  Shared by the generator and the two cluster test modules."""
import hashlib
import json
import os

import numpy as np

import helpers as H
import cluster_model as CM


def R(key, L, strands, percsmall, perclarge, forest, select=None,
      edgefiles=False):
    return dict(key=key, L=L, strands=strands, percsmall=percsmall,
                perclarge=perclarge, forest=forest, select=select,
                edgefiles=edgefiles)


# forest: the number of edges that join two different clusters
RUNS = [
    R("l100_50_50", 100, "d", 50, 50, 61, edgefiles=True),
    R("l30_10_5", 30, "d", 10, 5, 315),
    R("l20_5_2", 20, "d", 5, 2, 366),
    R("l14_2_1", 14, "d", 2, 1, 1598),
    R("l14_dp_2_1", 14, "dp", 2, 1, 1821),
    R("l30_dp_10_5", 30, "dp", 10, 5, 320),
    R("l30_p_10_5", 30, "p", 10, 5, 5),
    R("l30_10_5_evalue", 30, "d", 10, 5, 285, select=dict(evalue=1e-20)),
    R("l30_10_5_best20", 30, "d", 10, 5, None, select=dict(best=20)),
]


def run_of(key):
    return next(r for r in RUNS if r["key"] == key)


def keys():
    return [r["key"] for r in RUNS]


def engine_args(r):
    return ["-l", str(r["L"])] + {"d": [], "p": ["-p"],
                                  "dp": ["-d", "-p"]}[r["strands"]]


def select_args(r):
    s = r["select"] or {}
    return (["-evalue", repr(s["evalue"])] if "evalue" in s else []) + \
        (["-best", str(s["best"])] if "best" in s else [])


def cluster_args(r):
    return ["-dbcluster", str(r["percsmall"]), str(r["perclarge"])]


_text = None


def text():
    """(symbols with separators, separator positions) of at1MB"""
    global _text
    if _text is None:
        tis, ssp, _ = H.fasta_text([H._golden_fasta("at1MB.gz")])
        _text = (tis, np.asarray(ssp, np.uint64))
    return _text


def model_layout():
    tis, ssp = text()
    return CM.Layout(len(tis), ssp)


def parse_rows(lines):
    """the default columns -> rows (length, seq1, rel1, seq2, rel2,
    palindromic)"""
    out = np.zeros((len(lines), 6), np.int64)
    for i, l in enumerate(lines):
        f = l.split()
        assert int(f[0]) == int(f[4]) and int(f[7]) == 0
        out[i] = (int(f[0]), int(f[1]), int(f[2]), int(f[5]), int(f[6]),
                  1 if f[3] == "P" else 0)
    return out


def records_of(rows):
    """rows -> (engine records, D/P flags): a direct match is (length,
    start1, start2 absolute, 0), a palindromic one (length, dbstart, the
    sequence, the offset in its reverse complement)"""
    lay = model_layout()
    rows = np.asarray(rows, np.int64).reshape(-1, 6)
    pal = rows[:, 5] == 1
    rec = np.zeros(len(rows), H.MATCH_DTYPE)
    rec["length"] = rows[:, 0]
    rec["dbstart"] = lay.start[rows[:, 1]] + rows[:, 2]
    rec["queryseq"] = np.where(pal, rows[:, 3],
                               lay.start[rows[:, 3]] + rows[:, 4])
    rec["querystart"] = np.where(
        pal, lay.seqlen[rows[:, 3]] - (rows[:, 4] + rows[:, 0]), 0)
    return rec, pal.astype(np.uint8)


def rows_of(rec, flags):
    """the inverse of records_of"""
    lay = model_layout()
    out = np.zeros((len(rec), 6), np.int64)
    pal = np.asarray(flags, bool)
    out[:, 0] = rec["length"]
    out[:, 1] = np.searchsorted(lay.markpos, rec["dbstart"].astype(np.int64))
    out[:, 2] = rec["dbstart"].astype(np.int64) - lay.start[out[:, 1]]
    q = rec["queryseq"].astype(np.int64)
    s2 = np.where(pal, np.minimum(q, lay.numofsequences - 1),
                  np.searchsorted(lay.markpos, q))
    out[:, 3] = s2
    out[:, 4] = np.where(pal, lay.seqlen[s2] - (
        rec["querystart"].astype(np.int64) + out[:, 0]), q - lay.start[s2])
    out[:, 5] = pal
    return out


def layout_kwargs(r, **more):
    """arguments of V.sink_params for the lists of a run"""
    tis, ssp = text()
    kw = dict(kind=2, totallength=len(tis), markpos=ssp, numofchars=4,
              leastlength=r["L"])
    kw.update(more)
    return kw


def synthetic_layout(V, nseq, seqlen, **kw):
    """nseq sequences of seqlen symbols -> (sink parameters, model layout)"""
    total = nseq * (seqlen + 1) - 1
    markpos = np.arange(1, nseq, dtype=np.uint64) * np.uint64(seqlen + 1) - \
        np.uint64(1)
    args = dict(kind=2, totallength=total, markpos=markpos)
    args.update(kw)
    return V.sink_params(**args), CM.Layout(total, markpos)


def self_records(seqlen, pairs, length=5, rel=0):
    rec = np.zeros(len(pairs), H.MATCH_DTYPE)
    p = np.asarray(pairs, np.uint64).reshape(-1, 2)
    rec["length"] = length
    rec["dbstart"] = p[:, 0] * np.uint64(seqlen + 1) + np.uint64(rel)
    rec["queryseq"] = p[:, 1] * np.uint64(seqlen + 1) + np.uint64(rel)
    return rec


def md5(b):
    return hashlib.md5(b).hexdigest()


_manifest = None
_arrays = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(H.GOLDEN, "cluster_manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def array(name):
    global _arrays
    if _arrays is None:
        _arrays = np.load(os.path.join(H.GOLDEN, "cluster_expected.npz"))
    return _arrays[name]


def input_of(key):
    """(records, flags) of the list the clusterer of a run sees"""
    return records_of(array(key + "__in"))


def expected_clusters(key):
    """the recorded member lists in output numbering"""
    start, mem = array(key + "__clusterstart"), array(key + "__members")
    return [list(mem[start[c]:start[c + 1]]) for c in range(len(start) - 1)]

"""The recorded match clustering runs (tests/golden/matchcluster_manifest.json,
matchcluster_expected.npz, written by scripts/make_golden_matchcluster.py):
the recipes from which both the vmatch command line and the calls of the
engine are derived.  Six runs are self lists (-l L) on the index of
tests/golden/at1MB.gz.  Three runs pin the query-side view, where position2
is a query coordinate on the same axis as position1, counted from the other
end for a P record: -q micro_q.fna on the index of micro_db.fna with -d and
with -d -p, and -d -p -l 30 on at1MB.  The last one is clustered under a
layout against queries whose query set is the index's own sequences (a plain
-p pass): what the reference prints has one of two mirror images dropped
already, and the layout that drops them (selfpalindromic) is refused.  Shared
by the generator and the two matchcluster test modules."""
import json
import os

import numpy as np

import helpers as H
import cluster_cases as CC
import matchcluster_model as MM

md5 = CC.md5


def R(key, L, mode, value, matches, edges, clusters, db="at1MB.gz",
      query=None, strands="d"):
    return dict(key=key, L=L, mode=mode, value=value, matches=matches,
                edges=edges, clusters=clusters, db=db, query=query,
                strands=strands)


RUNS = [
    R("l60_gap50", 60, MM.GAP, 50, 1330, 477, 59),
    R("l60_overlap50", 60, MM.OVERLAP, 50, 1330, 20858, 43),
    R("l30_gap0", 30, MM.GAP, 0, 3012, 32, 10),
    R("l30_overlap100", 30, MM.OVERLAP, 100, 3012, 23670, 260),
    R("l20_gap500", 20, MM.GAP, 500, 4507, 21777, 38),
    R("l20_overlap1", 20, MM.OVERLAP, 1, 4507, 118628, 100),
    R("micro_q_l8_gap20", 8, MM.GAP, 20, 12, 11, 1, db="micro_db.fna",
      query="micro_q.fna"),
    R("micro_q_dp_l8_gap20", 8, MM.GAP, 20, 24, 20, 1,
      db="micro_db.fna", query="micro_q.fna", strands="dp"),
    R("l30_dp_gap50", 30, MM.GAP, 50, 3033, 2544, 156, strands="dp"),
]


def run_of(key):
    return next(r for r in RUNS if r["key"] == key)


def keys():
    return [r["key"] for r in RUNS]


def queryform(r):
    """the list is clustered under a layout against queries"""
    return r["query"] is not None or r["strands"] != "d"


def list_args(r):
    return ["-l", str(r["L"])] + {"d": [], "dp": ["-d", "-p"]}[r["strands"]] \
        + (["-q", r["query"]] if r["query"] else [])


_texts = {}


def db_text(r):
    """(symbols with separators, separator positions) of the database"""
    if r["db"] == "at1MB.gz":
        return CC.text()
    if r["db"] not in _texts:
        tis, ssp, _ = H.fasta_text([os.path.join(H.GOLDEN, r["db"])])
        _texts[r["db"]] = (tis, np.asarray(ssp, np.uint64))
    return _texts[r["db"]]


def starts_lengths(ssp, total):
    start = np.concatenate(([0], np.asarray(ssp, np.int64) + 1))
    return start.astype(np.uint64), (np.concatenate(
        (np.asarray(ssp, np.int64), [total])) - start).astype(np.uint64)


def query_set(r):
    """(start, length, total length) of the query sequences: those of the
    query file, or the index's own ones"""
    if r["query"] is None:
        tis, ssp = db_text(r)
    else:
        tis, ssp, _ = H.fasta_text([os.path.join(H.GOLDEN, r["query"])])
    return starts_lengths(ssp, len(tis)) + (len(tis),)


def cluster_args(r, prefix):
    return ["-pp", "matchcluster",
            "gapsize" if r["mode"] == MM.GAP else "overlap", str(r["value"]),
            "outprefix", prefix]


def layout_kwargs(r, **more):
    """arguments of V.sink_params for the list of a run"""
    if not queryform(r):
        return CC.layout_kwargs(r, **more)
    tis, ssp = db_text(r)
    qstart, qlen, qtotal = query_set(r)
    kw = dict(kind=1, totallength=len(tis), markpos=ssp, numofchars=4,
              leastlength=r["L"], querystart=qstart, querylength=qlen,
              querytotallength=qtotal)
    kw.update(more)
    return kw


def records_of(r, rows):
    """rows (length, seq1, rel1, seq2, rel2, palindromic) -> (records, D/P
    flags): of a self list (length, start1, start2, 0); of a list against
    queries (length, dbstart, query number, offset in the query, or in its
    reverse complement for a P row)"""
    if not queryform(r):
        rec, flags = CC.records_of(rows)
        assert not flags.any()
        return rec, flags
    tis, ssp = db_text(r)
    dbstart, _ = starts_lengths(ssp, len(tis))
    _, qlen, _ = query_set(r)
    rows = np.asarray(rows, np.int64).reshape(-1, 6)
    pal = rows[:, 5] == 1
    rec = np.zeros(len(rows), H.MATCH_DTYPE)
    rec["length"] = rows[:, 0]
    rec["dbstart"] = dbstart[rows[:, 1]] + rows[:, 2].astype(np.uint64)
    rec["queryseq"] = rows[:, 3]
    rec["querystart"] = np.where(
        pal, qlen[rows[:, 3]].astype(np.int64) - (rows[:, 4] + rows[:, 0]),
        rows[:, 4])
    return rec, pal.astype(np.uint8)


def model_of(r, rec, flags, **kw):
    """the model on the list of a run"""
    if not queryform(r):
        return model(rec, r["mode"], r["value"], **kw)
    qstart, qlen, _ = query_set(r)
    l1, p1, p2 = MM.view(1, rec, flags, qstart, qlen)
    return MM.cluster(l1, p1, p2, r["mode"], r["value"], **kw)


def lines_of(V, r, rec, flags):
    """the match line of every record with the reference's default widths,
    each strand through a sink of its own; the D records of -d -p IDX go
    through the self sink as (length, start1, start2, 0), its P records
    through the selfpalindromic one"""
    out = [None] * len(rec)
    for f in (0, 1):
        who = np.flatnonzero(np.asarray(flags) == f)
        if len(who) == 0:
            continue
        part = rec[who]
        if not queryform(r):
            sink = V.Sink(**layout_kwargs(r))
        elif r["query"] is not None:
            sink = V.Sink(**layout_kwargs(r, palindromic=bool(f)))
        elif f == 0:
            qstart, _, _ = query_set(r)
            part = part.copy()
            part["queryseq"] = qstart[part["queryseq"].astype(np.int64)] + \
                part["querystart"]
            part["querystart"] = 0
            sink = V.Sink(**CC.layout_kwargs(r))
        else:
            sink = V.Sink(**layout_kwargs(r, palindromic=True,
                                          selfpalindromic=True))
        sink.setdigits()
        lines = sink.format(part).decode().splitlines()
        assert len(lines) == len(who)
        for k, line in zip(who, lines):
            out[k] = line
    return out


def synthetic_layout(V, total=1 << 20):
    """one sequence of `total` symbols, matches of the index against itself"""
    return V.sink_params(kind=2, totallength=total,
                         markpos=np.zeros(0, np.uint64))


def records(length, position1, position2):
    """a self list: (length, start1, start2, 0)"""
    rec = np.zeros(len(position1), H.MATCH_DTYPE)
    rec["length"] = length
    rec["dbstart"] = position1
    rec["queryseq"] = position2
    return rec


def model(rec, mode, value, **kw):
    l1, p1, p2 = MM.view(2, rec)
    return MM.cluster(l1, p1, p2, mode, value, **kw)


_manifest = None
_arrays = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(H.GOLDEN, "matchcluster_manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def array(name):
    global _arrays
    if _arrays is None:
        _arrays = np.load(os.path.join(H.GOLDEN, "matchcluster_expected.npz"))
    return _arrays[name]


def input_name(r):
    """the self lists of one -l L are stored once"""
    return r["key"] + "__in" if queryform(r) else "l%d__in" % r["L"]


def input_of(key):
    """(records, D/P flags) of the list the clusterer of a run sees"""
    r = run_of(key)
    return records_of(r, array(input_name(r)))


def sink_of(V, r, **more):
    """the sink that prints the match lines of the cluster files"""
    s = V.Sink(**layout_kwargs(r, **more))
    s.setdigits()
    return s


def text_of(r, got, lines, flags):
    """cluster c of `got` (members, edges and values as arrays) -> the bytes
    of its file behind its first line, from the line of every record"""
    ids = MM.printed_ids([int(f) for f in flags])

    def text(c):
        a, b = (int(x) for x in got["clusterstart"][c:c + 2])
        e0, e1 = (int(x) for x in got["edgestart"][c:c + 2])
        mem = [int(m) for m in got["members"][a:b]]
        val = np.asarray(got["values"][e0:e1], np.uint64)
        val = val.tolist() if r["mode"] == MM.GAP else \
            val.view(np.float64).tolist()
        return MM.format_cluster(
            r["mode"], mem, [lines[m] for m in mem],
            list(zip(got["m0"][e0:e1].tolist(), got["m1"][e0:e1].tolist(),
                     val)), ids)
    return text


def check_against_manifest(key, got, cluster_text):
    """got: a dict like MM.cluster returns (stats as a dict); cluster_text(c)
    -> the bytes of the file of cluster c behind its first line"""
    e = manifest()[key]
    for k in ("matches", "candidates", "edges", "forestedges", "clusters",
              "inclusters"):
        assert got["stats"][k] == e["stats"][k], k
    assert md5(got["text"]) == e["md5_text"]
    assert np.array_equal(got["clusterstart"], array(key + "__clusterstart"))
    assert np.array_equal(got["members"], array(key + "__members"))
    assert np.array_equal(got["edgestart"], array(key + "__edgestart"))
    if key + "__m0" in e["stored"]:
        assert np.array_equal(got["m0"], array(key + "__m0"))
        assert np.array_equal(got["m1"], array(key + "__m1"))
        if run_of(key)["mode"] == MM.GAP:
            assert np.array_equal(got["values"], array(key + "__values"))
        else:
            assert ["%.2f" % v for v in
                    np.asarray(got["values"], np.uint64).view(np.float64)] \
                == list(array(key + "__values"))
    for c, want in enumerate(e["md5_files"]):
        assert md5(cluster_text(c)) == want, (key, c)

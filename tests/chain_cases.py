"""The recorded chaining runs (tests/golden/chain_manifest.json,
chain_expected.npz, written by scripts/make_golden_chain.py): the recipes
from which both the vmatch command line and the calls of the library are
derived.  The lists are those of the match clustering fixtures
(matchcluster_cases.py): `src` names the run there whose list a chaining run
reads.  One more list comes from tests/golden/chain_ties.fna, a text made so
that the unstable quicksort of the grouping leaves a run of equal keys in
another order than a stable sort.  Shared by the generator and the two chain
test modules."""
import json
import os

import numpy as np

import helpers as H
import cluster_cases as CC
import matchcluster_cases as MC
import matchcluster_model as MM
import chain_model as CH

md5 = CC.md5

KINDS = {"global": CH.GLOBAL, "gc": CH.GLOBAL_GC, "ov": CH.GLOBAL_OV}


def parse_words(words):
    """the words behind -pp chain -> dict(kind, value, maxgap, wf,
    withinborders, silent)"""
    o = dict(kind=CH.GLOBAL, value=0, maxgap=0, wf=1.0, withinborders=False,
             silent=False)
    w = list(words)
    while w:
        t = w.pop(0)
        if t == "global":
            o["kind"] = CH.GLOBAL
            if w and w[0] in ("gc", "ov"):
                o["kind"] = KINDS[w.pop(0)]
        elif t == "local":
            o["kind"] = CH.LOCAL_MAX
            if w and w[0][0].isdigit():
                v = w.pop(0)
                if v.endswith("b"):
                    o["kind"], o["value"] = CH.LOCAL_BEST, int(v[:-1])
                elif v.endswith("p"):
                    o["kind"], o["value"] = CH.LOCAL_PERCENT, int(v[:-1])
                else:
                    o["kind"], o["value"] = CH.LOCAL_THRESHOLD, int(v)
        elif t == "wf":
            o["wf"] = float(w.pop(0))
        elif t == "maxgap":
            o["maxgap"] = int(w.pop(0))
        elif t == "withinborders":
            o["withinborders"] = True
        elif t == "silent":
            o["silent"] = True
        else:
            raise ValueError(t)
    return o


def R(src, words):
    words = words.split()
    key = src.split("_gap")[0] + "__" + "_".join(words).replace(".", "")
    r = dict(key=key, src=src, words=words)
    r.update(parse_words(words))
    return r


TIES_DB = "chain_ties.fna"

RUNS = [R("l30_gap0", w) for w in (
    "global", "global gc", "global ov", "local", "local 100", "local 3b",
    "local 20p", "local withinborders", "global gc withinborders maxgap 500",
    "local maxgap 50 withinborders", "local 100 silent")] + [
    R("l20_gap500", "local 150 withinborders"),
    R("l20_gap500", "global ov withinborders"),
    R("l20_gap500", "global"),
    R("l60_gap50", "local 100 withinborders wf 0.5"),
    R("l30_dp_gap50", "global gc withinborders"),
    R("micro_q_l8_gap20", "local withinborders"),
    R("micro_q_dp_l8_gap20", "global gc"),
    R("ties", "local withinborders"),
    R("ties", "global gc withinborders"),
]

# the list of chain_ties.fna is no match clustering run: its recipe in the
# form of one
TIES_RUN = dict(key="ties", L=12, db=TIES_DB, query=None, strands="d",
                mode=MM.GAP, value=0)


def run_of(key):
    return next(r for r in RUNS if r["key"] == key)


def keys():
    return [r["key"] for r in RUNS]


def source(r):
    """the recipe of the list of a run, in the form of matchcluster_cases"""
    return TIES_RUN if r["src"] == "ties" else MC.run_of(r["src"])


def list_args(r):
    return MC.list_args(source(r))


def chain_args(r):
    return ["-pp", "chain"] + r["words"]


_ties = None


def ties_text():
    global _ties
    if _ties is None:
        tis, ssp, _ = H.fasta_text([os.path.join(H.GOLDEN, TIES_DB)])
        _ties = (tis, np.asarray(ssp, np.uint64))
    return _ties


def self_records(rows, ssp, total):
    """rows (length, seq1, rel1, seq2, rel2, 0) of a self list -> records
    (length, start1, start2, 0)"""
    start, _ = MC.starts_lengths(ssp, total)
    rows = np.asarray(rows, np.int64).reshape(-1, 6)
    rec = np.zeros(len(rows), H.MATCH_DTYPE)
    rec["length"] = rows[:, 0]
    rec["dbstart"] = start[rows[:, 1]] + rows[:, 2].astype(np.uint64)
    rec["queryseq"] = start[rows[:, 3]] + rows[:, 4].astype(np.uint64)
    return rec, np.zeros(len(rows), np.uint8)


def rows_of(r):
    if r["src"] == "ties":
        return array("ties__in")
    return MC.array(MC.input_name(source(r)))


def input_of(key):
    """(records, D/P flags) of the list a run chains"""
    r = run_of(key)
    if r["src"] == "ties":
        tis, ssp = ties_text()
        return self_records(rows_of(r), ssp, len(tis))
    return MC.input_of(r["src"])


def layout_kwargs(r, **more):
    if r["src"] == "ties":
        tis, ssp = ties_text()
        kw = dict(kind=2, totallength=len(tis), markpos=ssp, numofchars=4,
                  leastlength=TIES_RUN["L"])
        kw.update(more)
        return kw
    return MC.layout_kwargs(source(r), **more)


def lines_of(V, r, rec, flags):
    """the match line of every record with the field widths of the layout
    (outvmatchchain prints with the run's own widths, not with the default
    ones of the cluster files), each strand through a sink of its own like
    matchcluster_cases.lines_of"""
    s = source(r)
    out = [None] * len(rec)
    for f in (0, 1):
        who = np.flatnonzero(np.asarray(flags) == f)
        if len(who) == 0:
            continue
        part = rec[who]
        if r["src"] == "ties" or not MC.queryform(s):
            sink = V.Sink(**layout_kwargs(r))
        elif s["query"] is not None:
            sink = V.Sink(**layout_kwargs(r, palindromic=bool(f)))
        elif f == 0:
            qstart, _, _ = MC.query_set(s)
            part = part.copy()
            part["queryseq"] = qstart[part["queryseq"].astype(np.int64)] + \
                part["querystart"]
            part["querystart"] = 0
            sink = V.Sink(**CC.layout_kwargs(s))
        else:
            sink = V.Sink(**layout_kwargs(r, palindromic=True,
                                          selfpalindromic=True))
        lines = sink.format(part).decode().splitlines()
        assert len(lines) == len(who)
        for k, line in zip(who, lines):
            out[k] = line
    return out


def view_of(r, rec, flags):
    """(length1, position1, length2, position2, seqnum1, seqnum2) as lists:
    what processfinal stores of the list of a run"""
    s = source(r)
    rows = np.asarray(rows_of(r), np.int64).reshape(-1, 6)
    if r["src"] != "ties" and MC.queryform(s):
        qstart, qlen, _ = MC.query_set(s)
        l1, p1, p2 = MM.view(1, rec, flags, qstart, qlen)
    else:
        l1, p1, p2 = MM.view(2, rec)
    return l1, p1, list(l1), p2, rows[:, 1].tolist(), rows[:, 3].tolist()


def options(r):
    return {k: r[k] for k in ("kind", "value", "maxgap", "wf",
                              "withinborders")}


def model_of(r, rec, flags, **kw):
    return CH.chain(*view_of(r, rec, flags), **options(r), **kw)


def as_arrays(got):
    """the chains of the model as the arrays the library delivers"""
    rows = got["chains"]
    return dict(
        problem=np.array([c[0] for c in rows], np.uint64),
        number=np.array([c[1] for c in rows], np.uint64),
        score=np.array([c[2] for c in rows], np.int64),
        start=np.array([c[3] for c in rows] + [len(got["members"])],
                       np.uint64),
        members=np.array(got["members"], np.uint64))


def text_of(arr, lines, silent=False):
    """the reference's text from chain arrays and the line of every record"""
    rows = list(zip(arr["problem"].tolist(), arr["number"].tolist(),
                    arr["score"].tolist(), arr["start"].tolist()))
    return CH.format_chains(rows, arr["members"].tolist(), lines, silent)


_manifest = None
_arrays = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(H.GOLDEN, "chain_manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def array(name):
    global _arrays
    if _arrays is None:
        _arrays = np.load(os.path.join(H.GOLDEN, "chain_expected.npz"))
    return _arrays[name]


STAT_KEYS = ("matches", "problems", "single", "small", "wave", "group",
             "largest", "tieruns", "replayed", "chains", "chained")


def check_against_manifest(key, stats, arr, text):
    """stats: a dict; arr: problem, number, score, start, members; text: the
    bytes behind the "# args=" line"""
    e = manifest()["runs"][key]
    for k in STAT_KEYS:
        assert stats[k] == e["stats"][k], (key, k, stats[k], e["stats"][k])
    for k in ("problem", "number", "score", "start", "members"):
        assert np.array_equal(arr[k], array(key + "__" + k)), (key, k)
    assert md5(text) == e["md5_text"], key

"""The recorded selection runs (tests/golden/select_manifest.json,
select_expected.npz, written by scripts/make_golden_select.py): the recipes
from which both the vmatch command line and the calls of the engine are
derived, and the conversions between the rows vmatch prints and the records
of the engine.  Shared by the generator and the two select test modules."""
import hashlib
import json
import os

import numpy as np

import helpers as H
import select_model as SM


def R(key, engine, L=0, strands="d", approx=None):
    return dict(key=key, engine=engine, L=L, strands=strands, approx=approx)


# engine: query (-l L -q), complete (-complete -e|-h K -q), repeats (-l L
# IDX), supermax, tandem.  The self-palindromic runs (-p IDX) are left out:
# the engine answers VSA_NOT_COVERED for them.
RUNS = {
    "micro": [R("q_l3", "query", 3), R("q_l3_dp", "query", 3, "dp"),
              R("s_l2", "repeats", 2)],
    "grumbach": [R("q_l14", "query", 14), R("s_l12", "repeats", 12),
                 R("s_supermax12", "supermax", 12),
                 R("s_tandem3", "tandem", 3)],
    "c5": [R("c_e2", "complete", approx=[1, 2]),
           R("c_h2", "complete", approx=[0, 2]),
           R("q_l20_dp", "query", 20, "dp"), R("q_l16", "query", 16)],
}
# (run, filter) recorded besides the -best / -sort variants of every run
FILTERS = {
    ("micro", "q_l3"): [dict(evalue=1e-3)],
    ("grumbach", "q_l14"): [dict(evalue=1e-3)],
    ("c5", "c_e2"): [dict(evalue=1e-3), dict(identity=99),
                     dict(leastscore=196)],
    ("c5", "c_h2"): [dict(identity=99), dict(leastscore=196)],
    ("grumbach", "s_l12"): [dict(gap=[10, 200]), dict(gap=[-5, 3]),
                            dict(evalue=1e-3)],
    ("grumbach", "s_supermax12"): [dict(gap=[10, 200])],
}
SORTSETS = (("la", "id", "ja", "ed", "sd", "ida"),
            ("ld", "ia", "jd", "ea", "sa", "idd"))


def engine_args(r, gap=None):
    e = r["engine"]
    least = ["-l", str(r["L"])] + [str(g) for g in (gap or [])]
    if e == "query":
        return least + {"d": [], "p": ["-p"], "dp": ["-d", "-p"]}[r["strands"]]
    if e == "complete":
        return ["-complete", "-e" if r["approx"][0] else "-h",
                str(r["approx"][1])]
    return {"repeats": [], "supermax": ["-supermax"],
            "tandem": ["-tandem"]}[e] + least


def variant_args(v):
    a = []
    if v.get("best"):
        a += ["-best", str(v["best"])]
    if v.get("sort"):
        a += ["-sort", v["sort"]]
    if v.get("evalue") is not None:
        a += ["-evalue", repr(v["evalue"])]
    if v.get("identity"):
        a += ["-identity", str(v["identity"])]
    if v.get("leastscore") is not None:
        a += ["-leastscore", str(v["leastscore"])]
    return a


def withquery(r):
    return r["engine"] in ("query", "complete")


def kind_of(r):
    if r["engine"] == "query":
        return SM.QUERY
    if r["engine"] == "complete":
        return SM.EDIST if r["approx"][0] else SM.HAMMING
    return SM.SELF


def parse_rows(lines):
    """the default columns -> rows (length1, seq1, rel1, seq2, rel2 -- the
    |distance| for -complete -e/-h --, palindromic)"""
    out = np.zeros((len(lines), 6), np.int64)
    for i, l in enumerate(lines):
        f = l.split()
        out[i] = (int(f[0]), int(f[1]), int(f[2]), int(f[5]),
                  int(f[6]) if int(f[7]) == 0 else abs(int(f[7])),
                  1 if f[3] == "P" else 0)
    return out


def records_of(case, r, rows):
    """rows -> (engine records, D/P flags)"""
    idx, q = H.load_case(case)
    rows = np.asarray(rows, np.int64).reshape(-1, 6)
    starts = np.concatenate(([0], idx.ssp.astype(np.int64) + 1))
    rec = np.zeros(len(rows), H.MATCH_DTYPE)
    rec["length"] = rows[:, 0]
    rec["dbstart"] = starts[rows[:, 1]] + rows[:, 2]
    if not withquery(r):
        rec["queryseq"] = starts[rows[:, 3]] + rows[:, 4]
    else:
        rec["queryseq"] = rows[:, 3]
        rel = rows[:, 4].copy()
        if r["engine"] == "query":
            # a palindromic match is reported on the reverse strand
            pal = rows[:, 5] == 1
            qlen = q.length.astype(np.int64)[rows[:, 3]]
            rel[pal] = qlen[pal] - (rel[pal] + rows[pal, 0])
        rec["querystart"] = rel
    return rec, rows[:, 5].astype(np.uint8)


def query_multiseq(q):
    """(start, length, total length) of the query Multiseq"""
    length = q.length.astype(np.uint64)
    start = np.concatenate(([0], np.cumsum(length + np.uint64(1))[:-1]))
    return start.astype(np.uint64), length, int(length.sum()) + len(length) - 1


def layout_kwargs(case, r, **more):
    """arguments of V.sink_params / V.Sink for a run"""
    idx, q = H.load_case(case)
    kw = dict(kind=kind_of(r), totallength=idx.n, markpos=idx.ssp,
              numofchars=4, leastlength=r["L"])
    if withquery(r):
        kw["querystart"], kw["querylength"], kw["querytotallength"] = \
            query_multiseq(q)
    kw.update(more)
    return kw


def model_layout(case, r, **more):
    idx, q = H.load_case(case)
    return SM.Layout(kind_of(r), idx.n, 4,
                     q.length if withquery(r) else (), leastlength=r["L"],
                     **more)


def format_lines(V, case, r, rec, flags):
    """the lines of records with mixed D/P flags through the sink"""
    sinks = {p: V.Sink(**layout_kwargs(case, r, palindromic=bool(p)))
             for p in set(int(f) for f in flags)}
    out, i = [], 0
    while i < len(rec):
        j = i
        while j < len(rec) and flags[j] == flags[i]:
            j += 1
        out.append(sinks[int(flags[i])].format(rec[i:j]))
        i = j
    return b"".join(out)


def md5(text):
    return hashlib.md5(text).hexdigest()


_manifest = None
_arrays = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(H.GOLDEN, "select_manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def array(name):
    global _arrays
    if _arrays is None:
        _arrays = np.load(os.path.join(H.GOLDEN, "select_expected.npz"))
    return _arrays[name]


def all_variants():
    """[(case, run key, variant key)]"""
    m = manifest()
    return [(c, k, v) for c in sorted(m) for k in sorted(m[c])
            for v in sorted(m[c][k]["variants"])]


def run_of(case, key):
    return next(r for r in RUNS[case] if r["key"] == key)


def options_of(v):
    """a recorded variant -> keyword arguments of V.select_params and of
    select_model.select"""
    o = dict(best=v.get("best", 0), sort=v.get("sort"))
    for k in ("evalue", "identity", "leastscore", "gap"):
        if v.get(k) is not None:
            o[k] = v[k]
    return o

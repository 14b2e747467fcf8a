"""What the eight entries of the two seed extensions (-l L -h K, -l L -e K)
refuse, pinned from outside: (entry, defect) -> (code, exact message).  The
tables below were written from the sources while every entry still made its
own checks, and passed on them as they were; the shared drivers
(extend_shared.hpp, extend_host_common.h) have to give the same answers.  The
two host entries run without a GPU; the six device entries run on the
`borders` lists of extend_cases.py / extend_edist_cases.py and leave the
device's memory as they found it."""
import ctypes as C

import numpy as np
import pytest

import extend_cases as EC
import extend_edist_cases as DC
import helpers as H

NC = -4                                                 # VSA_NOT_COVERED
OK = (0, None)
# kind -> (cap of the device, bound of the record)
KINDS = {"hamming": (64, 0xFFFF), "edist": (31, 125)}
# a seed that does not fit its texts: the field edits of the GPU tests
DEVICE_MISFITS = (("dbstart", "n - 1"), ("queryseq", 1 << 40),
                  ("querystart", 1 << 33), ("length", 0),
                  ("length", 1 << 50))
# ... and those of the host tests
HOST_MISFITS = (("dbstart", "n"), ("queryseq", "nq"),
                ("querystart", 1 << 20), ("length", 0), ("length", 1 << 50))

_sc = {}


def borders(kind):
    if kind not in _sc:
        _sc[kind] = (EC.scenarios(256, 1024) if kind == "hamming" else
                     DC.scenarios(256))["borders"]
    return _sc[kind]


def edited(sc, at, field, value):
    value = {"n": len(sc.text), "n - 1": len(sc.text) - 1,
             "nq": sc.queries().nq}.get(value, value)
    bad = sc.records()
    bad[field][at] = value
    return bad


def test_the_limits_the_tables_are_written_for(V):
    assert NC == V.NOT_COVERED
    assert (V.SINK_QUERY, V.SINK_SELF) == (1, 2)
    assert KINDS["hamming"] == (V.EXTEND_MAXDIST, V.HAMMING_MAXDISTANCE)
    assert KINDS["edist"] == (V.EXTEND_EDIST_MAXDIST, V.EDIST_MAXDISTANCE)
    assert V.EXTEND_LANE_BUDGET == 256 and V.EXTEND_LONG_STEP == 1024


# --------------------------------------------------------------------------
# vsa_extend_hamming_host, vsa_extend_edist_host
# --------------------------------------------------------------------------

def host_who(kind):
    return "vsa_extend_%s_host" % kind


def H_NULL(kind):
    return (-1, host_who(kind) + ": NULL argument")


def H_LAYOUT(kind):
    return (-2, host_who(kind) + ": the seeds of a query layout "
            "(VSA_SINK_QUERY, with the query symbols) or of a self layout "
            "(VSA_SINK_SELF) are extended")


def H_BOUND(kind):
    return (-2, host_who(kind) + ": a least length and a distance bound from "
            "1 to %d" % KINDS[kind][1])


def H_MISFIT(kind):
    return (-2, host_who(kind) + ": record 5 does not fit the layout")


# defect -> (what is changed in the call, the answer)
HOST_DEFECTS = {
    "none": ({}, lambda k: OK),
    "null_layout": (dict(layout=None), H_NULL),
    "null_text": (dict(text=None), H_NULL),
    "null_seeds": (dict(seeds=None), H_NULL),
    "null_matches": (dict(matches=None), H_NULL),
    "null_numofmatches": (dict(numofmatches=None), H_NULL),
    "L0": (dict(L=0), H_BOUND),
    "K0": (dict(K=0), H_BOUND),
    "K_above_the_record": (dict(K="bound + 1"), H_BOUND),
    "kind_complete": (dict(laykind=0), H_LAYOUT),
    "kind_extended": (dict(laykind="extended"), H_LAYOUT),
    "query_layout_without_symbols": (dict(querysymbols=None), H_LAYOUT),
    "query_layout_without_arrays": (dict(noarrays=True), H_LAYOUT),
    "totallength0": (dict(totallength=0), H_LAYOUT),
    "numofchars1": (dict(numofchars=1), H_LAYOUT),
    # (the host entries have no palindromic flag, and a self layout does not
    # look at the query symbols it is given)
    "self_layout_with_symbols": (dict(laykind=2), lambda k: OK),
    "capacity": (dict(capacity="one too few"),
                 lambda k: (-3, host_who(k) + ": more than %d matches")),
}
HOST_DEFECTS.update({
    "misfit_%s_%s" % (f, i): (dict(edit=(f, v)), H_MISFIT)
    for i, (f, v) in enumerate(HOST_MISFITS)})


def host_call(V, kind, L=10, K=2, **d):
    """one raw call of the host entry -> (code, message, number of matches)"""
    sc = borders(kind)
    q = sc.queries()
    text = np.ascontiguousarray(sc.text, np.uint8)
    sym = np.ascontiguousarray(q.symbols, np.uint8)
    seeds = sc.records()
    if "edit" in d:
        seeds = edited(sc, 5, *d["edit"])
    laykind = d.get("laykind", 1)
    if laykind == "extended":
        laykind = 8 if kind == "hamming" else 10
    if K == "bound + 1":
        K = KINDS[kind][1] + 1
    if d.get("noarrays"):
        p, keep = V.sink_params(laykind, len(text), ())
        p.numofqueries = q.nq
    else:
        p, keep = V.sink_params(laykind, len(text), (), querystart=q.start,
                                querylength=q.length)
    p.totallength = d.get("totallength", len(text))
    p.numofchars = d.get("numofchars", 4)
    out = np.zeros(len(seeds), V.MATCH_DTYPE)
    n = C.c_uint64(12345)
    args = dict(layout=C.byref(p), text=text.ctypes.data,
                querysymbols=sym.ctypes.data, seeds=seeds.ctypes.data,
                matches=out.ctypes.data, numofmatches=C.byref(n))
    args.update({k: d[k] for k in args if k in d})
    capacity = d.get("capacity", len(out))
    fn = getattr(V.lib, host_who(kind))

    def run(cap):
        rc = fn(args["layout"], args["text"], args["querysymbols"],
                args["seeds"], len(seeds), L, K, 0, 2, args["matches"], cap,
                args["numofmatches"])
        return rc, V.messagespace() if rc != 0 else None, int(n.value)

    if capacity == "one too few":
        rc, _, full = run(len(out))
        assert rc == 0 and full > 1
        return run(full - 1) + (full - 1,)
    return run(capacity) + (None,)


@pytest.mark.parametrize("defect", sorted(HOST_DEFECTS))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_what_the_host_entries_refuse(V, kind, defect):
    change, want = HOST_DEFECTS[defect]
    rc, message, n, cap = host_call(V, kind, **change)
    code, text = want(kind)
    if cap is not None:
        text = text % cap
    assert (rc, message) == (code, text)
    if defect == "none":
        assert n > 0
    elif code != 0 and "numofmatches" not in change and "layout" not in change and \
            "text" not in change and "matches" not in change:
        assert n == 0               # (set behind the first NULL checks)


# --------------------------------------------------------------------------
# the six device entries
# --------------------------------------------------------------------------

ENTRIES = ("extend", "findquerymatches", "findselfmatches")


def who(kind, entry):
    return "vsa_%s_%s" % (entry, kind) if entry != "extend" else \
        "vsa_extend_" + kind


def D_NULL(kind, entry):
    return (-1, who(kind, entry) + ": NULL argument")


def D_LAYOUT(kind, entry):
    return (-2, who(kind, entry) + ": the seeds of a query layout "
            "(VSA_SINK_QUERY, with their batch) or of a self layout "
            "(VSA_SINK_SELF, no batch, not palindromic) are extended")


def D_BOUND(kind, entry):
    return (-2, who(kind, entry) + ": a least length and a distance bound of "
            "at least 1")


def D_CAP(kind, entry):
    cap, bound = KINDS[kind]
    tail = "(vsa_extend_hamming_host takes any)" if kind == "hamming" else \
        "(vsa_extend_edist_host takes up to %d)" % bound
    return (NC, who(kind, entry) + ": distance bound %d: up to %d are covered "
            "on the device %s" % (cap + 1, cap, tail))


def D_PACKED(kind, entry):
    return (NC, who(kind, entry) + ": a packed candidate result has no "
            "records to extend")


def D_EXTENDED(kind, entry):
    return (NC, who(kind, entry) + ": the list holds extended seeds already")


def D_MISFIT(kind, entry):
    return (-2, who(kind, entry) + ": 1 seeds do not fit the index or their "
            "query sequence")


# defect -> (the entries it can be put to, the change, the answer)
DEVICE_DEFECTS = {
    "null_index": (ENTRIES, dict(index=None), D_NULL),
    "null_result": (ENTRIES, dict(result=None), D_NULL),
    "null_seeds": (("extend",), dict(seeds=None), D_NULL),
    "null_layout": (("extend",), dict(layout=None), D_NULL),
    "null_queries": (("findquerymatches",), dict(queries=None), D_NULL),
    "L0": (ENTRIES, dict(L=0), D_BOUND),
    "K0": (ENTRIES, dict(K=0), D_BOUND),
    "K_above_the_cap": (ENTRIES, dict(K="cap + 1"), D_CAP),
    "kind_complete": (("extend",), dict(laykind=0), D_LAYOUT),
    "kind_extended": (("extend",), dict(laykind="extended"), D_LAYOUT),
    "self_layout_with_batch": (("extend",), dict(laykind=2), D_LAYOUT),
    "self_layout_palindromic": (("extend",),
                                dict(laykind=2, queries=None, palindromic=1),
                                D_LAYOUT),
    "query_layout_without_batch": (("extend",), dict(queries=None), D_LAYOUT),
    "packed_list": (("extend",), dict(seeds="packed"), D_PACKED),
    "extended_list": (("extend",), dict(seeds="extended"), D_EXTENDED),
}
DEVICE_DEFECTS.update({
    "misfit_%s_%s" % (f, i): (("extend",), dict(seeds=(f, v)), D_MISFIT)
    for i, (f, v) in enumerate(DEVICE_MISFITS)})
DEVICE_CASES = [(k, e, d) for k in sorted(KINDS) for d in sorted(DEVICE_DEFECTS)
                for e in DEVICE_DEFECTS[d][0]]

_device = {}


def device_things(V, kind):
    """the index, the batch and the seed lists of `borders`, uploaded once"""
    if kind not in _device:
        sc = borders(kind)
        i = H.oracle_build_index(sc.text, 4)
        gi = V.Index.from_tables(i.n, i.prefixlength, i.numofchars, i.tis,
                                 i.suf, i.lcp, i.llv, i.bck, i.bwt,
                                 i.querysepposition, i.hasqueries)
        q = sc.queries()
        gq = V.Queries.from_host(q.symbols, q.start, q.length)
        seeds = V.Result.from_host(sc.records())
        ext = getattr(V, "extend_" + kind)(gi, gq, seeds, 10, 2)
        assert ext.count > 0
        # a packed candidate list, with the index and the batch it is of
        c1, cq = H.load_case("c1")
        ci = V.Index.from_tables(c1.n, c1.prefixlength, c1.numofchars, c1.tis,
                                 c1.suf, c1.lcp, c1.llv, c1.bck, c1.bwt,
                                 c1.querysepposition, c1.hasqueries)
        cgq = V.Queries.from_host(cq.symbols, cq.start, cq.length)
        packed = V.findmumcandidates_packed(ci, cgq, 20)
        assert packed.count > 0 and packed.packbits
        lists = {"packed": packed, "extended": ext, None: None,
                 "of packed": (ci, cgq)}
        for f, v in DEVICE_MISFITS:
            lists[f, v] = V.Result.from_host(edited(sc, 7, f, v))
        _device[kind] = gi, gq, seeds, lists
    return _device[kind]


def device_call(V, kind, entry, L=10, K=2, **d):
    gi, gq, seeds, lists = device_things(V, kind)
    if K == "cap + 1":
        K = KINDS[kind][0] + 1
    index = d.get("index", gi)
    queries = d.get("queries", gq)
    if "seeds" in d:
        seeds = lists[d["seeds"]]
        if d["seeds"] == "packed":
            index, queries = lists["of packed"]
    laykind = d.get("laykind", 1)
    if laykind == "extended":
        laykind = 8 if kind == "hamming" else 10
    p = V.SinkParams()
    p.kind = laykind
    h = C.c_void_p()
    handle = lambda x: None if x is None else x._h
    result = d.get("result", C.byref(h))
    fn = getattr(V.lib, who(kind, entry))
    before = V.device_meminfo()
    if entry == "extend":
        rc = fn(handle(index), handle(queries), handle(seeds),
                d.get("layout", C.byref(p)), d.get("palindromic", 0), L, K, 0,
                result)
    elif entry == "findquerymatches":
        rc = fn(handle(index), handle(queries), L, K, 0, 0, result)
    else:
        rc = fn(handle(index), L, K, 0, result)
    message = V.messagespace() if rc != 0 else None
    if h.value:
        V.Result(h).close()
    assert rc != 0 and not h.value
    assert V.device_meminfo() == before
    return rc, message


@pytest.mark.gpu
@pytest.mark.parametrize("kind,entry,defect", DEVICE_CASES)
def test_what_the_device_entries_refuse(V, monkeypatch, kind, entry, defect):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    monkeypatch.delenv("VSA_EXTEND_EDIST_SCRATCH", raising=False)
    _, change, want = DEVICE_DEFECTS[defect]
    assert device_call(V, kind, entry, **change) == want(kind, entry)

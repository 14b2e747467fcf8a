"""What the four entries of the X-drop extension (-hxdrop X, -exdrop X)
refuse, pinned from outside: (entry, defect) -> (code, exact message), in the
words of the shared drivers (extend_shared.hpp, extend_host_common.h) as
test_extend_refusals.py pins them for the two sibling kinds, plus the bound
of X, which names the reference's.  The host entry runs without a GPU; the
three device entries run on the `borders` lists of extend_xdrop_cases.py and
leave the device's memory as they found it.  (A list of 2^31 seeds cannot be
made in a test; that refusal is the driver's own line, shared with the
siblings.)"""
import ctypes as C

import numpy as np
import pytest

import extend_xdrop_cases as XC
import helpers as H

NC = -4                                                 # VSA_NOT_COVERED
OK = (0, None)
MODES = (1, 0)                                          # hamming
DEVICE_MISFITS = (("dbstart", "n - 1"), ("queryseq", 1 << 40),
                  ("querystart", 1 << 33), ("length", 0),
                  ("length", 1 << 50))
HOST_MISFITS = (("dbstart", "n"), ("queryseq", "nq"),
                ("querystart", 1 << 20), ("length", 0), ("length", 1 << 50))

_sc = []


def borders():
    if not _sc:
        _sc.append(XC.scenarios(256, 1024)["borders"])
    return _sc[0]


def edited(sc, at, field, value):
    value = {"n": len(sc.text), "n - 1": len(sc.text) - 1,
             "nq": sc.queries().nq}.get(value, value)
    bad = sc.records()
    bad[field][at] = value
    return bad


def test_the_limits_the_tables_are_written_for(V):
    assert NC == V.NOT_COVERED
    assert (V.SINK_QUERY, V.SINK_SELF) == (1, 2)
    assert V.XDROP_MAXDROP == 255
    assert V.SINK_QUERY_HXDROP == 12 and V.SINK_SELF_EXDROP == 15


def xbound(who, X):
    return (-2, "%s: X = %d: the reference takes 1 to 255 (FLAGXDROP, "
            "Vmatch/parsevm.c)" % (who, X))


# --------------------------------------------------------------------------
# vsa_extend_xdrop_host
# --------------------------------------------------------------------------

HWHO = "vsa_extend_xdrop_host"
H_NULL = (-1, HWHO + ": NULL argument")
H_LAYOUT = (-2, HWHO + ": the seeds of a query layout (VSA_SINK_QUERY, with "
            "the query symbols) or of a self layout (VSA_SINK_SELF) are "
            "extended")
H_BOUND = (-2, HWHO + ": a least length and a distance bound from 1 to 255")
H_MISFIT = (-2, HWHO + ": record 5 does not fit the layout")

# defect -> (what is changed in the call, the answer)
HOST_DEFECTS = {
    "none": ({}, OK),
    "null_layout": (dict(layout=None), H_NULL),
    "null_text": (dict(text=None), H_NULL),
    "null_seeds": (dict(seeds=None), H_NULL),
    "null_matches": (dict(matches=None), H_NULL),
    "null_numofmatches": (dict(numofmatches=None), H_NULL),
    "L0": (dict(L=0), H_BOUND),
    "X0": (dict(X=0), H_BOUND),
    "X255": (dict(X=255), OK),
    "X256": (dict(X=256), xbound(HWHO, 256)),
    "X_huge": (dict(X=1 << 40), xbound(HWHO, 1 << 40)),
    "kind_complete": (dict(laykind=0), H_LAYOUT),
    "kind_extended": (dict(laykind=12), H_LAYOUT),
    "kind_extended_edit": (dict(laykind=15), H_LAYOUT),
    "query_layout_without_symbols": (dict(querysymbols=None), H_LAYOUT),
    "query_layout_without_arrays": (dict(noarrays=True), H_LAYOUT),
    "totallength0": (dict(totallength=0), H_LAYOUT),
    "numofchars1": (dict(numofchars=1), H_LAYOUT),
    "text_too_long_for_the_record": (
        dict(totallength=0xFFFFFFF0, seeds="none"),
        (NC, HWHO + ": texts and query sequences below 2^32 - 16 symbols "
         "are covered")),
    "self_layout_with_symbols": (dict(laykind=2), OK),
    "capacity": (dict(capacity="one too few"),
                 (-3, HWHO + ": more than %d matches")),
}
HOST_DEFECTS.update({
    "misfit_%s_%s" % (f, i): (dict(edit=(f, v)), H_MISFIT)
    for i, (f, v) in enumerate(HOST_MISFITS)})


def host_call(V, hamming, L=10, X=2, **d):
    """one raw call of the host entry -> (code, message, number of matches)"""
    sc = borders()
    q = sc.queries()
    text = np.ascontiguousarray(sc.text, np.uint8)
    sym = np.ascontiguousarray(q.symbols, np.uint8)
    seeds = sc.records()
    if "edit" in d:
        seeds = edited(sc, 5, *d["edit"])
    nseeds = 0 if d.get("seeds") == "none" else len(seeds)
    laykind = d.get("laykind", 1)
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
    args.update({k: d[k] for k in args if k in d and k != "seeds"})
    if "seeds" in d and d["seeds"] is None:
        args["seeds"] = None
    capacity = d.get("capacity", len(out))

    def run(cap):
        rc = V.lib.vsa_extend_xdrop_host(
            args["layout"], args["text"], args["querysymbols"], args["seeds"],
            nseeds, L, X, hamming, 4, 2, args["matches"], cap,
            args["numofmatches"])
        return rc, V.messagespace() if rc != 0 else None, int(n.value)

    if capacity == "one too few":
        rc, _, full = run(len(out))
        assert rc == 0 and full > 1
        return run(full - 1) + (full - 1,)
    return run(capacity) + (None,)


@pytest.mark.parametrize("defect", sorted(HOST_DEFECTS))
@pytest.mark.parametrize("hamming", MODES)
def test_what_the_host_entry_refuses(V, hamming, defect):
    change, (code, text) = HOST_DEFECTS[defect]
    rc, message, n, cap = host_call(V, hamming, **change)
    if cap is not None:
        text = text % cap
    assert (rc, message) == (code, text)
    if code == 0 and "totallength" not in change:
        assert n > 0
    elif code != 0 and not {"numofmatches", "layout", "text",
                            "matches"} & set(change):
        assert n == 0               # (set behind the first NULL checks)


# --------------------------------------------------------------------------
# the three device entries
# --------------------------------------------------------------------------

ENTRIES = ("extend", "findquerymatches", "findselfmatches")


def who(entry):
    return "vsa_%s_xdrop" % entry


def D_NULL(entry):
    return (-1, who(entry) + ": NULL argument")


def D_LAYOUT(entry):
    return (-2, who(entry) + ": the seeds of a query layout (VSA_SINK_QUERY, "
            "with their batch) or of a self layout (VSA_SINK_SELF, no batch, "
            "not palindromic) are extended")


def D_BOUND(entry):
    return (-2, who(entry) + ": a least length and a distance bound of at "
            "least 1")


def D_X(entry):
    return xbound(who(entry), 256)


def D_PACKED(entry):
    return (NC, who(entry) + ": a packed candidate result has no records to "
            "extend")


def D_EXTENDED(entry):
    return (NC, who(entry) + ": the list holds extended seeds already")


def D_MISFIT(entry):
    return (-2, who(entry) + ": 1 seeds do not fit the index or their query "
            "sequence")


# defect -> (the entries it can be put to, the change, the answer)
DEVICE_DEFECTS = {
    "null_index": (ENTRIES, dict(index=None), D_NULL),
    "null_result": (ENTRIES, dict(result=None), D_NULL),
    "null_seeds": (("extend",), dict(seeds=None), D_NULL),
    "null_layout": (("extend",), dict(layout=None), D_NULL),
    "null_queries": (("findquerymatches",), dict(queries=None), D_NULL),
    "L0": (ENTRIES, dict(L=0), D_BOUND),
    "X0": (ENTRIES, dict(X=0), D_BOUND),
    "X256": (ENTRIES, dict(X=256), D_X),
    "kind_complete": (("extend",), dict(laykind=0), D_LAYOUT),
    "kind_extended": (("extend",), dict(laykind=14), D_LAYOUT),
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
DEVICE_CASES = [(h, e, d) for h in MODES for d in sorted(DEVICE_DEFECTS)
                for e in DEVICE_DEFECTS[d][0]]

_device = {}


def device_things(V, hamming):
    """the index, the batch and the seed lists of `borders`, uploaded once"""
    if hamming not in _device:
        sc = borders()
        i = H.oracle_build_index(sc.text, 4)
        gi = V.Index.from_tables(i.n, i.prefixlength, i.numofchars, i.tis,
                                 i.suf, i.lcp, i.llv, i.bck, i.bwt,
                                 i.querysepposition, i.hasqueries)
        q = sc.queries()
        gq = V.Queries.from_host(q.symbols, q.start, q.length)
        seeds = V.Result.from_host(sc.records())
        ext = V.extend_xdrop(gi, gq, seeds, 10, 2, 4, hamming=hamming)
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
        _device[hamming] = gi, gq, seeds, lists
    return _device[hamming]


def device_call(V, hamming, entry, L=10, X=2, **d):
    gi, gq, seeds, lists = device_things(V, hamming)
    index = d.get("index", gi)
    queries = d.get("queries", gq)
    if "seeds" in d:
        seeds = lists[d["seeds"]]
        if d["seeds"] == "packed":
            index, queries = lists["of packed"]
    p = V.SinkParams()
    p.kind = d.get("laykind", 1)
    h = C.c_void_p()
    handle = lambda x: None if x is None else x._h
    result = d.get("result", C.byref(h))
    fn = getattr(V.lib, who(entry))
    before = V.device_meminfo()
    if entry == "extend":
        rc = fn(handle(index), handle(queries), handle(seeds),
                d.get("layout", C.byref(p)), d.get("palindromic", 0), L, X,
                hamming, 4, result)
    elif entry == "findquerymatches":
        rc = fn(handle(index), handle(queries), L, X, hamming, 4, 0, result)
    else:
        rc = fn(handle(index), L, X, hamming, 4, result)
    message = V.messagespace() if rc != 0 else None
    if h.value:
        V.Result(h).close()
    assert rc != 0 and not h.value
    assert V.device_meminfo() == before
    return rc, message


@pytest.mark.gpu
@pytest.mark.parametrize("hamming,entry,defect", DEVICE_CASES)
def test_what_the_device_entries_refuse(V, monkeypatch, hamming, entry,
                                        defect):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    monkeypatch.delenv("VSA_EXTEND_XDROP_BAND", raising=False)
    _, change, want = DEVICE_DEFECTS[defect]
    assert device_call(V, hamming, entry, **change) == want(entry)


@pytest.mark.gpu
def test_the_recorded_error_is_a_refusal_of_the_drivers_too(V):
    """X = 256: the reference refuses it on its command line (the recorded
    text); the drivers refuse the same bound and name it"""
    r = XC.run_of("c5_q_l40_hx256")
    assert "[1,255]" in XC.manifest()[r["key"]]["stderr"]
    for hamming in MODES:
        assert device_call(V, hamming, "findquerymatches", r["L"], r["X"]) \
            == D_X("findquerymatches")

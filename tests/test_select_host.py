"""Match selection without a GPU: the pure-Python model (select_model.py) and
vsa_select_host reproduce every recorded answer of the real reference
(tests/golden/select_*, scripts/make_golden_select.py) -- rows, order, the md5
of the lines through the sink, the number of contained matches removed -- and
agree with each other on hand-made lists."""
import numpy as np
import pytest

import helpers as H
import select_cases as SC
import select_model as SM

_inputs = {}


def run_input(case, key):
    """(recipe, records, flags, model layout, model values) of a run"""
    if (case, key) not in _inputs:
        r = SC.run_of(case, key)
        rec, flags = SC.records_of(case, r, SC.array("%s__%s__in" % (case,
                                                                    key)))
        lay = SC.model_layout(case, r)
        _inputs[case, key] = (r, rec, flags, lay,
                              SM.all_values(lay, rec, flags))
    return _inputs[case, key]


def test_the_fixtures_cover_what_was_asked_for():
    m = SC.manifest()
    assert {c: sorted(m[c]) for c in m} == \
        {c: sorted(r["key"] for r in SC.RUNS[c]) for c in SC.RUNS}
    modes = set()
    for c, k, v in SC.all_variants():
        e = m[c][k]["variants"][v]
        modes.add(e.get("sort"))
        assert m[c][k]["lines"] <= 6000
    assert modes == set(SM.SORT_MODES) | {None}
    for (c, k), filters in SC.FILTERS.items():
        for f in filters:
            assert any(all(e.get(a) == b for a, b in f.items()) and
                       not e.get("best")
                       for e in m[c][k]["variants"].values()), (c, k, f)


@pytest.mark.parametrize("case,key,vkey", SC.all_variants())
def test_model_and_host_reproduce_the_reference(V, case, key, vkey):
    r, rec, flags, lay, vals = run_input(case, key)
    e = SC.manifest()[case][key]["variants"][vkey]
    want, wantflags = SC.records_of(case, r, SC.array(
        "%s__%s__%s" % (case, key, vkey)))
    assert len(want) == e["lines"]
    opts = SC.options_of(e)
    sel, ev, st = SM.select(lay, rec, flags, vals=vals, **opts)
    assert np.array_equal(rec[sel], want)
    assert np.array_equal(flags[sel], wantflags)
    assert st["containedremoved"] == e["contained"]
    layout = V.sink_params(**SC.layout_kwargs(case, r))
    got, gotflags, gotev, gst = V.select_host(layout, rec, flags, **opts)
    assert np.array_equal(got, want)
    assert np.array_equal(gotflags, wantflags)
    assert np.array_equal(gotev, np.array(ev, np.float64))   # bit for bit
    assert gst.asdict() == st
    text = SC.format_lines(V, case, r, got, gotflags)
    assert text.count(b"\n") == e["lines"]
    assert SC.md5(text) == e["md5_lines"]


def random_list(rng, kind, n, nq=7):
    """records that need not be real matches: nothing reads the text"""
    qlen = rng.integers(40, 80, nq).astype(np.uint64)
    rec = np.zeros(n, H.MATCH_DTYPE)
    rec["dbstart"] = rng.integers(0, 40, n)
    if kind == SM.SELF:
        rec["length"] = rng.integers(8, 20, n)
        rec["queryseq"] = rec["dbstart"] + rng.integers(1, 60, n).astype(
            np.uint64)
    elif kind == SM.QUERY:
        rec["length"] = rng.integers(8, 20, n)
        rec["queryseq"] = rng.integers(0, nq, n)
        rec["querystart"] = rng.integers(0, 20, n)
    else:
        rec["queryseq"] = rng.integers(0, nq, n)
        rec["querystart"] = rng.integers(0, 5, n)        # the distance
        rec["length"] = qlen[rec["queryseq"].astype(np.int64)] + \
            rng.integers(0, 3, n).astype(np.uint64)
    flags = (rng.integers(0, 2, n).astype(np.uint8) if kind != SM.SELF
             else np.zeros(n, np.uint8))
    return rec, flags, qlen


@pytest.mark.parametrize("kind", [SM.QUERY, SM.SELF, SM.COMPLETE, SM.EDIST,
                                  SM.HAMMING])
def test_host_agrees_with_the_model_on_hand_made_lists(V, kind):
    rng = np.random.default_rng(kind)
    for n in (0, 1, 30, 400):
        rec, flags, qlen = random_list(rng, kind, n)
        # a third of the list a second time: duplicates
        rec = np.concatenate([rec, rec[:n // 3]])
        flags = np.concatenate([flags, flags[:n // 3]])
        qstart = np.concatenate(([0], np.cumsum(qlen + np.uint64(1))[:-1]))
        withq = kind != SM.SELF
        kw = dict(kind=kind, totallength=5000, markpos=[], leastlength=10)
        if withq:
            kw.update(querystart=qstart, querylength=qlen,
                      querytotallength=int(qlen.sum()) + len(qlen) - 1)
        layout = V.sink_params(**kw)
        lay = SM.Layout(kind, 5000, 4, qlen if withq else (), leastlength=10)
        vals = SM.all_values(lay, rec, flags)
        options = [dict(), dict(best=1), dict(best=7), dict(best=n + 5),
                   dict(evalue=1e-2), dict(identity=95, best=20, sort="ea"),
                   dict(leastscore=30, best=50, sort="sd")]
        options += [dict(best=max(1, n // 2), sort=s) for s in SM.SORT_MODES]
        if kind == SM.SELF:
            options += [dict(gap=[-3, 8]), dict(gap=[5], best=9, sort="ja")]
        for o in options:
            sel, ev, st = SM.select(lay, rec, flags, vals=vals, **o)
            got, gotflags, gotev, gst = V.select_host(layout, rec, flags, **o)
            assert np.array_equal(got, rec[sel]), (n, o)
            assert np.array_equal(gotflags, flags[sel]), (n, o)
            assert np.array_equal(gotev, np.array(ev, np.float64)), (n, o)
            assert gst.asdict() == st, (n, o)


def test_noevalue_and_the_long_distance_branches(V):
    qlen = np.array([600, 100], np.uint64)
    qstart = np.array([0, 601], np.uint64)
    rec = np.zeros(4, H.MATCH_DTYPE)
    rec["length"] = [600, 100, 100, 100]
    rec["queryseq"] = [0, 1, 1, 1]
    rec["querystart"] = [0, 23, 121, 3]                  # distances
    rec["dbstart"] = [1, 2, 3, 4]
    kw = dict(totallength=10 ** 6, markpos=[], querystart=qstart,
              querylength=qlen, querytotallength=701)
    lay = SM.Layout(SM.EDIST, 10 ** 6, 4, qlen)
    want = [SM.values(lay, r, 0).evalue for r in rec]
    # length 600 on four characters is below 1e-300: 0.0; so is a distance
    # beyond 120; 23 takes the branch above 20
    assert want[0] == 0.0 and want[2] == 0.0 and want[1] > 0.0
    got = V.select_host(V.sink_params(kind=SM.EDIST, **kw), rec)
    assert np.array_equal(got[2], np.array(want))
    got = V.select_host(V.sink_params(kind=SM.EDIST, showmode=V.SHOW_NOEVALUE,
                                      **kw), rec, best=4)
    assert not got[2].any()
    assert list(got[0]["dbstart"]) == [1, 2, 3, 4]       # length1 decides


def test_errors_of_the_host_form(V):
    rec = np.zeros(2, H.MATCH_DTYPE)
    rec["length"], rec["queryseq"] = 10, [50, 60]
    self_ = V.sink_params(kind=SM.SELF, totallength=100, markpos=[])
    query = V.sink_params(kind=SM.QUERY, totallength=100, markpos=[],
                          querystart=[0], querylength=[80],
                          querytotallength=80)
    with pytest.raises(V.VsaError) as e:
        V.select_host(query, rec[:0], gap=[1, 2])
    assert e.value.code == -2 and "gap" in e.value.message
    with pytest.raises(V.VsaError) as e:
        V.select_host(self_, rec, sort="la")
    assert e.value.code == -2 and "bestnumber" in e.value.message
    with pytest.raises(V.VsaError) as e:
        V.select_host(query, rec)                        # queryseq 50 of 1
    assert e.value.code == -2
    with pytest.raises(V.VsaError) as e:
        V.select_host(self_, rec, np.array([0, 1], np.uint8))
    assert e.value.code == V.NOT_COVERED
    sp = V.sink_params(kind=SM.QUERY, totallength=100, markpos=[],
                       querystart=[0], querylength=[80], querytotallength=80,
                       selfpalindromic=True, palindromic=True)
    with pytest.raises(V.VsaError) as e:
        V.select_host(sp, rec[:0])
    assert e.value.code == V.NOT_COVERED
    assert len(V.select_host(self_, rec, gap=[0], best=5)[0]) == 2


def test_every_select_entry_of_the_header_has_its_mirror(V):
    import os
    import re
    text = open(os.path.join(H.ROOT, "include", "vstree_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = set(re.findall(r"\b(vsa_select_[a-z0-9_]+)\s*\(", text))
    assert len(syms) == 9 and syms <= set(V.ABI_SYMBOLS)
    assert V.C.sizeof(V.SelectParams) == 64
    assert V.C.sizeof(V.SelectStats) == 40
    assert V.SORT_NONE == len(V.SORT_MODES) == 12
    assert V.SORT_MODES == SM.SORT_MODES

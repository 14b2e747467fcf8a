"""The X-drop extension of exact seeds on the GPU (vmatch -l L -hxdrop X |
-exdrop X): every recorded run of the real reference through the two drivers,
rows and the md5 of the sink's lines, on both table widths; vsa_extend_xdrop
on hand-made seed lists against the literal Python model
(extend_xdrop_model.py, pinned to the same recorded runs by the generator and
test_extend_xdrop_host.py) with the scans and slides forced to the lane form,
to the cooperative form and left to the budget; the band of the edit
extension against narrower groups, with the hand-over to the host rules; and
what is refused."""
import numpy as np
import pytest

import extend_cases as EC
import extend_xdrop_cases as XC
import extend_xdrop_model as XM
import helpers as H

pytestmark = pytest.mark.gpu

_index = {}


def clean(monkeypatch):
    for name in ("VSA_EXTEND_STAGE", "VSA_EXTEND_XDROP_BAND"):
        monkeypatch.delenv(name, raising=False)


def upload(V, monkeypatch, i, wide=False):
    if wide:
        i = i.as_width(64)
        monkeypatch.setenv("VSA_FORCE_WIDE", "1")
    try:
        gi = V.Index.from_tables(i.n, i.prefixlength, i.numofchars, i.tis,
                                 i.suf, i.lcp, i.llv, i.bck, i.bwt,
                                 i.querysepposition, i.hasqueries)
    finally:
        if wide:
            monkeypatch.delenv("VSA_FORCE_WIDE")
    assert gi.info().device_integersize == (64 if wide else 32)
    return gi


def golden_index(V, monkeypatch, r, wide=False):
    k = (r["case"], r["alphabet"], wide)
    if k not in _index:
        _index[k] = upload(V, monkeypatch, XC.load(r)[0], wide)
    return _index[k]


def run_drivers(V, gi, r):
    """the passes of a run through the drivers -> [(palindromic, Result)]"""
    _, q = XC.load(r)
    if not r["q"]:
        return [(0, V.findselfmatches_xdrop(gi, r["L"], r["X"], r["S"],
                                            hamming=r["hamming"]))]
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    return [(pal, V.findquerymatches_xdrop(gi, gq, r["L"], r["X"], r["S"],
                                           palindromic=pal,
                                           hamming=r["hamming"]))
            for pal in ([0] if "d" in r["strands"] else []) +
            ([1] if "p" in r["strands"] else [])]


def check_golden(V, gi, key):
    r, e = XC.run_of(key), XC.manifest()[key]
    rows, text, handed = [], [], 0
    for pal, res in run_drivers(V, gi, r):
        got = res.fetch()
        st = res.stats()
        assert st.count == len(got) <= st.candidates
        assert st.sumlength == int(V.xdrop_lengths1(got).sum())
        assert st.search_kernel_ms > 0 and st.total_device_ms > 0
        handed += st.kernel_searches
        rows.append(XC.rows_of(r, got, pal))
        text.append(V.Sink(**XC.sink_kwargs(V, r, pal)).format(got))
    assert np.array_equal(np.concatenate(rows), XC.expected_rows(key))
    assert XC.md5(b"".join(text)) == e["md5_lines"]
    # a band the widest group does not hold is handed over, and only that
    if r["hamming"] or e["maxwidth"] <= 64:
        assert handed == 0
    elif e["maxwidth"] > 64:
        assert handed > 0


@pytest.mark.parametrize("key", XC.golden_keys())
def test_golden_runs_through_the_drivers(V, monkeypatch, key):
    clean(monkeypatch)
    check_golden(V, golden_index(V, monkeypatch, XC.run_of(key)), key)


@pytest.mark.parametrize("key", XC.golden_keys())
def test_golden_runs_on_wide_tables(V, monkeypatch, key):
    clean(monkeypatch)
    check_golden(V, golden_index(V, monkeypatch, XC.run_of(key), True), key)


# --------------------------------------------------------------------------
# seed lists made by the test
# --------------------------------------------------------------------------

_scenarios = {}
_models = {}


def scenario(V, name):
    if not _scenarios:
        _scenarios.update(XC.scenarios(V.EXTEND_LANE_BUDGET,
                                       V.EXTEND_LONG_STEP))
    return _scenarios[name]


def model(sc, L, X, S, hamming):
    """computed once, shared, left unchanged; with what the generations of
    the edit extension saw"""
    k = (sc.name, L, X, S, hamming)
    if k not in _models:
        trace = {}
        rec = sc.model(L, X, S, hamming,
                       **({} if hamming else {"trace": trace}))
        rec.setflags(write=False)
        _models[k] = rec, trace
    return _models[k]


def scenario_index(V, monkeypatch, sc):
    k = ("scenario", sc.name)
    if k not in _index:
        _index[k] = upload(V, monkeypatch, H.oracle_build_index(sc.text, 4))
    return _index[k]


def batch(V, q):
    return None if q is None else V.Queries.from_host(q.symbols, q.start,
                                                      q.length)


@pytest.mark.parametrize("name", XC.SCENARIOS)
def test_extension_of_hand_made_seeds_equals_the_model(V, monkeypatch, name):
    clean(monkeypatch)
    sc = scenario(V, name)
    gi = scenario_index(V, monkeypatch, sc)
    gq, seeds = batch(V, sc.queries()), V.Result.from_host(sc.records())
    assert len(sc.text) <= 4096 and seeds.count <= 1024
    coop, some = {}, 0
    for L, X, S, hamming in XC.modes(sc):
        want, trace = model(sc, L, X, S, hamming)
        some += len(want)
        for stage in ("lane", "long", None):
            if stage is None:
                monkeypatch.delenv("VSA_EXTEND_STAGE")
            else:
                monkeypatch.setenv("VSA_EXTEND_STAGE", stage)
            res = V.extend_xdrop(gi, gq, seeds, L, X, S, hamming=hamming)
            assert np.array_equal(res.fetch(), want), (L, X, S, hamming, stage)
            st = res.stats()
            assert st.candidates == seeds.count and st.count == len(want)
            assert st.sumlength == int(XM.lengths1(want).sum())
            coop[stage] = coop.get(stage, 0) + st.searches
            # handed over: the seeds whose band outgrows 64 lanes, no others
            assert (st.kernel_searches > 0) == \
                (not hamming and trace.get("maxwidth", 0) > 64)
    assert some > 0
    assert coop["lane"] == 0
    if name != "bothempty":
        assert coop["long"] > 0
    if name == "slides":
        assert coop[None] > 0
    if name in ("borders", "borders_dense", "hspecials", "drops"):
        assert coop[None] == 0
    # a list in which every seed is dropped, and an empty list
    assert V.extend_xdrop(gi, gq, seeds, 100000, 2, hamming=True).count == 0
    empty = V.extend_xdrop(gi, gq, V.Result.from_host(sc.records()[:0]), 20,
                           2, hamming=False)
    assert empty.count == 0 and len(empty.fetch()) == 0


@pytest.mark.parametrize("name", ("tandem", "selfseeds", "manygenerations",
                                  "indels"))
def test_narrower_groups_hand_over_and_give_the_same_lists(V, monkeypatch,
                                                           name):
    """VSA_EXTEND_XDROP_BAND = 16, 32: what the widest group kept does not
    hold goes through the host rules; the lists stay what they are"""
    clean(monkeypatch)
    sc = scenario(V, name)
    gi = scenario_index(V, monkeypatch, sc)
    gq, seeds = batch(V, sc.queries()), V.Result.from_host(sc.records())
    for L, X, S, hamming in XC.modes(sc):
        if hamming:
            continue
        want, trace = model(sc, L, X, S, False)
        for band in (16, 32, 64):
            monkeypatch.setenv("VSA_EXTEND_XDROP_BAND", str(band))
            res = V.extend_xdrop(gi, gq, seeds, L, X, S, hamming=False)
            assert np.array_equal(res.fetch(), want), (L, X, S, band)
            st = res.stats()
            assert st.sumlength == int(XM.lengths1(want).sum())
            assert (st.kernel_searches > 0) == (trace.get("maxwidth", 0) > band), \
                (L, X, S, band, trace)
            assert st.kernel_searches <= seeds.count


def test_scenarios_cover_what_they_are_meant_to(V):
    assert V.XDROP_MAXDROP == 255 and V.extend_xdrop_seedlength() == 30
    # the C division of dback: X = 1, 2, 3 and the largest X
    xs = {X for name in XC.SCENARIOS for _, X, _, h in
          XC.modes(scenario(V, name)) if not h}
    assert {1, 2, 3, 255} <= xs
    # bands that pass 16, 32 and 64 diagonals; more generations than the ring
    sc = scenario(V, "tandem")
    widths = [model(sc, L, X, S, h)[1]["maxwidth"]
              for L, X, S, h in XC.modes(sc) if not h]
    assert min(widths) <= 16 and any(16 < w <= 32 for w in widths) and \
        max(widths) > 64
    sc = scenario(V, "manygenerations")
    assert all(model(sc, L, X, S, h)[1]["generations"] > 128
               for L, X, S, h in XC.modes(sc) if not h)
    # unequal lengths, the reject rule, left sides that read a separator
    sc = scenario(V, "indels")
    want = model(sc, 30, 20, 10, False)[0]
    assert (XM.lengths1(want) != XM.lengths2(want)).any()
    sc = scenario(V, "drops")
    assert len(model(sc, 14, 1, 10, True)[0]) < len(sc.seeds)
    assert model(scenario(V, "mirrored"), 10, 5, 100000,
                 False)[1]["sepreads"] > 0
    # pairs of self seeds 1 .. 9 apart
    gaps = {abs(int(b) - int(a)) for _, a, b, _ in
            scenario(V, "selfseeds").seeds}
    assert set(range(1, 10)) <= gaps


def test_the_mirrored_left_case(V, monkeypatch):
    """left sides whose record depends on ulen / vlen being state and on the
    order of the diagonals within a generation: the model with the lengths
    frozen and the model with every diagonal under the lengths of the start
    of its generation each give another result; host code and kernel give
    the reference's"""
    clean(monkeypatch)
    sc = scenario(V, "mirrored")
    L, X, S, _ = sc.params[0]
    recs = sc.records()
    literal = XM.matches(recs, sc.text, X, False, S, sc.triple())[0]
    frozen = XM.matches(recs, sc.text, X, False, S, sc.triple(),
                        frozen=True)[0]
    unordered = XM.matches(recs, sc.text, X, False, S, sc.triple(),
                           unordered=True)[0]
    both = [i for i in range(len(recs))
            if literal[i] != frozen[i] and literal[i] != unordered[i]]
    assert len(both) >= 3
    want = model(sc, L, X, S, False)[0]
    gi = scenario_index(V, monkeypatch, sc)
    res = V.extend_xdrop(gi, batch(V, sc.queries()), V.Result.from_host(recs),
                         L, X, S, hamming=False)
    assert np.array_equal(res.fetch(), want)
    assert np.array_equal(V.extend_xdrop_host(sc.text, recs, L, X, S,
                                              queries=sc.triple(),
                                              hamming=False), want)
    # ... seed by seed, so that the records of those seeds are compared
    for i in both[:3]:
        one = V.extend_xdrop(gi, batch(V, sc.queries()),
                             V.Result.from_host(recs[i:i + 1]), 1, X, S,
                             hamming=False).fetch()
        assert np.array_equal(one, XM.extend(recs[i:i + 1], sc.text, 1, X,
                                             False, S, sc.triple()))


def test_reverse_complement_pass_and_packed_reads(V, monkeypatch):
    clean(monkeypatch)
    sc = scenario(V, "borders_dense")
    gi = scenario_index(V, monkeypatch, sc)
    q, seeds = sc.queries(), V.Result.from_host(sc.records())
    for L, X, S, hamming in XC.modes(sc)[:2]:
        want = model(sc, L, X, S, hamming)[0]
        # palindromic: the seeds lie on the reverse complement of the batch
        fwd = EC.reverse_complement(q)
        got = V.extend_xdrop(gi, batch(V, fwd), seeds, L, X, S,
                             palindromic=True, hamming=hamming)
        assert np.array_equal(got.fetch(), want)
        # reads at two bits per symbol are expanded to bytes first
        packed = V.Queries.from_host_packed(q.symbols, int(q.length[0]))
        got = V.extend_xdrop(gi, packed, seeds, L, X, S, hamming=hamming)
        assert np.array_equal(got.fetch(), want)


def test_handles_refuse_lists_of_extended_seeds(V, monkeypatch):
    clean(monkeypatch)
    sc = scenario(V, "borders")
    gi = scenario_index(V, monkeypatch, sc)
    q = sc.queries()
    gq, seeds = batch(V, q), V.Result.from_host(sc.records())
    res = V.extend_xdrop(gi, gq, seeds, 10, 2, 4, hamming=False)
    assert res.count > 0
    qs, ql, total = EC.query_multiseq(q)
    kw = dict(totallength=len(sc.text), markpos=[], querystart=qs,
              querylength=ql, querytotallength=total)
    sel = V.Select(V.sink_params(kind=V.SINK_QUERY, **kw), gq)
    with pytest.raises(V.VsaError) as e:
        sel.add(res)
    assert e.value.code == V.NOT_COVERED and sel.stats().seen == 0
    cov = V.Coverage.over_index(gi)
    with pytest.raises(V.VsaError) as e:
        cov.mark(res)
    assert e.value.code == V.NOT_COVERED and cov.stats().marked == 0
    # ... and a layout of the new kinds opens none of them
    for kind in (V.SINK_QUERY_HXDROP, V.SINK_QUERY_EXDROP):
        with pytest.raises(V.VsaError) as e:
            V.Select(V.sink_params(kind=kind, **kw), gq)
        assert e.value.code == V.NOT_COVERED
    # an extended list is not extended again
    with pytest.raises(V.VsaError) as e:
        V.extend_xdrop(gi, gq, res, 10, 2, hamming=True)
    assert e.value.code == V.NOT_COVERED
    # the list travels like any other
    back = V.Result.from_host(res.fetch())
    assert np.array_equal(back.fetch(), res.fetch())

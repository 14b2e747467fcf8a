"""Degenerate matches by edit distance on the GPU (vmatch -l L -e K outside
-complete): every recorded run of the real reference through the two drivers,
rows and the md5 of the sink's lines, on both table widths; vsa_extend_edist
on hand-made seed lists against the literal Python model
(extend_edist_model.py, pinned to the same recorded runs by the generator and
test_extend_edist_host.py) with the slides forced to the lane form, to the
cooperative form and left to the budget; the seed list in several pieces of
scratch; and what is refused."""
import numpy as np
import pytest

import extend_cases as EC
import extend_edist_cases as DC
import extend_edist_model as DM
import helpers as H

pytestmark = pytest.mark.gpu

_index = {}


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
        _index[k] = upload(V, monkeypatch, DC.load(r)[0], wide)
    return _index[k]


def run_drivers(V, gi, r):
    """the passes of a run through the drivers -> [(palindromic, Result)]"""
    _, q = DC.load(r)
    if not r["q"]:
        return [(0, V.findselfmatches_edist(gi, r["L"], r["K"], r["S"]))]
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    return [(pal, V.findquerymatches_edist(gi, gq, r["L"], r["K"], r["S"],
                                           palindromic=pal))
            for pal in ([0] if "d" in r["strands"] else []) +
            ([1] if "p" in r["strands"] else [])]


def check_golden(V, gi, key):
    r, e = DC.run_of(key), DC.manifest()[key]
    rows, text = [], []
    for pal, res in run_drivers(V, gi, r):
        got = res.fetch()
        st = res.stats()
        assert st.count == len(got) <= st.candidates
        assert st.sumlength == int(V.edist_lengths1(got).sum())
        assert st.search_kernel_ms > 0 and st.total_device_ms > 0
        rows.append(DC.rows_of(r, got, pal))
        text.append(V.Sink(**DC.sink_kwargs(V, r, pal)).format(got))
    want = DC.expected_rows(key)
    assert np.array_equal(np.concatenate(rows), want)
    assert (want[:, 0] != want[:, 3]).any()
    assert DC.md5(b"".join(text)) == e["md5_lines"]


@pytest.mark.parametrize("key", DC.golden_keys())
def test_golden_runs_through_the_drivers(V, monkeypatch, key):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    monkeypatch.delenv("VSA_EXTEND_EDIST_SCRATCH", raising=False)
    check_golden(V, golden_index(V, monkeypatch, DC.run_of(key)), key)


@pytest.mark.parametrize("key", DC.golden_keys())
def test_golden_runs_on_wide_tables(V, monkeypatch, key):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    monkeypatch.delenv("VSA_EXTEND_EDIST_SCRATCH", raising=False)
    check_golden(V, golden_index(V, monkeypatch, DC.run_of(key), True), key)


def test_the_recorded_error_comes_back_verbatim(V, monkeypatch):
    r = DC.run_of("c5_q_l10_e2")
    gi = golden_index(V, monkeypatch, r)
    _, q = DC.load(r)
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    for pal in (False, True):
        with pytest.raises(V.VsaError) as e:
            V.findquerymatches_edist(gi, gq, r["L"], r["K"], r["S"], pal)
        assert e.value.message == DC.manifest()[r["key"]]["stderr"]


# --------------------------------------------------------------------------
# seed lists made by the test
# --------------------------------------------------------------------------

_scenarios = {}
_models = {}


def scenario(V, name):
    if not _scenarios:
        _scenarios.update(DC.scenarios(V.EXTEND_LANE_BUDGET))
    return _scenarios[name]


def model(sc, L, K, S):
    """computed once, shared, left unchanged"""
    k = (sc.name, L, K, S)
    if k not in _models:
        _models[k] = sc.model(L, K, S)
        _models[k].setflags(write=False)
    return _models[k]


def scenario_index(V, monkeypatch, sc):
    k = ("scenario", sc.name)
    if k not in _index:
        _index[k] = upload(V, monkeypatch, H.oracle_build_index(sc.text, 4))
    return _index[k]


def batch(V, q):
    return None if q is None else V.Queries.from_host(q.symbols, q.start,
                                                      q.length)


@pytest.mark.parametrize("name", DC.SCENARIOS)
def test_extension_of_hand_made_seeds_equals_the_model(V, monkeypatch, name):
    monkeypatch.delenv("VSA_EXTEND_EDIST_SCRATCH", raising=False)
    sc = scenario(V, name)
    gi = scenario_index(V, monkeypatch, sc)
    gq, seeds = batch(V, sc.queries()), V.Result.from_host(sc.records())
    assert len(sc.text) <= 4096 and seeds.count <= 1024
    coop, some = {}, 0
    for L, K, S in sc.params:
        assert K <= V.EXTEND_EDIST_MAXDIST
        want = model(sc, L, K, S)
        some += len(want)
        for stage in ("lane", "long", None):
            if stage is None:
                monkeypatch.delenv("VSA_EXTEND_STAGE")
            else:
                monkeypatch.setenv("VSA_EXTEND_STAGE", stage)
            res = V.extend_edist(gi, gq, seeds, L, K, S)
            assert np.array_equal(res.fetch(), want), (L, K, S, stage)
            st = res.stats()
            assert st.candidates == seeds.count and st.count == len(want)
            assert st.sumlength == int(DM.lengths1(want).sum())
            coop[stage] = coop.get(stage, 0) + st.searches
    assert some > 0 or name == "bothempty"
    assert coop["lane"] == 0
    if name != "bothempty":
        assert coop["long"] > 0
    # the group finishes a slide only where the budget does not suffice
    if name == "words":
        assert coop[None] > 0
    if name in ("borders", "borders_dense", "specials", "indels"):
        assert coop[None] == 0
    # a list in which every seed is dropped, and an empty list
    assert V.extend_edist(gi, gq, seeds, 100000, 2).count == 0
    empty = V.extend_edist(gi, gq, V.Result.from_host(sc.records()[:0]), 20, 2)
    assert empty.count == 0 and len(empty.fetch()) == 0


def test_scenarios_cover_what_they_are_meant_to(V):
    assert V.EXTEND_EDIST_MAXDIST == 31 and V.EDIST_MAXDISTANCE == 125
    assert len(DC.residues(scenario(V, "words"))) == 64
    ks = {K for _, K, _ in scenario(V, "everywidth").params}
    assert ks == set(DC.KS) and max(ks) == V.EXTEND_EDIST_MAXDIST
    # unequal lengths, and distances up to a bound of 8
    sc = scenario(V, "indels")
    want = model(sc, 50, 8, 0)
    assert (DM.lengths1(want) != DM.lengths2(want)).any()
    assert int(DM.distances(model(scenario(V, "everywidth"), 40, 31,
                                  0)).max()) > 16
    # the ties: every match of this list is longer than the E-value table,
    # so every candidate of it has the E-value 0.0 and identity, then length,
    # then "later wins" decide
    from extend_model import Evalues
    ev = Evalues(4)
    ties = model(scenario(V, "fewerrors"), *DC.TIES)
    assert len(ties) >= 2 and DC.TIES in scenario(V, "fewerrors").params
    assert int(np.minimum(DM.lengths1(ties), DM.lengths2(ties)).min()) >= 700
    assert all(DM.incgetevalue(ev, 1.0, d, n) == 0.0
               for d in range(DC.TIES[1] + 1) for n in (700, 720, 840, 900))
    # pairs of self seeds 1 .. K + 1 apart for the largest K
    sc = scenario(V, "selfseeds")
    gaps = {abs(int(b) - int(a)) for _, a, b, _ in sc.seeds}
    assert set(range(1, max(K for _, K, _ in sc.params) + 2)) <= gaps


def test_the_seed_list_in_pieces_of_scratch(V, monkeypatch):
    """a scratch budget of a few seeds: many pieces, the same list"""
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    sc = scenario(V, "indels")
    gi = scenario_index(V, monkeypatch, sc)
    gq, seeds = batch(V, sc.queries()), V.Result.from_host(sc.records())
    L, K, S = 40, 5, 0
    # 8 (K + 1)^2 bytes per seed: 7 seeds per piece, then one
    for nbytes in (7 * 8 * 36, 1):
        monkeypatch.setenv("VSA_EXTEND_EDIST_SCRATCH", str(nbytes))
        res = V.extend_edist(gi, gq, seeds, L, K, S)
        assert np.array_equal(res.fetch(), model(sc, L, K, S))


def test_reverse_complement_pass_and_packed_reads(V, monkeypatch):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    monkeypatch.delenv("VSA_EXTEND_EDIST_SCRATCH", raising=False)
    sc = scenario(V, "borders_dense")
    gi = scenario_index(V, monkeypatch, sc)
    q, seeds = sc.queries(), V.Result.from_host(sc.records())
    L, K, S = sc.params[0]
    want = model(sc, L, K, S)
    # palindromic: the seeds lie on the reverse complement of the batch
    fwd = EC.reverse_complement(q)
    got = V.extend_edist(gi, batch(V, fwd), seeds, L, K, S, palindromic=True)
    assert np.array_equal(got.fetch(), want)
    # reads at two bits per symbol are expanded to bytes first
    packed = V.Queries.from_host_packed(q.symbols, int(q.length[0]))
    got = V.extend_edist(gi, packed, seeds, L, K, S)
    assert np.array_equal(got.fetch(), want)


def test_what_is_refused_leaves_the_device_untouched(V, monkeypatch):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    monkeypatch.delenv("VSA_EXTEND_EDIST_SCRATCH", raising=False)
    sc = scenario(V, "borders")
    gi = scenario_index(V, monkeypatch, sc)
    gq, seeds = batch(V, sc.queries()), V.Result.from_host(sc.records())
    V.extend_edist(gi, gq, seeds, 10, 2).close()
    before = V.device_meminfo()
    K = V.EXTEND_EDIST_MAXDIST + 1
    assert K == 32
    for call in (lambda: V.extend_edist(gi, gq, seeds, 10, K),
                 lambda: V.findquerymatches_edist(gi, gq, 10, K),
                 lambda: V.findselfmatches_edist(gi, 10, K)):
        with pytest.raises(V.VsaError) as e:
            call()
        assert e.value.code == V.NOT_COVERED
        assert V.device_meminfo() == before
    # the host path takes that bound
    assert np.array_equal(
        V.extend_edist_host(sc.text, sc.records(), 10, K,
                            queries=sc.triple()), sc.model(10, K, 0))
    # a packed-pair seed list has no records
    c1, cq = H.load_case("c1")
    ci = upload(V, monkeypatch, c1)
    cgq = V.Queries.from_host(cq.symbols, cq.start, cq.length)
    packed = V.findmumcandidates_packed(ci, cgq, 20)
    assert packed.count > 0 and packed.packbits
    before = V.device_meminfo()
    with pytest.raises(V.VsaError) as e:
        V.extend_edist(ci, cgq, packed, 40, 2)
    assert e.value.code == V.NOT_COVERED and V.device_meminfo() == before
    # a seed that does not fit its texts is read by no kernel
    # ... and the call that finds it gives all its scratch back
    for field, value in (("dbstart", len(sc.text) - 1), ("queryseq", 1 << 40),
                         ("querystart", 1 << 33), ("length", 0),
                         ("length", 1 << 50)):
        bad = sc.records()
        bad[field][7] = value
        badseeds = V.Result.from_host(bad)
        before = V.device_meminfo()
        with pytest.raises(V.VsaError) as e:
            V.extend_edist(gi, gq, badseeds, 10, 2)
        assert e.value.code == -2 and "1 seeds do not fit" in e.value.message
        assert V.device_meminfo() == before
        badseeds.close()
    before = V.device_meminfo()
    for L, K in ((0, 2), (10, 0)):
        with pytest.raises(V.VsaError) as e:
            V.extend_edist(gi, gq, seeds, L, K)
        assert e.value.code == -2
        assert V.device_meminfo() == before
    # a self layout takes no batch, a query layout needs one
    with pytest.raises(V.VsaError) as e:
        V.extend_edist(gi, None, seeds, 10, 2, palindromic=True)
    assert e.value.code == -2


def test_handles_refuse_lists_of_extended_seeds(V, monkeypatch):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    monkeypatch.delenv("VSA_EXTEND_EDIST_SCRATCH", raising=False)
    sc = scenario(V, "borders")
    gi = scenario_index(V, monkeypatch, sc)
    q = sc.queries()
    gq, seeds = batch(V, q), V.Result.from_host(sc.records())
    res = V.extend_edist(gi, gq, seeds, 10, 2)
    assert res.count > 0
    qs, ql, total = EC.query_multiseq(q)
    kw = dict(totallength=len(sc.text), markpos=[], querystart=qs,
              querylength=ql, querytotallength=total)
    sel = V.Select(V.sink_params(kind=V.SINK_QUERY, **kw), gq)
    with pytest.raises(V.VsaError) as e:
        sel.add(res)
    assert e.value.code == V.NOT_COVERED and sel.stats().seen == 0
    sel.add(seeds)
    assert sel.stats().seen == seeds.count
    cov = V.Coverage.over_index(gi)
    with pytest.raises(V.VsaError) as e:
        cov.mark(res)
    assert e.value.code == V.NOT_COVERED and cov.stats().marked == 0
    # ... and a layout of the new kinds opens none of them
    with pytest.raises(V.VsaError) as e:
        V.Select(V.sink_params(kind=V.SINK_QUERY_EDIST, **kw), gq)
    assert e.value.code == V.NOT_COVERED
    # an extended list is not extended again
    with pytest.raises(V.VsaError) as e:
        V.extend_edist(gi, gq, res, 10, 2)
    assert e.value.code == V.NOT_COVERED
    # the list travels like any other
    back = V.Result.from_host(res.fetch())
    assert np.array_equal(back.fetch(), res.fetch())

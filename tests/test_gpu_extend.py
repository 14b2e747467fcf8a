"""Degenerate matches on the GPU (vmatch -l L -h K outside -complete): every
recorded run of the real reference through the two drivers, order and
distances included, on both table widths; vsa_extend_hamming on hand-made
seed lists against the pure-Python model (extend_model.py, pinned to the
same recorded runs by test_extend_host.py) -- the borders of both texts,
separators and wildcards, every alignment of the two texts in memory, the
last mismatch around the words, the scan budget and the step of the long
stage, the left stop rule, few mismatches, long seeds, several distance
bounds up to the cap -- with the scan stages forced in turn; and what is
refused."""
import numpy as np
import pytest

import extend_cases as EC
import extend_model as EM
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
        _index[k] = upload(V, monkeypatch, EC.load(r)[0], wide)
    return _index[k]


def run_drivers(V, gi, r):
    """the passes of a run through the drivers -> [(palindromic, Result)]"""
    _, q = EC.load(r)
    if not r["q"]:
        return [(0, V.findselfmatches_hamming(gi, r["L"], r["K"], r["S"]))]
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    return [(pal, V.findquerymatches_hamming(gi, gq, r["L"], r["K"], r["S"],
                                             palindromic=pal))
            for pal in ([0] if "d" in r["strands"] else []) +
            ([1] if "p" in r["strands"] else [])]


def check_golden(V, gi, key):
    r, e = EC.run_of(key), EC.manifest()[key]
    rows, text = [], []
    for pal, res in run_drivers(V, gi, r):
        got = res.fetch()
        st = res.stats()
        assert st.count == len(got) <= st.candidates
        assert st.sumlength == int(V.hamming_lengths(got).sum())
        assert st.search_kernel_ms > 0 and st.total_device_ms > 0
        rows.append(EC.rows_of(r, got, pal))
        text.append(V.Sink(**EC.sink_kwargs(V, r, pal)).format(got))
    assert np.array_equal(np.concatenate(rows), EC.expected_rows(key))
    assert EC.md5(b"".join(text)) == e["md5_lines"]


@pytest.mark.parametrize("key", EC.golden_keys())
def test_golden_runs_through_the_drivers(V, monkeypatch, key):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    check_golden(V, golden_index(V, monkeypatch, EC.run_of(key)), key)


@pytest.mark.parametrize("key", ["c5_q_l40_h2", "grumbach_q_l30_h2_dp",
                                 "grumbach_all_l30_h2", "prot_l12_h2"])
def test_golden_runs_on_wide_tables(V, monkeypatch, key):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    check_golden(V, golden_index(V, monkeypatch, EC.run_of(key), True), key)


def test_the_recorded_error_comes_back_verbatim(V, monkeypatch):
    r = EC.run_of("c5_q_l10_h2")
    gi = golden_index(V, monkeypatch, r)
    _, q = EC.load(r)
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    for pal in (False, True):
        with pytest.raises(V.VsaError) as e:
            V.findquerymatches_hamming(gi, gq, r["L"], r["K"], r["S"], pal)
        assert e.value.message == EC.manifest()[r["key"]]["stderr"]


# --------------------------------------------------------------------------
# seed lists made by the test
# --------------------------------------------------------------------------

_scenarios = {}


def scenario(V, name):
    if not _scenarios:
        _scenarios.update(EC.scenarios(V.EXTEND_LANE_BUDGET,
                                       V.EXTEND_LONG_STEP))
    return _scenarios[name]


def scenario_index(V, monkeypatch, sc, wide=False):
    k = ("scenario", sc.name, wide)
    if k not in _index:
        _index[k] = upload(V, monkeypatch, H.oracle_build_index(sc.text, 4),
                           wide)
    return _index[k]


def batch(V, q):
    return None if q is None else V.Queries.from_host(q.symbols, q.start,
                                                      q.length)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("name", EC.SCENARIOS)
def test_extension_of_hand_made_seeds_equals_the_model(V, monkeypatch, name,
                                                       wide):
    sc = scenario(V, name)
    gi = scenario_index(V, monkeypatch, sc, wide)
    gq, seeds = batch(V, sc.queries()), V.Result.from_host(sc.records())
    assert len(sc.text) <= 8192 and seeds.count <= 2048
    tolong = {}
    for L, K, S in sc.params:
        assert K <= V.EXTEND_MAXDIST
        want = sc.model(L, K, S)
        # the lane scan and the long stage, each forced, and the two together
        for stage in ("lane", "long", None):
            if stage is None:
                monkeypatch.delenv("VSA_EXTEND_STAGE")
            else:
                monkeypatch.setenv("VSA_EXTEND_STAGE", stage)
            res = V.extend_hamming(gi, gq, seeds, L, K, S)
            assert np.array_equal(res.fetch(), want), (L, K, S, stage)
            st = res.stats()
            assert st.candidates == seeds.count and st.count == len(want)
            assert st.sumlength == int(EM.lengths(want).sum())
            tolong[stage] = tolong.get(stage, 0) + st.searches
    assert tolong["lane"] == 0 < tolong["long"]
    # a side goes to the long stage only where the budget does not suffice
    if name in ("budget", "longstep"):
        assert tolong[None] > 0
    if name in ("borders", "borders_dense", "specials", "stoprule"):
        assert tolong[None] == 0    # no side of theirs has that many symbols
    # a list in which every seed is dropped, and an empty list
    assert V.extend_hamming(gi, gq, seeds, 100000, 2).count == 0
    empty = V.extend_hamming(gi, gq, V.Result.from_host(sc.records()[:0]), 20,
                             2)
    assert empty.count == 0 and len(empty.fetch()) == 0


def test_scenarios_cover_what_they_are_meant_to(V):
    sc = scenario(V, "alignment")
    assert len(EC.alignment_residues(sc)) == 64
    assert V.EXTEND_LANE_BUDGET % 8 == 0 and V.EXTEND_MAXDIST >= 32
    assert V.EXTEND_LONG_STEP == 64 * 16
    assert any(K == V.EXTEND_MAXDIST for _, K, _ in sc.params)
    # the long match: every E-value of its candidates is 0.0
    ev = EM.Evalues(4)
    assert all(ev.lookup(d, 650) == 0.0 for d in range(6))


def test_reverse_complement_pass_and_packed_reads(V, monkeypatch):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    sc = scenario(V, "borders_dense")
    gi = scenario_index(V, monkeypatch, sc)
    q, seeds = sc.queries(), V.Result.from_host(sc.records())
    L, K, S = sc.params[0]
    want = sc.model(L, K, S)
    # palindromic: the seeds lie on the reverse complement of the batch
    fwd = EC.reverse_complement(q)
    got = V.extend_hamming(gi, batch(V, fwd), seeds, L, K, S,
                           palindromic=True)
    assert np.array_equal(got.fetch(), want)
    # reads at two bits per symbol are expanded to bytes first
    m = int(q.length[0])
    packed = V.Queries.from_host_packed(q.symbols, m)
    got = V.extend_hamming(gi, packed, seeds, L, K, S)
    assert np.array_equal(got.fetch(), want)


def test_what_is_refused_leaves_the_device_untouched(V, monkeypatch):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    sc = scenario(V, "borders")
    gi = scenario_index(V, monkeypatch, sc)
    gq, seeds = batch(V, sc.queries()), V.Result.from_host(sc.records())
    V.extend_hamming(gi, gq, seeds, 10, 2).close()
    before = V.device_meminfo()
    for call in (
            lambda: V.extend_hamming(gi, gq, seeds, 10,
                                     V.EXTEND_MAXDIST + 1),
            lambda: V.findquerymatches_hamming(gi, gq, 10,
                                               V.EXTEND_MAXDIST + 1),
            lambda: V.findselfmatches_hamming(gi, 10,
                                              V.EXTEND_MAXDIST + 1)):
        with pytest.raises(V.VsaError) as e:
            call()
        assert e.value.code == V.NOT_COVERED
        assert V.device_meminfo() == before
    # the host path takes that bound
    K = V.EXTEND_MAXDIST + 1
    assert np.array_equal(
        V.extend_hamming_host(sc.text, sc.records(), 10, K,
                              queries=(sc.queries().symbols,
                                       sc.queries().start,
                                       sc.queries().length)),
        sc.model(10, K, 0))
    # a seed that does not fit its texts is read by no kernel
    for field, value in (("dbstart", len(sc.text) - 1), ("queryseq", 1 << 40),
                         ("querystart", 1 << 33), ("length", 0),
                         ("length", 1 << 50)):
        bad = sc.records()
        bad[field][7] = value
        with pytest.raises(V.VsaError) as e:
            V.extend_hamming(gi, gq, V.Result.from_host(bad), 10, 2)
        assert e.value.code == -2 and "1 seeds do not fit" in e.value.message
    for L, K in ((0, 2), (10, 0)):
        with pytest.raises(V.VsaError) as e:
            V.extend_hamming(gi, gq, seeds, L, K)
        assert e.value.code == -2
    # a self layout takes no batch, a query layout needs one
    with pytest.raises(V.VsaError) as e:
        V.extend_hamming(gi, None, seeds, 10, 2, palindromic=True)
    assert e.value.code == -2


def test_handles_refuse_lists_of_extended_seeds(V, monkeypatch):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    sc = scenario(V, "borders")
    gi = scenario_index(V, monkeypatch, sc)
    q = sc.queries()
    gq, seeds = batch(V, q), V.Result.from_host(sc.records())
    res = V.extend_hamming(gi, gq, seeds, 10, 2)
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
        V.Select(V.sink_params(kind=V.SINK_QUERY_HAMMING, **kw), gq)
    assert e.value.code == V.NOT_COVERED
    # the list travels like any other
    back = V.Result.from_host(res.fetch())
    assert np.array_equal(back.fetch(), res.fetch())

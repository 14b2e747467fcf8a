"""Match selection on the GPU (vsa_select_*): every recorded run of the real
reference through the engine's entry points and the selection; the E-values
of the kernels bit for bit against the model; and the kernels against the
pure-Python model (select_model.py) on hand-made lists -- sizes around the
wavefront and the workgroup tile, N around the groups of equal keys, ties on
every word of the key, duplicates, accumulation over several lists, the
filters alone, and the forms that are refused."""
import numpy as np
import pytest

import helpers as H
import select_cases as SC
import select_model as SM

pytestmark = pytest.mark.gpu

TILE = 1024
_engine = {}


def engine_lists(V, case, key):
    """the match lists of a recorded run from the real entry points ->
    ([(Result, palindromic)], the batch or None)"""
    if (case, key) in _engine:
        return _engine[case, key]
    r = SC.run_of(case, key)
    i, q = H.load_case(case)
    if case not in _engine:
        _engine[case] = V.Index.from_tables(
            i.n, i.prefixlength, i.numofchars, i.tis, i.suf, i.lcp, i.llv,
            i.bck, i.bwt, i.querysepposition, i.hasqueries)
    gi, eng, L = _engine[case], r["engine"], r["L"]
    gq, out = None, []
    if eng == "repeats":
        out = [(V.findmaximalrepeats(gi, L), False)]
    elif eng == "supermax":
        out = [(V.findsupermaximalrepeats(gi, L), False)]
    elif eng == "tandem":
        out = [(V.findtandems(gi, L), False)]
    else:
        gq = V.Queries.from_host(q.symbols, q.start, q.length)
        if eng == "complete":
            out = [(V.findapproxcompletematches(gi, gq, r["approx"][0],
                                                r["approx"][1]), False)]
        else:
            if "d" in r["strands"]:
                out.append((V.findquerymatches(gi, gq, L), False))
            if "p" in r["strands"]:
                rc = gq.reverse_complement()
                out.append((V.findquerymatches(gi, rc, L), True))
    _engine[case, key] = (out, gq)
    return _engine[case, key]


@pytest.mark.parametrize("case,key,vkey", SC.all_variants())
def test_golden_runs_through_the_engine(V, case, key, vkey):
    r = SC.run_of(case, key)
    e = SC.manifest()[case][key]["variants"][vkey]
    lists, gq = engine_lists(V, case, key)
    assert sum(x.count for x, _ in lists) == SC.manifest()[case][key]["lines"]
    want, wantflags = SC.records_of(case, r, SC.array(
        "%s__%s__%s" % (case, key, vkey)))
    sel = V.Select(V.sink_params(**SC.layout_kwargs(case, r)), gq,
                   **SC.options_of(e))
    for x, pal in lists:
        sel.add(x, pal)
    res = sel.finish()
    got = res.fetch()
    flags = sel.flags(len(got))
    assert np.array_equal(got, want)
    assert np.array_equal(flags, wantflags)
    st = sel.stats()
    assert st.seen == SC.manifest()[case][key]["lines"]
    assert st.selected == e["lines"] and st.duplicates == 0
    assert st.containedremoved == e["contained"]
    if not e.get("best"):
        assert st.rejected == st.seen - e["lines"]
    text = SC.format_lines(V, case, r, got, flags)
    assert text.count(b"\n") == e["lines"]
    assert SC.md5(text) == e["md5_lines"]


# --------------------------------------------------------------------------
# E-values: bit for bit the model's
# --------------------------------------------------------------------------

def ragged_batch(V, lengths):
    lengths = np.asarray(lengths, np.uint64)
    start = np.concatenate(([0], np.cumsum(lengths + np.uint64(1))[:-1]))
    total = int(lengths.sum()) + len(lengths) - 1
    sym = np.zeros(total, np.uint8)
    sym[(start[1:] - np.uint64(1)).astype(np.int64)] = H.SEPARATOR
    return V.Queries.from_host(sym, start, lengths), start, lengths, total


@pytest.mark.parametrize("kind", [SM.QUERY, SM.COMPLETE, SM.EDIST,
                                  SM.HAMMING])
def test_evalues_equal_the_models_bit_for_bit(V, kind):
    gq, start, lengths, total = ragged_batch(V, np.arange(100, 152))
    nq, n = len(lengths), 3000003
    rec = np.zeros(nq * 6, H.MATCH_DTYPE)
    rec["queryseq"] = np.repeat(np.arange(nq), 6)
    qlen = lengths[rec["queryseq"].astype(np.int64)]
    rec["dbstart"] = np.arange(len(rec)) * 7
    if kind == SM.QUERY:
        rec["length"] = qlen - np.tile(np.arange(6), nq).astype(np.uint64) * 9
        rec["querystart"] = np.tile(np.arange(6), nq)
    else:
        rec["length"] = qlen + np.tile([0, 1, 2, 0, 3, 5], nq).astype(
            np.uint64)
        rec["querystart"] = np.tile(np.arange(6), nq)    # distances 0..5
    layout = V.sink_params(kind=kind, totallength=n, markpos=[],
                           querystart=start, querylength=lengths,
                           querytotallength=total)
    lay = SM.Layout(kind, n, 4, lengths)
    for queries in (gq, None):
        sel = V.Select(layout, queries)
        for pal in (False, True):
            got = sel.evalues(V.Result.from_host(rec), pal)
            want = np.array([SM.values(lay, x, pal).evalue for x in rec])
            assert np.array_equal(got, want)             # == on float64
            assert (want > 0).all()


def test_evalues_of_long_distances_and_long_matches(V):
    gq, start, lengths, total = ragged_batch(V, [600, 100, 130])
    rec = np.zeros(6, H.MATCH_DTYPE)
    rec["length"] = [600, 100, 100, 100, 131, 130]
    rec["queryseq"] = [0, 1, 1, 1, 2, 2]
    rec["querystart"] = [0, 23, 121, 20, 21, 64]
    for kind in (SM.EDIST, SM.HAMMING):
        layout = V.sink_params(kind=kind, totallength=10 ** 6, markpos=[],
                               querystart=start, querylength=lengths,
                               querytotallength=total)
        lay = SM.Layout(kind, 10 ** 6, 4, lengths)
        want = np.array([SM.values(lay, x, 0).evalue for x in rec])
        # length 600 on four characters: the table has ended, 0.0
        assert want[0] == 0.0
        if kind == SM.EDIST:
            # 23 and 21 take the branch above 20; beyond 120 it is 0.0
            assert want[1] > 0 and want[4] > 0 and want[2] == 0.0
        got = V.Select(layout, gq).evalues(V.Result.from_host(rec))
        assert np.array_equal(got, want)
        host = V.select_host(layout, rec)[2]
        assert np.array_equal(host, want)


# --------------------------------------------------------------------------
# hand-made lists against the model
# --------------------------------------------------------------------------

SELFLEN = 1 << 40        # positions beyond 2^32 are positions like others


def self_layout(V, **kw):
    kw.setdefault("leastlength", 1)
    return (V.sink_params(kind=SM.SELF, totallength=SELFLEN, markpos=[],
                          **{k: v for k, v in kw.items()
                             if k in ("leastlength", "showmode")}),
            SM.Layout(SM.SELF, SELFLEN, 4, leastlength=kw["leastlength"],
                      noevalue=bool(kw.get("showmode", 0) & 4)))


def self_records(length, pos1, pos2):
    n = [np.size(x) for x in (length, pos1, pos2) if np.ndim(x)][0]
    rec = np.zeros(n, H.MATCH_DTYPE)
    rec["length"], rec["dbstart"], rec["queryseq"] = length, pos1, pos2
    return rec


def gpu_select(V, layout, lists, queries=None, **opts):
    """lists: [(records, palindromic)] -> (records, flags, stats)"""
    sel = V.Select(layout, queries, **opts)
    for rec, pal in lists:
        sel.add(V.Result.from_host(rec), pal)
    got = sel.finish().fetch()
    return got, sel.flags(len(got)), sel.stats()


def check(V, layout, lay, rec, dupsdefined=True, **opts):
    sel, ev, st = SM.select(lay, rec, None, **opts)
    got, flags, gst = gpu_select(V, layout, [(rec, False)], **opts)
    assert np.array_equal(got, rec[sel]), opts
    assert not flags.any()
    g = gst.asdict()
    if not dupsdefined:
        g.pop("duplicates"), st.pop("duplicates")
    assert g == st, opts


def ladder(kind, n, rng):
    """n records whose keys tie down to one word"""
    i = rng.permutation(n).astype(np.uint64)
    if kind == "pos1":       # all equal but for the low bits of position1
        return self_records(30, i * np.uint64(3), 1 << 20)
    if kind == "pos1high":   # ... but for bits above bit 32
        return self_records(30, i << np.uint64(33), 1 << 39)
    if kind == "pos2":       # equal down to position2
        return self_records(30, 5, np.uint64(100) + i)
    # groups of equal E-value and length: 16 lengths
    return self_records(20 + (i % np.uint64(16)), i, i + np.uint64(1 << 34))


SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_n_around_the_groups_of_equal_keys(V, n):
    rng = np.random.default_rng(n)
    layout, lay = self_layout(V)
    for kind in ("pos1", "pos1high", "pos2", "groups"):
        rec = ladder(kind, n, rng)
        # the first group of equal E-values of "groups" ends at its size
        boundary = int((rec["length"] == 35).sum()) if kind == "groups" \
            else n // 2
        for best in sorted({1, max(1, boundary - 1), max(1, boundary),
                            boundary + 1, max(1, n - 1), max(1, n), n + 1}):
            check(V, layout, lay, rec, best=best)
        check(V, layout, lay, rec)                       # filters only
    if n == SIZES[-1]:
        # the tile boundaries once more, sorted and with a filter
        rec = ladder("groups", n, rng)
        check(V, layout, lay, rec, best=2 * TILE + 3, sort="jd")
        check(V, layout, lay, rec, best=TILE, evalue=1e-3, sort="la")


def test_equal_but_for_the_strand(V):
    gq, start, lengths, total = ragged_batch(V, [80, 90])
    layout = V.sink_params(kind=SM.QUERY, totallength=10 ** 5, markpos=[],
                           querystart=start, querylength=lengths,
                           querytotallength=total, leastlength=10)
    lay = SM.Layout(SM.QUERY, 10 ** 5, 4, lengths, leastlength=10)
    d = np.zeros(40, H.MATCH_DTYPE)
    d["length"], d["dbstart"] = 20, np.arange(40) % 20
    d["queryseq"], d["querystart"] = np.arange(40) // 20, 7
    p = d.copy()             # the same place on the forward strand
    p["querystart"] = lengths[p["queryseq"].astype(np.int64)] - (
        d["querystart"] + d["length"])
    both = np.concatenate([d, p])
    bflags = np.repeat([0, 1], 40).astype(np.uint8)
    for best in (1, 2, 3, 39, 40, 41, 79, 80, 81):
        sel, ev, st = SM.select(lay, both, bflags, best=best)
        for lists in ([(d, False), (p, True)], [(p, True), (d, False)]):
            got, flags, gst = gpu_select(V, layout, lists, gq, best=best)
            assert np.array_equal(got, both[sel])
            assert np.array_equal(flags, bflags[sel])
            assert gst.selected == st["selected"]
    # direct before palindromic: the pairs alternate
    got, flags, _ = gpu_select(V, layout, [(p, True), (d, False)], gq,
                               best=80)
    assert list(flags[:6]) == [0, 1, 0, 1, 0, 1]


@pytest.mark.parametrize("n", [1, 65, 2 * TILE + 5])
def test_an_all_equal_list_is_one_match(V, n):
    layout, lay = self_layout(V)
    rec = self_records(33, np.full(n, 1 << 35, np.uint64), 1 << 36)
    for best in (1, 2, n + 1):
        got, flags, st = gpu_select(V, layout, [(rec, False)], best=best)
        assert np.array_equal(got, rec[:1])
        assert st.duplicates == n - 1 and st.selected == 1 and st.seen == n
    # many copies of a few keys, more copies than N: every round of the
    # select finds fewer distinct keys than it was asked for
    rec = self_records(33, np.arange(n, dtype=np.uint64) % np.uint64(5), 999)
    check(V, layout, lay, rec, best=5)
    check(V, layout, lay, rec, best=4, dupsdefined=False)
    check(V, layout, lay, rec, best=3, sort="id", dupsdefined=False)


def test_a_tie_on_a_word_costs_one_pass(V):
    """all keys agree on E-value, length1 and length2: one pass for each of
    these words, however many records tie; position1 (11 low bits differ) and
    position2 (one value) need no more than two each"""
    layout, lay = self_layout(V)
    n = 2 * TILE
    rec = self_records(30, np.random.default_rng(9).permutation(n).astype(
        np.uint64) + np.uint64(1 << 33), 1 << 36)
    sel = V.Select(layout, best=100)
    sel.add(V.Result.from_host(rec))
    assert 5 <= sel.passes <= 7
    want = rec[SM.select(lay, rec, None, best=100)[0]]
    assert np.array_equal(sel.finish().fetch(), want)
    # nothing to select from: no pass at all
    few = V.Select(layout, best=n + 1)
    few.add(V.Result.from_host(rec))
    assert few.passes == 0


def test_zero_evalues_among_tiny_ones(V):
    # totallength 2: the multiplier is 2.0, the E-value 2 T[0][length]; T
    # ends where it falls to 1e-300, near length 498 on four characters
    layout = V.sink_params(kind=SM.SELF, totallength=2, markpos=[],
                           leastlength=1)
    lay = SM.Layout(SM.SELF, 2, 4, leastlength=1)
    rng = np.random.default_rng(5)
    n = TILE + 77
    rec = self_records(rng.integers(470, 530, n), rng.permutation(n), 7)
    ev = np.array([SM.values(lay, x, 0).evalue for x in rec])
    assert (ev == 0.0).sum() > 100 and ((ev > 0) & (ev < 1e-290)).sum() > 100
    sel = V.Select(layout)
    assert np.array_equal(sel.evalues(V.Result.from_host(rec)), ev)
    nzero = int((ev == 0.0).sum())
    for opts in (dict(evalue=0.0), dict(evalue=0.0, best=nzero - 1),
                 dict(best=nzero - 1), dict(best=nzero), dict(best=nzero + 1),
                 dict(evalue=1e-299, best=n), dict(best=n, sort="ed")):
        check(V, layout, lay, rec, **opts)
    got, _, st = gpu_select(V, layout, [(rec, False)], evalue=0.0)
    assert len(got) == nzero and st.rejected == n - nzero


def test_noevalue(V):
    layout, lay = self_layout(V, showmode=V.SHOW_NOEVALUE)
    rng = np.random.default_rng(6)
    rec = ladder("groups", 700, rng)
    sel = V.Select(layout)
    assert not sel.evalues(V.Result.from_host(rec)).any()
    for opts in (dict(best=1), dict(best=44), dict(best=300, sort="ea"),
                 dict(evalue=0.0)):
        check(V, layout, lay, rec, **opts)


@pytest.mark.parametrize("best", [50, 1500, 5000])
def test_accumulation_over_several_lists(V, best):
    layout, lay = self_layout(V)
    rng = np.random.default_rng(7)
    rec = ladder("groups", 3 * TILE + 1, rng)
    rec["length"] += rng.integers(0, 3, len(rec)).astype(np.uint64)
    want = rec[SM.select(lay, rec, None, best=best)[0]]
    chunk = rec[100:400]
    for parts in (1, 2, 7):
        cuts = np.linspace(0, len(rec), parts + 1).astype(int)
        pieces = [rec[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        for order in (pieces, pieces[::-1]):
            lists = [(x, False) for x in order] + [(chunk, False)]
            got, _, st = gpu_select(V, layout, lists, best=best)
            assert np.array_equal(got, want), (parts, best)
            assert st.seen == len(rec) + len(chunk) and st.rejected == 0
            if best >= len(rec):
                # nothing was dropped as worse: every copy was compared
                assert st.duplicates == len(chunk)
            # a record that equals the worst of a full selection counts
            assert st.duplicates <= len(chunk)
    # the full selection meets its own records again: all duplicates
    sel = V.Select(layout, best=best)
    sel.add(V.Result.from_host(rec))
    sel.add(V.Result.from_host(want))
    assert np.array_equal(sel.finish().fetch(), want)
    assert sel.stats().duplicates == len(want)


def test_filters_alone_keep_the_order_across_workgroups(V):
    layout, lay = self_layout(V, leastlength=22)
    rng = np.random.default_rng(8)
    n = 3 * TILE + 1
    pos1 = rng.integers(0, 1 << 20, n).astype(np.uint64)
    length = rng.integers(18, 40, n).astype(np.uint64)
    # gaps from -length (the second instance starts at the first) upwards
    pos2 = pos1 + rng.integers(0, 120, n).astype(np.uint64)
    rec = self_records(length, pos1, pos2)
    for opts in (dict(), dict(gap=[10, 50]), dict(gap=[-5, 3]),
                 dict(gap=[-1000]), dict(gap=[0]), dict(evalue=1e-2),
                 dict(gap=[-5, 30], evalue=1e-3, best=700, sort="ia")):
        check(V, layout, lay, rec, **opts)
    sel, _, st = SM.select(lay, rec, None, gap=[-5, 3])
    assert 0 < len(sel) < n and st["rejected"] == n - len(sel)
    # two lists: the second behind the first
    got, _, _ = gpu_select(V, layout, [(rec[:TILE + 9], False),
                                       (rec[TILE + 9:], False)], gap=[-5, 3])
    assert np.array_equal(got, rec[sel])


def test_the_offset_of_a_batch_is_honoured(V):
    gq, start, lengths, total = ragged_batch(V, [50, 60, 70])
    gq.set_offset(1000)
    layout = V.sink_params(kind=SM.QUERY, totallength=10 ** 4, markpos=[],
                           leastlength=5)
    lay = SM.Layout(SM.QUERY, 10 ** 4, 4, lengths, leastlength=5,
                    seqoffset=1000)
    rec = np.zeros(30, H.MATCH_DTYPE)
    rec["length"] = 8 + np.arange(30) % 4
    rec["dbstart"] = np.arange(30) * 11 % 17
    rec["queryseq"] = 1000 + np.arange(30) % 3
    rec["querystart"] = np.arange(30)
    sel, _, _ = SM.select(lay, rec, None, best=12, sort="ja")
    got, _, _ = gpu_select(V, layout, [(rec, False)], gq, best=12, sort="ja")
    assert np.array_equal(got, rec[sel])
    bad = rec.copy()
    bad["queryseq"][3] = 999
    s = V.Select(layout, gq, best=12)
    with pytest.raises(V.VsaError) as e:
        s.add(V.Result.from_host(bad))
    assert e.value.code == -2
    assert s.stats().seen == 0 and s.finish().count == 0   # state untouched


def test_errors_and_composition(V):
    i, q = H.load_case("micro")
    gi = V.Index.from_tables(i.n, i.prefixlength, i.numofchars, i.tis, i.suf,
                             i.lcp, i.llv, i.bck, i.bwt, i.querysepposition,
                             i.hasqueries)
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    r = SC.run_of("micro", "q_l3")
    kw = SC.layout_kwargs("micro", r)
    with pytest.raises(V.VsaError) as e:
        V.Select(V.sink_params(**kw), gq, gap=[1, 5])
    assert e.value.code == -2 and "gap" in e.value.message
    with pytest.raises(V.VsaError) as e:
        V.Select(V.sink_params(**kw), gq, sort="la")
    assert e.value.code == -2 and "bestnumber" in e.value.message
    sel = V.Select(V.sink_params(**kw), gq, best=5)
    packed = V.findmumcandidates_packed(gi, gq, 3)
    with pytest.raises(V.VsaError) as e:
        sel.add(packed)
    assert e.value.code == V.NOT_COVERED
    mems = V.findquerymatches(gi, gq, 3)
    sp = V.Select(V.sink_params(selfpalindromic=True, palindromic=True, **kw),
                  gq, best=5)
    with pytest.raises(V.VsaError) as e:
        sp.add(mems, True)
    assert e.value.code == V.NOT_COVERED
    selfsel = V.Select(V.sink_params(**SC.layout_kwargs(
        "micro", SC.run_of("micro", "s_l2"))), best=5)
    with pytest.raises(V.VsaError) as e:
        selfsel.add(V.findmaximalrepeats(gi, 2), True)
    assert e.value.code == V.NOT_COVERED
    assert sel.stats().seen == 0 and sp.stats().seen == 0
    # the selected list is a result like any other: the coverage marks it
    sel.add(mems)
    best = sel.finish()
    assert best.count == 5
    cov, ref = V.Coverage.over_index(gi), V.Coverage.over_index(gi)
    cov.mark(best, V.COVERAGE_QUERY, V.COVERAGE_DATABASE)
    ref.mark(V.Result.from_host(best.fetch()), V.COVERAGE_QUERY,
             V.COVERAGE_DATABASE)
    assert cov.stats().marked == ref.stats().marked > 0
    assert np.array_equal(cov.bits(), ref.bits())

"""What the tests of the degenerate-match chain (test_gpu_degenerate_chain.py,
test_gpu_degenerate_forms.py) rest on and that needs no GPU: a separator
behind a read changes no list of a model, symbols behind it change no script;
the host entries give the models' lists on the padded batches, and these are
not vacuous; the packed form reads rows and side list; the cuts of the query
files leave matches on both sides; and the recorded order of the kinds
without an extension is the order of the oracle's enumeration."""
import numpy as np
import pytest

import align_cases as AC
import batch_forms as BF
import helpers as H


def host_entry(V, case, how, p, pal=False):
    sc = BF.scenario(case, how)
    if case[0] == "align":
        q = BF.forward_batch(case, how, pal)
        return V.align_host(sc.kind, sc.text, sc.records(),
                            (q.symbols, q.start, q.length), pal)
    q = sc.queries()
    kw = dict(queries=(q.symbols, q.start, q.length))
    if case[0] == "xdrop":
        kw["hamming"] = p[3]
    return getattr(V, "extend_%s_host" % case[0])(sc.text, sc.records(),
                                                  *p[:3], **kw)


def same(a, b):
    if isinstance(a, tuple):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


@pytest.mark.parametrize("case", BF.CASES, ids=BF.case_id)
def test_padded_scenarios_give_the_lists_of_the_unpadded_ones(V, case):
    align = case[0] == "align"
    sc = BF.scenario(case)
    assert len(sc.text) <= 4096 and 0 < len(sc.records()) <= 1024
    m = BF.common_length(BF.reads_of(sc))
    assert m % 4 != 0 and m % 32 != 0
    for how in (None, "sep", "plain"):
        padded = BF.scenario(case, how)
        assert np.array_equal(padded.records(), sc.records())
        if how is not None:
            assert all(len(r) == m for r in BF.reads_of(padded))
            # behind the read: what a record names stays where it is
            assert all(np.array_equal(a[:len(b)], b) for a, b in
                       zip(BF.reads_of(padded), BF.reads_of(sc)))
        some = far = 0
        for p in BF.params(case):
            want = BF.model(case, None, p)
            got = BF.model(case, how, p)
            if how != "plain" or align:
                assert same(got, want), (how, p)
            assert same(host_entry(V, case, how, p), got), (how, p)
            if align:
                assert len(got[1]) > 0
                for pal in ((True,) if BF.may_reverse(padded) else ()):
                    assert same(BF.model(case, how, p, pal), want)
                    assert same(host_entry(V, case, how, p, pal), want)
            else:
                some += len(got)
                far += int((BF.distances(case, p, got) > 0).sum())
        assert align or (some > 0 and far > 0)


def test_which_strands_and_what_the_packed_form_holds():
    reverse = {case for case in BF.CASES
               if BF.may_reverse(BF.scenario(case))}
    # a separator in a read: no reverse complement
    assert set(BF.CASES) - reverse == {("edist", "specials"),
                                       ("xdrop", "hspecials")}
    rows = 0
    for case in BF.CASES:
        assert not BF.may_reverse(BF.scenario(case, "sep")) or \
            case == ("xdrop", "hspecials")      # (of one length as it is)
        q = BF.scenario(case, "plain").queries()
        side = BF.in_side_list(q)
        assert 0 < side <= q.nq
        # every read of hspecials holds a special symbol
        assert side < q.nq or case == ("xdrop", "hspecials")
        rows += q.nq - side
    assert rows > 0


@pytest.mark.parametrize("case,mode", sorted(BF.PIECED))
def test_the_cuts_leave_matches_on_both_sides(case, mode):
    _, q = AC.load(case)
    a, b = BF.CUTS[case]
    assert 0 < a < b < len(q.length) and a % 64 and b % 64
    assert 1 in [last - first for first, last in BF.pieces(case)]
    have = BF.recorded_reads(case, mode)
    for first, last in BF.pieces(case):
        assert have & set(range(first, last))
    assert set(BF.beside_cuts(case)) <= have
    if case == "micro":
        # no other pair of neighbours with matches: with a batch of one read
        # wanted, "both sides of every cut" can hold for c6 only
        assert not any({i, i + 1} <= have for i in range(1, len(q.length)))
    # the reverse strand: the recorded -d -p runs hold no P row, so there
    # is no piece of which a palindromic record could be demanded
    skey = BF.PIECED[case, mode][2]
    if skey is not None:
        rows = AC.expected(skey, "rows")
        assert "p" not in AC.run_of(skey)["strands"] or \
            not (rows[:, 7] == 1).any()


@pytest.mark.parametrize("key", [r["key"] for r in AC.RUNS if r["kind"] in (
    AC.SELF, AC.QUERY, AC.COMPLETE, AC.APPROX_EDIST, AC.APPROX_HAMMING)])
def test_recorded_order_is_the_order_of_the_enumeration(key):
    """... which the device drivers are held to elsewhere: the chain may
    compare these kinds record by record, the repeat list included"""
    r = AC.run_of(key)
    db, q = AC.load(r["case"])
    idx = H.oracle_build_index(db.symbols, 4)
    hq = H.Queries(q.symbols, q.start, q.length) if r["q"] else None
    kind, a = r["kind"], r["args"]
    if kind == AC.SELF:
        got = H.oracle_repeats(idx, int(a[1]))
    elif kind == AC.QUERY:
        got = H.oracle_querymatches(idx, hq, int(a[1]), speedup=2)
    elif kind == AC.COMPLETE:
        got = H.oracle_complete(idx, hq)
    else:
        got = H.oracle_approx(idx, hq, kind == AC.APPROX_EDIST, int(a[2]))
    want = AC.records_of(r, AC.expected(key, "rows"))
    assert len(want) > 0 and np.array_equal(got, want)

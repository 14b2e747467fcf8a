"""vmatch -l L -h K | -e K [-s] as one chain on the GPU: the index built on the
device from the golden text, the device driver of the run's kind, and
vsa_align on THAT Result -- no host round trip between the links -- for every
recorded run of align_cases.RUNS, on 32-bit and on 64-bit tables; and the
same chain on a query file cut into batches with a sequence offset each.

Every kind compares in the recorded ORDER, the repeat list (vmatch -l L -s)
included: findmaximalrepeats delivers the order of the reference's
enumeration (test_gpu_parity.py asserts it against the oracle, and
test_batch_forms_host.py asserts the oracle's order against the recorded
rows), so no kind needs the multiset route."""
import numpy as np
import pytest

import align_cases as AC
import batch_forms as BF
import extend_cases as EC
import extend_edist_cases as DC
import helpers as H

pytestmark = pytest.mark.gpu

_index = {}


def built_index(V, monkeypatch, case, wide=False):
    """the index of a golden text, built on the GPU; wide: its tables
    uploaded again at 64 bits (the builder keeps 32 for a short text)"""
    monkeypatch.delenv("VSA_FORCE_WIDE", raising=False)
    if (case, False) not in _index:
        db, _ = AC.load(case)
        _index[case, False] = V.Index.build(db.symbols, 4, 0)
    gi = _index[case, False]
    if wide and (case, True) not in _index:
        db, _ = AC.load(case)
        i, t = gi.info(), gi.download()
        assert np.array_equal(t["tis"], db.symbols)
        monkeypatch.setenv("VSA_FORCE_WIDE", "1")
        try:
            _index[case, True] = V.Index.from_tables(
                i.totallength, i.prefixlength, 4, t["tis"],
                t["suf"].astype(np.uint64), t["lcp"],
                t["llv"].astype(np.uint64), t["bck"].astype(np.uint64),
                t["bwt"])
        finally:
            monkeypatch.delenv("VSA_FORCE_WIDE")
    gi = _index[case, wide]
    assert gi.info().device_integersize == (64 if wide else 32)
    return gi


def option(r, name):
    return int(r["args"][r["args"].index(name) + 1])


def drive(V, r, gi, gq, pal):
    """the device driver of a recorded run -> Result"""
    kind = r["kind"]
    if kind == AC.SELF_EDIST:
        return V.findselfmatches_edist(gi, option(r, "-l"), option(r, "-e"))
    if kind == AC.SELF_HAMMING:
        return V.findselfmatches_hamming(gi, option(r, "-l"), option(r, "-h"))
    if kind == AC.SELF:
        return V.findmaximalrepeats(gi, option(r, "-l"))
    if kind == AC.QUERY_EDIST:
        return V.findquerymatches_edist(gi, gq, option(r, "-l"),
                                        option(r, "-e"), palindromic=pal)
    if kind == AC.QUERY_HAMMING:
        return V.findquerymatches_hamming(gi, gq, option(r, "-l"),
                                          option(r, "-h"), palindromic=pal)
    assert not pal
    if kind == AC.QUERY:
        return V.findquerymatches(gi, gq, option(r, "-l"))
    if kind == AC.COMPLETE:
        return V.findcompletematches(gi, gq)
    doedist = kind == AC.APPROX_EDIST
    return V.findapproxcompletematches(gi, gq, doedist,
                                       option(r, "-e" if doedist else "-h"))


def same_records(got, want):
    """field by field, for the message; the self drivers write 0 into
    querystart (extend.hip, extend_edist_rules.h, selfmatch_search.inc), as
    records_of does"""
    assert len(got) == len(want)
    for f in ("length", "dbstart", "queryseq", "querystart"):
        assert np.array_equal(got[f], want[f]), f


def chain(V, monkeypatch, key, wide):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    r, e = AC.run_of(key), AC.manifest()[key]
    db, q = AC.load(r["case"])
    gi = built_index(V, monkeypatch, r["case"], wide)
    gq = V.Queries.from_host(q.symbols, q.start, q.length) if r["q"] else None
    qt = (q.symbols, q.start, q.length) if r["q"] else None
    want_off, want_words = AC.expected(key, "offsets"), AC.expected(key,
                                                                    "words")
    text, base, nwords = [], 0, 0
    for pal, rows in AC.passes(r, AC.expected(key, "rows")):
        res = drive(V, r, gi, gq, pal)
        al = V.align(gi, gq, res, r["kind"], pal)   # the driver's own Result
        rec = res.fetch()
        offsets, words = al.fetch()
        st = al.stats()
        assert st.count == len(rec) and st.words == len(words)
        # the order of the reference, for every kind (see the module's text)
        same_records(rec, AC.records_of(r, rows))
        host = V.align_host(r["kind"], db.symbols, rec, qt, pal)
        assert np.array_equal(offsets, host[0])
        assert np.array_equal(words, host[1])
        n = len(rec)
        assert np.array_equal(offsets + np.uint64(nwords),
                              want_off[base:base + n + 1])
        assert np.array_equal(words, want_words[nwords:nwords + len(words)])
        base, nwords = base + n, nwords + len(words)
        sink = V.Sink(**AC.sink_kwargs(V, r, pal))
        text.append(V.align_format(sink, rec, offsets, words, db.symbols,
                                   db.orig, qt, q.orig if r["q"] else None,
                                   r["width"]))
    assert base == len(AC.expected(key, "rows")) > 0
    assert nwords == e["words"]
    assert AC.md5(b"".join(text)) == e["md5"]


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("key", [r["key"] for r in AC.RUNS])
def test_recorded_runs_through_driver_and_align(V, monkeypatch, key, wide):
    chain(V, monkeypatch, key, wide)


# --------------------------------------------------------------------------
# a query file in three batches
# --------------------------------------------------------------------------

# (the cuts: batch_forms.CUTS; test_batch_forms_host.py checks on the
# recorded rows that they leave matches where this test wants them)

def piece_of(q, first, last):
    return H.Queries.from_list(
        [q.symbols[int(q.start[i]):int(q.start[i] + q.length[i])]
         for i in range(first, last)])


@pytest.mark.parametrize("case,mode", sorted(BF.PIECED))
def test_a_query_file_in_three_batches(V, monkeypatch, case, mode):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    L, K, skey, ekey = BF.PIECED[case, mode]
    kind = AC.QUERY_EDIST if mode == "e" else AC.QUERY_HAMMING
    find = V.findquerymatches_edist if mode == "e" else \
        V.findquerymatches_hamming
    db, q = AC.load(case)
    gi = built_index(V, monkeypatch, case)
    r = dict(case=case, kind=kind, q=True)
    for pal in (0, 1):
        def run(hq, first):
            gq = V.Queries.from_host(hq.symbols, hq.start, hq.length)
            if first is not None:
                gq.set_offset(first)
            res = find(gi, gq, L, K, palindromic=pal)
            al = V.align(gi, gq, res, kind, pal)
            return (res.fetch(),) + al.fetch()

        whole = run(q, None)
        if skey is not None and not pal:
            rows = dict(AC.passes(AC.run_of(skey), AC.expected(skey,
                                                               "rows")))[0]
            same_records(whole[0], AC.records_of(AC.run_of(skey), rows))
        sink = V.Sink(**AC.sink_kwargs(V, r, pal))
        recs, offs, words, lines, nwords = [], [np.zeros(1, np.uint64)], [], \
            [], 0
        for first, last in BF.pieces(case):
            rec, off, w = run(piece_of(q, first, last), first)
            # every piece yields records on the direct strand.  The reverse
            # strand has nothing to ask for: the recorded -d -p runs of c6
            # hold no P row (test_batch_forms_host.py asserts it), and a
            # batch of one read need not have a palindromic match at all;
            # there the pieces only have to add up to the single batch
            assert len(rec) > 0 or pal
            if len(rec):
                assert first <= int(rec["queryseq"].min()) and \
                    int(rec["queryseq"].max()) < last
            recs.append(rec)
            offs.append(off[1:] + np.uint64(nwords))
            words.append(w)
            nwords += len(w)
            # a Sink over the whole query file names the global number
            lines.append(sink.format(rec))
        assert np.array_equal(np.concatenate(recs), whole[0])
        assert np.array_equal(np.concatenate(offs), whole[1])
        assert np.array_equal(np.concatenate(words), whole[2])
        assert b"".join(lines) == sink.format(whole[0])
        if not pal:
            # the last read of a piece and the first of the next have matches
            assert set(BF.beside_cuts(case)) <= \
                set(whole[0]["queryseq"].tolist())
        if ekey is not None and not pal:
            # ... which is the line of the recorded run of the extension
            mod = DC if mode == "e" else EC
            golden = V.Sink(**mod.sink_kwargs(V, mod.run_of(ekey), 0))
            assert mod.md5(b"".join(golden.format(x) for x in recs)) == \
                mod.manifest()[ekey]["md5_lines"]

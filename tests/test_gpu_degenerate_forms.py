"""Every form of a query batch through vsa_extend_hamming, vsa_extend_edist,
vsa_extend_xdrop (both modes) and vsa_align: the hand-made scenarios of the
four case modules as a ragged byte batch (the scenario as it is), and with
their reads padded to one length (batch_forms.py) as a uniform byte batch
with separators, as reads at two bits per symbol with a side list, and as
dense device memory; each without and with a sequence offset, direct and
palindromic, align also on 64-bit tables.  Expected: the list of the model
and of the host entry.  Then the borders of the offset: the sequence numbers
just outside [offset, offset + nq) are refused by all four entries, the ones
just inside taken, and an offset that ends at 2^48 is taken, too."""
import numpy as np
import pytest

import batch_forms as BF
import helpers as H

pytestmark = pytest.mark.gpu

_index = {}
_host = {}


def index_of(V, monkeypatch, case, wide=False):
    k = (case, wide)
    if k not in _index:
        i = H.oracle_build_index(BF.scenario(case).text, 4)
        if wide:
            i = i.as_width(64)
            monkeypatch.setenv("VSA_FORCE_WIDE", "1")
        try:
            _index[k] = V.Index.from_tables(
                i.n, i.prefixlength, i.numofchars, i.tis, i.suf, i.lcp, i.llv,
                i.bck, i.bwt, i.querysepposition, i.hasqueries)
        finally:
            if wide:
                monkeypatch.delenv("VSA_FORCE_WIDE")
    assert _index[k].info().device_integersize == (64 if wide else 32)
    return _index[k]


def triple(q):
    return q.symbols, q.start, q.length


def run_entry(V, case, p, gi, gq, res, pal):
    """the device entry of a case on the list `res` -> (what it delivers,
    its statistics)"""
    entry = case[0]
    if entry == "align":
        al = V.align(gi, gq, res, BF.scenario(case).kind, pal)
        return al.fetch(), al.stats()
    if entry == "xdrop":
        L, X, S, hamming = p
        out = V.extend_xdrop(gi, gq, res, L, X, S, palindromic=pal,
                             hamming=hamming)
    else:
        L, K, S = p
        out = (V.extend_hamming if entry == "hamming" else V.extend_edist)(
            gi, gq, res, L, K, S, palindromic=pal)
    return out.fetch(), out.stats()


def host_entry(V, case, how, p, rec, pal=False):
    """the host entry of a case on the records `rec` of the scenario with
    its reads padded by `how`"""
    entry, sc = case[0], BF.scenario(case, how)
    if entry == "align":
        return V.align_host(sc.kind, sc.text, rec,
                            triple(BF.forward_batch(case, how, pal)), pal)
    qt = triple(sc.queries())
    if entry == "xdrop":
        L, X, S, hamming = p
        return V.extend_xdrop_host(sc.text, rec, L, X, S, queries=qt,
                                   hamming=hamming)
    L, K, S = p
    return (V.extend_hamming_host if entry == "hamming" else
            V.extend_edist_host)(sc.text, rec, L, K, S, queries=qt)


def same(case, got, want, k=0):
    if case[0] == "align":
        return np.array_equal(got[0], want[0]) and \
            np.array_equal(got[1], want[1])
    return np.array_equal(got, BF.shifted(want, k))


def strands(case):
    return ("direct", "palindromic") if BF.may_reverse(BF.scenario(case)) \
        else ("direct",)


def combinations(entries, widths=(False,)):
    return [pytest.param(case, form, strand == "palindromic", wide,
                         id="%s-%s-%s-%s" % (BF.case_id(case), form, strand,
                                             "wide" if wide else "narrow"))
            for case in BF.CASES if case[0] in entries
            for form in BF.FORMS for strand in strands(case)
            for wide in widths]


def check_forms(V, monkeypatch, case, form, pal, wide):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    monkeypatch.delenv("VSA_EXTEND_EDIST_SCRATCH", raising=False)
    monkeypatch.delenv("VSA_EXTEND_XDROP_BAND", raising=False)
    gi = index_of(V, monkeypatch, case, wide)
    align = case[0] == "align"
    rec = BF.scenario(case).records()
    assert len(BF.scenario(case).text) <= 4096 and 0 < len(rec) <= 1024
    staged = 0
    for how in BF.pads(form, pal):
        q = BF.forward_batch(case, how, pal)
        if form == "packed" and how == "plain":
            # rows and side list are both read (every read of hspecials
            # holds a special symbol: the side list alone)
            assert 0 < BF.in_side_list(q) <= q.nq
            assert BF.in_side_list(q) < q.nq or case == ("xdrop", "hspecials")
        some = far = 0
        for k in BF.OFFSETS:
            gq = BF.device_batch(V, q, form, k)
            res = V.Result.from_host(BF.shifted(rec, k))
            for p in BF.params(case):
                # a separator behind a read changes no list: the model of the
                # scenario as it is; symbols behind it: the model of that batch
                want = BF.model(case, how if how == "plain" or align else None,
                                p, pal)
                if (case, how, p, pal) not in _host:
                    _host[case, how, p, pal] = host_entry(V, case, how, p,
                                                          rec, pal)
                assert same(case, _host[case, how, p, pal], want), (how, p)
                if align:
                    assert same(case, want, BF.model(case, None, p))
                else:
                    some += len(want)
                    far += int((BF.distances(case, p, want) > 0).sum())
                for stage in ("long", None):
                    if stage is None:
                        monkeypatch.delenv("VSA_EXTEND_STAGE")
                    else:
                        monkeypatch.setenv("VSA_EXTEND_STAGE", stage)
                    got, st = run_entry(V, case, p, gi, gq, res, pal)
                    assert same(case, got, want, k), (how, k, p, stage)
                    if align:
                        assert st.count == len(rec) and st.edist > 0
                        assert st.words == len(want[1]) > 0
                        staged += st.staged if stage else 0
                    else:
                        assert st.candidates == len(rec)
                        assert st.count == len(want)
                        staged += st.searches if stage else 0
        assert align or (some > 0 and far > 0)
    assert staged > 0


@pytest.mark.parametrize("case,form,pal,wide",
                         combinations(("hamming", "edist", "xdrop")))
def test_extension_on_every_batch_form(V, monkeypatch, case, form, pal, wide):
    check_forms(V, monkeypatch, case, form, pal, wide)


@pytest.mark.parametrize("case,form,pal,wide",
                         combinations(("align",), (False, True)))
def test_alignment_on_every_batch_form(V, monkeypatch, case, form, pal, wide):
    check_forms(V, monkeypatch, case, form, pal, wide)


# --------------------------------------------------------------------------
# the borders of the offset
# --------------------------------------------------------------------------

BORDER_CASES = [("hamming", "borders_dense"), ("edist", "borders_dense"),
                ("xdrop", "borders_dense"), ("align", "distance8")]


@pytest.mark.parametrize("case", BORDER_CASES, ids=BF.case_id)
def test_sequence_numbers_at_the_borders_of_the_offset(V, monkeypatch, case):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    gi = index_of(V, monkeypatch, case)
    q, p = BF.scenario(case).queries(), BF.params(case)[0]
    nq = q.nq
    # the records of the first and of the last read: both reads come back
    ends = BF.border_records(case)
    want = host_entry(V, case, None, p, ends)
    if case[0] != "align":
        assert {0, nq - 1} == set(want["queryseq"].tolist())
    # 2^48: only the packed pairs of -mum count the bits of a sequence
    # number (recordform in esa_search.hip); the records of these entries
    # have 64 bits for it, so such an offset is an offset like any other
    for k in (7, (1 << 48) - nq, 1 << 48):
        gq = BF.device_batch(V, q, "ragged", k)
        # offset and offset + nq - 1 are taken
        res = V.Result.from_host(BF.shifted(ends, k))
        got, st = run_entry(V, case, p, gi, gq, res, False)
        assert same(case, got, want, k), k
        assert (st.count == len(ends)) if case[0] == "align" else \
            (st.candidates == len(ends) and st.count == len(want))
        # offset - 1 and offset + nq are read by no kernel
        for seqnum in (k - 1, k + nq):
            wrong = BF.shifted(ends, k)
            wrong["queryseq"][-1] = seqnum
            bad = V.Result.from_host(wrong)
            before = V.device_meminfo()
            with pytest.raises(V.VsaError) as e:
                run_entry(V, case, p, gi, gq, bad, False)
            assert e.value.code == -2, e.value.message
            assert "1 %s do not fit" % ("records" if case[0] == "align"
                                        else "seeds") in e.value.message
            assert V.device_meminfo() == before
            bad.close()


@pytest.mark.parametrize("case", BORDER_CASES, ids=BF.case_id)
def test_a_packed_batch_of_no_reads(V, monkeypatch, case):
    """flatten_batch refuses a ragged batch without a host copy of its
    lengths.  Every constructor of a ragged batch keeps them (from_host, the
    reverse complement, the translated batches) and a uniform batch needs
    none; what is left is the packed batch of no reads, which counts as
    ragged and keeps one length.  An empty list on it is taken, a record is
    refused by every entry, and nothing stays behind."""
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    gi = index_of(V, monkeypatch, case)
    rec, p = BF.scenario(case).records(), BF.params(case)[0]
    gq = V.Queries.from_host_packed(np.zeros(0, np.uint8), 29)
    assert gq.nq == 0 and gq.info().numofsymbols == 0
    got, st = run_entry(V, case, p, gi, gq, V.Result.from_host(rec[:0]),
                        False)
    assert st.count == 0 and len(got[0] if case[0] == "align" else got) == \
        (1 if case[0] == "align" else 0)
    one = V.Result.from_host(rec[:1])
    # The entries return an empty list before they ask for the bytes of the
    # batch (extend_shared.hpp: seeds->count == 0; align.hip: n == 0), so
    # the call above has not made them.  The first refused call does
    # (vsa_queries_bytes), and they stay with the batch, which is alive:
    # memory is compared over the second refusal, where nothing is made.
    for kept in (False, True):
        before = V.device_meminfo()
        with pytest.raises(V.VsaError) as e:
            run_entry(V, case, p, gi, gq, one, False)
        assert e.value.code == -2
        assert ("1 seeds do not fit" if case[0] == "hamming" else
                "no host copy of its lengths") in e.value.message
        assert not kept or V.device_meminfo() == before

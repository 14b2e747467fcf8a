"""vmatch -s on the GPU: vsa_align on the records of every recorded run of the
real reference == vsa_align_host == the recorded scripts, and the text
formatted from the device's scripts has the recorded md5 (no reference program
in the loop); the match lists made by hand (align_cases.py) against
vsa_align_host and the literal Python model, with the slides left to the
budget and forced to one form; and what the device entry refuses."""
import os

import numpy as np
import pytest

import align_cases as AC
import helpers as H

pytestmark = pytest.mark.gpu

_index = {}


def index_of(V, name, text):
    """an index over `text`, made once per text"""
    if name not in _index:
        i = H.oracle_build_index(np.ascontiguousarray(text, np.uint8), 4)
        _index[name] = V.Index.from_tables(
            i.n, i.prefixlength, i.numofchars, i.tis, i.suf, i.lcp, i.llv,
            i.bck, i.bwt, i.querysepposition, i.hasqueries)
    return _index[name]


def batch(V, q):
    return None if q is None else V.Queries.from_host(q.symbols, q.start,
                                                      q.length)


@pytest.mark.parametrize("key", [r["key"] for r in AC.RUNS])
def test_recorded_runs(V, monkeypatch, key):
    monkeypatch.delenv("VSA_EXTEND_STAGE", raising=False)
    r, e = AC.run_of(key), AC.manifest()[key]
    db, q = AC.load(r["case"])
    gi = index_of(V, r["case"], db.symbols)
    gq = batch(V, q) if r["q"] else None
    qt = (q.symbols, q.start, q.length) if r["q"] else None
    text, base, nwords = [], 0, 0
    want_off, want_words = AC.expected(key, "offsets"), AC.expected(key,
                                                                    "words")
    for pal, rows in AC.passes(r, AC.expected(key, "rows")):
        rec = AC.records_of(r, rows)
        al = V.align(gi, gq, V.Result.from_host(rec), r["kind"], pal)
        offsets, words = al.fetch()
        st = al.stats()
        assert st.count == len(rec) and st.words == len(words)
        assert st.total_device_ms > 0
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
    assert nwords == e["words"]
    assert AC.md5(b"".join(text)) == e["md5"]


def check(V, sc, stages=(None,), rec=None):
    """vsa_align on the list of a scenario == vsa_align_host == the model"""
    rec = sc.records() if rec is None else rec
    gi = index_of(V, "planted " + sc.name, sc.text)
    gq = batch(V, sc.queries())
    host = V.align_host(sc.kind, sc.text, rec, sc.triple(), sc.palindromic)
    want = sc.model(rec)
    assert np.array_equal(host[0], want[0])
    assert np.array_equal(host[1], want[1])
    stats = {}
    for stage in stages:
        if stage is None:
            os.environ.pop("VSA_EXTEND_STAGE", None)
        else:
            os.environ["VSA_EXTEND_STAGE"] = stage
        try:
            al = V.align(gi, gq, V.Result.from_host(rec), sc.kind,
                         sc.palindromic)
        finally:
            os.environ.pop("VSA_EXTEND_STAGE", None)
        got = al.fetch()
        assert np.array_equal(got[0], want[0]), (sc.name, stage)
        assert np.array_equal(got[1], want[1]), (sc.name, stage)
        stats[stage] = al.stats()
        assert stats[stage].count == len(rec)
    return stats


@pytest.mark.parametrize("D", AC.DISTANCES)
def test_every_group_width_and_the_last_bit_pair(V, D):
    """stored distances 1, 7 | 8, 15 | 16, 31: groups of 16, 32 and 64 lanes;
    the end diagonal on the outermost lanes; indels in the first and the last
    column; a distance stored above the real one; matches at both ends of the
    text; wildcards"""
    sc = AC.planted_distance(D)
    assert len(sc.text) <= 1400
    st = check(V, sc, ("lane", "long", None))
    assert st["lane"].staged == 0 and st["long"].staged > 0
    assert st[None].edist == len(sc.recs)


def test_palindromic_query_lists(V):
    check(V, AC.planted_distance(8, True), ("long", None))
    # the pairs of the tandem text, read from another array: no shortcut
    check(V, AC.planted_tandem(AC.QUERY_EDIST))


def test_overlapping_self_matches_take_the_same_text_shortcut(V):
    check(V, AC.planted_tandem(), ("lane", "long", None))


def test_backward_slide_that_passes_the_forward_one(V):
    check(V, AC.planted_overshoot(), ("long", None))


def test_a_run_of_more_than_16383_symbols(V):
    """... which is also a slide over the lane budget: the group stage"""
    sc = AC.planted_longrun()
    st = check(V, sc, (None, "lane", "long"))
    assert st[None].staged == len(sc.recs) and st["lane"].staged == 0


@pytest.mark.parametrize("kind", (AC.QUERY_HAMMING, AC.QUERY, AC.QUERY_EDIST))
def test_records_of_distance_zero_and_mismatches_in_one_list(V, kind):
    sc = AC.planted_mixed(kind)
    st = check(V, sc)[None]
    if kind != AC.QUERY_EDIST:
        assert st.edist == 0
    else:
        assert 0 < st.edist < len(sc.recs)


@pytest.mark.parametrize("count", (0, 1, 63, 64, 65))
def test_lists_around_a_wavefront_of_groups(V, count):
    """groups of 16 lanes: four to a wavefront, sixteen to a workgroup"""
    sc = AC.planted_mixed(AC.QUERY_EDIST, 65)
    st = check(V, sc, rec=sc.records()[:count])[None]
    assert st.count == count
    if count == 0:
        assert st.words == 0


def test_what_is_refused_leaves_no_handle(V):
    sc = AC.planted_distance(7)
    gi = index_of(V, "planted " + sc.name, sc.text)
    gq, rec = batch(V, sc.queries()), sc.records()
    res = V.Result.from_host(rec)
    V.align(gi, gq, res, sc.kind).close()
    before = V.device_meminfo()

    def refused(call, code):
        with pytest.raises(V.VsaError) as e:
            call()
        assert e.value.code == code, e.value.message
        assert V.device_meminfo() == before

    # a stored distance above 31 (the host takes it)
    far = rec[:1].copy()
    far["length"][0] = (int(far["length"][0]) & ~(0xFF << 48)) | 32 << 48
    bad = V.Result.from_host(far)
    before = V.device_meminfo()
    refused(lambda: V.align(gi, gq, bad, sc.kind), V.NOT_COVERED)
    host = V.align_host(sc.kind, sc.text, far, sc.triple())
    assert np.array_equal(host[1], sc.model(far)[1])
    bad.close()
    before = V.device_meminfo()
    # the X-drop and the translated kinds, a selfpalindromic layout
    for kind in (12, 13, 14, 15, 5, 6):
        refused(lambda: V.align(gi, gq, res, kind), V.NOT_COVERED)
    p = V.SinkParams()
    p.kind, p.selfpalindromic = sc.kind, 1
    h = V.C.c_void_p()
    assert V.lib.vsa_align(gi._h, gq._h, res._h, V.C.byref(p), 1,
                           V.C.byref(h)) == V.NOT_COVERED and not h.value
    assert V.device_meminfo() == before
    # a self kind takes no batch, a query kind needs one
    refused(lambda: V.align(gi, gq, res, AC.SELF_EDIST), -2)
    refused(lambda: V.align(gi, None, res, sc.kind), -2)
    # a packed-pair result has no records
    c1, cq = H.load_case("c1")
    ci = V.Index.from_tables(c1.n, c1.prefixlength, c1.numofchars, c1.tis,
                             c1.suf, c1.lcp, c1.llv, c1.bck, c1.bwt,
                             c1.querysepposition, c1.hasqueries)
    cgq = V.Queries.from_host(cq.symbols, cq.start, cq.length)
    packed = V.findmumcandidates_packed(ci, cgq, 20)
    assert packed.count > 0 and packed.packbits
    before = V.device_meminfo()
    refused(lambda: V.align(ci, cgq, packed, AC.QUERY), V.NOT_COVERED)
    # a record that does not fit its texts is read by no kernel
    for field, value in (("dbstart", len(sc.text) - 3),
                         ("queryseq", len(sc.reads)), ("querystart", 1 << 33),
                         ("length", 0), ("length", 5 | 7 << 48)):
        wrong = rec.copy()
        wrong[field][2] = value
        badres = V.Result.from_host(wrong)
        before = V.device_meminfo()
        with pytest.raises(V.VsaError) as e:
            V.align(gi, gq, badres, sc.kind)
        assert e.value.code == -2 and "1 records do not fit" in e.value.message
        assert V.device_meminfo() == before
        badres.close()
    # a distance below the real one is the reference's error
    low = rec.copy()
    low["length"][0] = (int(low["length"][0]) & ~(0xFF << 48)) | 3 << 48
    lowres = V.Result.from_host(low)
    before = V.device_meminfo()
    with pytest.raises(V.VsaError) as e:
        V.align(gi, gq, lowres, sc.kind)
    assert e.value.code == -2 and "of 1 records is above" in e.value.message
    assert V.device_meminfo() == before

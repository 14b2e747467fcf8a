"""Match coverage on the GPU (vsa_coverage_*): every recorded run of the real
reference through the engine's entry points, mark and extract; and the
kernels against the numpy model of tests/test_coverage_host.py on hand-made
lists -- bit edges, the cooperative path, contention, extraction across
workgroups, the forms of a query batch, the keep flags, accumulation and the
forms that are not covered."""
import hashlib

import numpy as np
import pytest

import helpers as H
import test_coverage_host as M

pytestmark = pytest.mark.gpu

_index = {}


def gpu_index(V, case, which="db"):
    if (case, which) not in _index:
        if which == "all":
            tis, ssp, dblen, ndb = M.all_text(case)
            i = H.oracle_build_index(tis, 4, None, ssp=ssp,
                                     querysepposition=dblen, hasqueries=True)
        else:
            i = H.load_case(case)[0]
        _index[(case, which)] = V.Index.from_tables(
            i.n, i.prefixlength, i.numofchars, i.tis, i.suf, i.lcp, i.llv,
            i.bck, i.bwt, i.querysepposition, i.hasqueries)
    return _index[(case, which)]


def marked_of(cov):
    """the device table as one bool per position"""
    w = cov.bits()
    return np.unpackbits(w.view(np.uint8), bitorder="little")[
        :cov.nbits].astype(bool)


def engine_results(V, case, e):
    """the match lists of a recorded run from the real entry points -> list
    of (Result, palindromic), and the batch the query table is made from"""
    gi = gpu_index(V, case, e["index"])
    q = H.load_case(case)[1]
    eng, L = e["engine"], e["L"]
    if eng == "repeats":
        return [(V.findmaximalrepeats(gi, L), False)], None
    if eng == "supermax":
        return [(V.findsupermaximalrepeats(gi, L), False)], None
    if eng == "tandem":
        return [(V.findtandems(gi, L), False)], None
    if eng == "selfmum":
        return [(V.findmaximaluniquematches(gi, L), False)], None
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    if eng == "complete":
        if e["approx"]:
            return [(V.findapproxcompletematches(gi, gq, e["approx"][0],
                                                 e["approx"][1]), False)], gq
        return [(V.findcompletematches(gi, gq), False)], gq
    out = []
    if "d" in e["strands"]:
        out.append((V.findquerymatches(gi, gq, L, mum=e["mum"]), False))
    if "p" in e["strands"]:
        rc = gq.reverse_complement()
        out.append((V.findquerymatches(gi, rc, L, mum=e["mum"]), True))
    return out, gq


@pytest.mark.parametrize("case,key", M.RUNS)
def test_golden_runs_through_the_engine(V, case, key):
    e = M.CM[case][key]
    name = "%s__%s" % (case, key)
    results, gq = engine_results(V, case, e)
    layout = M.run_layout(e)
    side = V.COVERAGE_DATABASE if e["side"] == "db" else V.COVERAGE_QUERIES
    if side == V.COVERAGE_QUERIES and layout == M.QUERY:
        cov = V.Coverage.over_queries(gq)
    else:
        cov = V.Coverage.over_index(gpu_index(V, case, e["index"]))
    t = M.new_table(case, e)
    assert cov.nbits == len(t.marked)
    assert np.array_equal(marked_of(cov), t.marked)     # the separators
    for r, pal in results:
        cov.mark(r, layout, side, palindromic=pal,
                 complete=e["engine"] == "complete", **M.run_flags(e))
    t.marked = marked_of(cov)
    M.check_run(case, key, t, V)       # the table itself against the fixture
    st = cov.stats()
    assert st.marked == t.count()
    assert st.positions == len(t.marked) - len(t.ssp)
    if e["mask"]:
        assert st.marked == e["masked"] and st.positions == e["positions"]
        return
    # ... and the extraction kernels
    first, length, posoffset = M.run_range(t, e)
    if e["index"] == "all":
        iv = cov.nomatch(e["minlength"],
                         part="database" if e["side"] == "db" else "queries")
    elif layout == M.SELF:
        iv = cov.nomatch(e["minlength"], part="database")
    else:
        iv = cov.nomatch(e["minlength"])
    assert np.array_equal(iv, M.model_nomatch(t, e["minlength"], first,
                                              length))
    assert np.array_equal(M.rows_as_printed(iv, e["absolute"], posoffset),
                          M.cexpected(name + "__intervals"))
    text = V.nomatch_format(iv, V.SHOW_ABSOLUTE if e["absolute"] else 0,
                            posoffset)
    assert hashlib.md5(text).hexdigest() == e["md5_lines"]


# --------------------------------------------------------------------------
# hand-made lists against the model
# --------------------------------------------------------------------------

def one_sequence(V, nbits):
    """a table of nbits positions without separators, and its model"""
    q = V.Queries.from_host(np.zeros(nbits, np.uint8), [0], [nbits])
    return V.Coverage.over_queries(q), M.Table(nbits, [])


def records(instances):
    """(position, length) pairs as query-layout records of query 0"""
    rec = np.zeros(len(instances), H.MATCH_DTYPE)
    for i, (p, l) in enumerate(instances):
        rec[i] = (l, 0, 0, p)
    return rec


def mark_both(V, cov, t, rec, **kw):
    kw.setdefault("layout", V.COVERAGE_QUERY)
    kw.setdefault("side", V.COVERAGE_QUERIES)
    cov.mark(V.Result.from_host(rec), **kw)
    M.model_mark(t, rec, kw.pop("layout"), kw.pop("side"), **kw)


@pytest.mark.parametrize("nbits", [1, 63, 64, 65, 127, 128, 129])
def test_bit_edges_of_small_tables(V, nbits):
    cand = [(0, 1), (63, 1), (64, 1), (0, 64), (64, 64), (30, 65), (63, 2),
            (max(0, nbits - 3), min(3, nbits)), (nbits - 1, 1)]
    fit = [(p, l) for p, l in cand if p + l <= nbits]
    lists = [[]] + [[x] for x in fit] + [fit, [(0, nbits)]]
    for inst in lists:
        cov, t = one_sequence(V, nbits)
        mark_both(V, cov, t, records(inst))
        assert np.array_equal(cov.bits(), t.words()), inst
        assert cov.stats().marked == t.count()
    # the last list covered everything: no unmarked run is left
    assert t.marked.all() and len(cov.nomatch(1)) == 0


def test_instances_around_the_cooperative_threshold(V):
    T = V.COVERAGE_COOP_THRESHOLD
    nbits = 4 * T + 77
    inst = [(3, T - 1), (T + 67, T), (2 * T + 190, T + 1),
            (nbits - (T + 5), T + 5)]
    for some in [[x] for x in inst] + [inst]:
        cov, t = one_sequence(V, nbits)
        mark_both(V, cov, t, records(some))
        assert np.array_equal(cov.bits(), t.words()), some
    # a repeat of 250 000 symbols next to short ones in the same wavefront
    cov, t = one_sequence(V, 300001)
    mark_both(V, cov, t, records([(1, 2), (17, 250000), (299990, 11),
                                  (270000, T), (64, 64)]))
    assert np.array_equal(cov.bits(), t.words())


def test_contention_on_the_same_words(V):
    T = V.COVERAGE_COOP_THRESHOLD
    three = [(10, 100), (60, 2 * T), (100, 30)]
    cov, t = one_sequence(V, 5000)
    mark_both(V, cov, t, records(three))
    many, _ = one_sequence(V, 5000)
    many.mark(V.Result.from_host(np.tile(records(three), 100000)),
              V.COVERAGE_QUERY, V.COVERAGE_QUERIES)
    assert np.array_equal(many.bits(), cov.bits())
    assert np.array_equal(many.bits(), t.words())


def test_extraction_across_workgroups(V):
    tile = V.COVERAGE_EXTRACT_TILE
    rng = np.random.default_rng(1)
    # four sequences, one of length 0 between two adjacent separators
    lengths = np.array([tile + 4465, 0, 2 * tile + 34454, tile - 1000 + 37],
                       np.uint64)
    start = np.concatenate(([0], np.cumsum(lengths + np.uint64(1))[:-1]))
    nsym = int(lengths.sum()) + 3
    q = V.Queries.from_host(np.zeros(nsym, np.uint8), start, lengths)
    cov = V.Coverage.over_queries(q)
    t = M.Table(nsym, M.query_ssp(q_host(lengths)))
    assert cov.nbits == nsym >= 4 * tile
    assert t.ssp[1] == t.ssp[0] + 1
    # marked blocks at random, then: one clear run longer than a workgroup's
    # span that crosses two of their boundaries (inside sequence 2), and clear
    # positions at both ends of the range looked at
    first, length = 5, nsym - 5 - 9
    want = np.zeros(nsym, bool)
    pos = 0
    while pos < nsym:
        a, b = int(rng.integers(1, 300)), int(rng.integers(1, 200))
        want[pos:pos + a] = True
        pos += a + b
    lo, hi = 2 * tile - 3000, 3 * tile + 2000
    assert t.ssp[1] < lo and hi < t.ssp[2]
    want[lo:hi] = False
    want[lo - 1] = want[hi] = True
    want[first - 2:first + 7] = False
    want[first + length - 4:first + length + 3] = False
    want[t.ssp] = False
    d = np.diff(np.concatenate(([0], want.astype(np.int8), [0])))
    s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    rec = np.zeros(len(s), H.MATCH_DTYPE)
    seq = np.searchsorted(t.ssp, s, side="left")
    # blocks are cut at the separators so that each lies in one sequence
    cut = [(a, min(b, int(t.ends[k]))) for a, b, k in zip(s, e, seq)]
    rec["length"] = [b - a for a, b in cut]
    rec["queryseq"] = seq
    rec["querystart"] = [a - int(t.starts[k]) for (a, b), k in zip(cut, seq)]
    mark_both(V, cov, t, rec)
    assert np.array_equal(cov.bits(), t.words())
    assert not t.marked[first] and not t.marked[first + length - 1]
    whole = M.model_nomatch(t, 1, first, length)
    assert whole["length"].max() == hi - lo > tile
    assert whole["start"][0] == first
    assert whole["start"][-1] + whole["length"][-1] == first + length
    r = int(np.median(whole["length"]))
    for minlength in (1, r, r + 1, hi - lo, hi - lo + 1):
        got = cov.nomatch(minlength, first, length)
        assert np.array_equal(got, M.model_nomatch(t, minlength, first,
                                                   length)), minlength
    assert len(cov.nomatch(hi - lo, first, length)) == 1
    assert len(cov.nomatch(hi - lo + 1, first, length)) == 0   # no run at all
    # ranges inside one word, inside one marked block, of length 0, the
    # whole table
    blk = int(s[5])
    assert len(cov.nomatch(1, blk, int(e[5]) - blk)) == 0
    for f, l in ((70, 30), (0, 0), (nsym, 0), (0, nsym), (63, 2), (64, 64),
                 (int(t.ssp[0]) - 3, 9)):
        assert np.array_equal(cov.nomatch(1, f, l),
                              M.model_nomatch(t, 1, f, l)), (f, l)
    assert cov.stats().marked == t.count()
    # everything covered: nothing to report anywhere
    mark_both(V, cov, t, np.array([(l, 0, i, 0) for i, l in
                                   enumerate(lengths)], H.MATCH_DTYPE))
    assert t.marked.all() and len(cov.nomatch(1)) == 0
    with pytest.raises(V.VsaError):
        cov.nomatch(0)
    with pytest.raises(V.VsaError):
        cov.nomatch(1, 10, nsym)


@pytest.mark.parametrize("nruns", [1023, 1024, 1025, 2049])
def test_run_compaction_at_tile_edges(V, nruns):
    """exactly nruns maximal clear runs, alternately 1 and 2 positions long
    with one marked position between two of them: the runs of at least
    minlength are compacted over tiles of SELECT_TILE = 1024 runs"""
    assert V.SELECT_TILE == 1024
    lengths = 1 + np.arange(nruns) % 2
    starts = np.concatenate(([0], np.cumsum(lengths + 1)[:-1]))
    nbits = int(starts[-1] + lengths[-1])
    assert nbits < 10000
    cov, t = one_sequence(V, nbits)
    mark_both(V, cov, t, records([(int(p) - 1, 1) for p in starts[1:]]))
    assert np.array_equal(cov.bits(), t.words())
    every = cov.nomatch(1)
    assert len(every) == nruns
    assert np.array_equal(every["start"], starts)
    assert np.array_equal(every["length"], lengths)
    assert np.array_equal(every, M.model_nomatch(t, 1))
    two = cov.nomatch(2)
    assert len(two) == nruns // 2 and (two["length"] == 2).all()
    assert np.array_equal(two["start"], starts[lengths == 2])
    assert np.array_equal(two, M.model_nomatch(t, 2))
    assert len(cov.nomatch(3)) == 0 == len(M.model_nomatch(t, 3))


def test_more_than_256_extraction_tiles(V):
    """the tile counts of one extraction are more than one workgroup scans in
    one step: clear runs in the first tile, across the edge between tiles
    255 and 256, in tile 256 and at the very end"""
    tile = V.COVERAGE_EXTRACT_TILE
    nbits = 257 * tile + 100
    clear = [(1000, 7), (256 * tile - 3, 7), (256 * tile + 5000, 5),
             (nbits - 6, 6)]
    cov, t = one_sequence(V, nbits)
    inst, pos = [], 0
    for p, l in clear:
        inst.append((pos, p - pos))
        pos = p + l
    assert pos == nbits
    mark_both(V, cov, t, records(inst))
    assert np.array_equal(cov.bits(), t.words())
    want = M.model_nomatch(t, 1)
    assert [(int(r["start"]), int(r["length"])) for r in want] == clear
    assert np.array_equal(cov.nomatch(1), want)
    first = 255 * tile + 777
    for length in (nbits - first, nbits - first - 2, tile + 5002 - 777):
        sub = M.model_nomatch(t, 1, first, length)
        assert len(sub) in (2, 3)
        assert np.array_equal(cov.nomatch(1, first, length), sub), length
    assert np.array_equal(cov.nomatch(6), M.model_nomatch(t, 6))


def q_host(lengths):
    lengths = np.asarray(lengths, np.uint64)
    start = np.concatenate(([0], np.cumsum(lengths + np.uint64(1))[:-1]))
    return H.Queries(np.zeros(int(lengths.sum()) + len(lengths), np.uint8),
                     start, lengths)


def test_the_forms_of_a_query_batch_give_the_same_table(V):
    rng = np.random.default_rng(2)
    nq, m = 700, 100
    reads = rng.integers(0, 4, nq * m).astype(np.uint8)
    reads[rng.integers(0, nq * m, 20)] = H.WILDCARD      # side list rows
    multiseq = np.full(nq * (m + 1), H.SEPARATOR, np.uint8)
    multiseq.reshape(nq, m + 1)[:, :m] = reads.reshape(nq, m)
    ar = np.arange(nq, dtype=np.uint64)
    forms = {
        "bytes": V.Queries.from_host(multiseq[:-1], ar * (m + 1),
                                     np.full(nq, m, np.uint64)),
        "dense": V.Queries.from_host(reads, ar * m, np.full(nq, m, np.uint64)),
        "packed": V.Queries.from_host_packed(reads, m),
    }
    rec = np.zeros(2000, H.MATCH_DTYPE)
    rec["queryseq"] = rng.integers(0, nq, len(rec))
    qs = rng.integers(0, m - 20, len(rec))
    rec["querystart"] = qs
    rec["length"] = 20 + rng.integers(0, m - 20 - qs + 1)
    t = M.Table(nq * (m + 1) - 1, M.query_ssp(q_host(np.full(nq, m))))
    M.model_mark(t, rec, M.QUERY, M.QUERIES)
    for name, q in forms.items():
        cov = V.Coverage.over_queries(q)
        cov.mark(V.Result.from_host(rec), V.COVERAGE_QUERY,
                 V.COVERAGE_QUERIES)
        assert np.array_equal(cov.bits(), t.words()), name
    # a batch numbered from k marks as if numbered from 0
    k = 123456789
    forms["packed"].set_offset(k)
    cov = V.Coverage.over_queries(forms["packed"])
    shifted = rec.copy()
    shifted["queryseq"] += np.uint64(k)
    cov.mark(V.Result.from_host(shifted), V.COVERAGE_QUERY,
             V.COVERAGE_QUERIES)
    assert np.array_equal(cov.bits(), t.words())


def test_reads_of_mixed_length_and_the_palindromic_flip(V):
    rng = np.random.default_rng(3)
    lengths = rng.integers(1, 400, 300).astype(np.uint64)
    lengths[[7, 8, 100]] = 0
    hq = q_host(lengths)
    q = V.Queries.from_host(hq.symbols[:-1], hq.start, hq.length)
    rec = np.zeros(1500, H.MATCH_DTYPE)
    rec["queryseq"] = rng.choice(np.flatnonzero(lengths > 0), len(rec))
    ql = lengths[rec["queryseq"]].astype(np.int64)
    ln = 1 + rng.integers(0, ql)
    rec["length"] = ln
    rec["querystart"] = rng.integers(0, ql - ln + 1)
    for pal in (False, True):
        cov = V.Coverage.over_queries(q)
        t = M.Table(int(lengths.sum()) + len(lengths) - 1, M.query_ssp(hq))
        assert np.array_equal(cov.bits(), t.words())
        mark_both(V, cov, t, rec, palindromic=pal)
        assert np.array_equal(cov.bits(), t.words()), pal
        assert np.array_equal(cov.nomatch(3), M.model_nomatch(t, 3))


def three_sequence_index(V, withqueries):
    rng = np.random.default_rng(4)
    tis = rng.integers(0, 4, 3000).astype(np.uint8)
    ssp = np.array([899, 2100])
    tis[ssp] = H.SEPARATOR
    gi = V.Index.build(tis, 4, 0, 0)
    if withqueries:
        gi.set_queryseparator(int(ssp[0]))
    return gi, tis, ssp


@pytest.mark.parametrize("withqueries", [False, True],
                         ids=["plain", "indexedqueries"])
def test_keep_flags_on_self_lists(V, withqueries):
    gi, tis, ssp = three_sequence_index(V, withqueries)
    rng = np.random.default_rng(5)
    n, nrec = len(tis), 400
    rec = np.zeros(nrec, H.MATCH_DTYPE)
    rec["length"] = rng.integers(1, 60, nrec)
    if withqueries:
        a = rng.integers(0, ssp[0] - 60, nrec)
        b = rng.integers(ssp[0] + 1, n - 60, nrec)
    else:
        a = rng.integers(0, n - 60, nrec)
        b = rng.integers(0, n - 60, nrec)
        a, b = np.minimum(a, b), np.maximum(a, b)
    # no instance starts on a separator
    a[np.isin(a, ssp)] += 1
    b[np.isin(b, ssp)] += 1
    rec["dbstart"], rec["queryseq"] = a, b
    res = V.Result.from_host(rec)
    sides = [V.COVERAGE_DATABASE] + ([V.COVERAGE_QUERIES] if withqueries
                                     else [])
    for side in sides:
        for combo in range(16):
            flags = dict(markleft=combo & 1, markright=combo >> 1 & 1,
                         markleftifdifferentsequence=combo >> 2 & 1,
                         markrightifdifferentsequence=combo >> 3 & 1)
            cov = V.Coverage.over_index(gi)
            t = (M.Table(n, ssp, int(ssp[0]), 1) if withqueries
                 else M.Table(n, ssp))
            assert np.array_equal(cov.bits(), t.words())
            cov.mark(res, V.COVERAGE_SELF, side, **flags)
            M.model_mark(t, rec, M.SELF, side, **flags)
            assert np.array_equal(cov.bits(), t.words()), (side, flags)
    if not withqueries:
        cov = V.Coverage.over_index(gi)
        with pytest.raises(V.VsaError) as err:
            cov.mark(res, V.COVERAGE_SELF, V.COVERAGE_QUERIES)
        assert err.value.message == ("option -qnomatch requires index "
                                     "containing query sequences or option -q")
        # the reference's scan of a self run leaves the last position out
        t = M.Table(n, ssp)
        assert np.array_equal(cov.nomatch(1, part="database"),
                              M.model_nomatch(t, 1, 0, n - 1))
        assert np.array_equal(cov.nomatch(1), M.model_nomatch(t, 1))


def test_accumulation_merge_and_counts(V):
    gi, tis, ssp = three_sequence_index(V, False)
    rng = np.random.default_rng(6)
    n = len(tis)

    def some(k):
        rec = np.zeros(k, H.MATCH_DTYPE)
        rec["length"] = rng.integers(1, 40, k)
        rec["dbstart"] = rng.integers(0, n - 40, k)
        return rec
    r1, r2 = some(30), some(25)
    both = V.Coverage.over_index(gi)
    both.mark(V.Result.from_host(np.concatenate([r1, r2])),
              V.COVERAGE_QUERY, V.COVERAGE_DATABASE)
    twice = V.Coverage.over_index(gi)
    a, b = V.Coverage.over_index(gi), V.Coverage.over_index(gi)
    for cov, rec in ((twice, r1), (twice, r2), (a, r1), (b, r2)):
        cov.mark(V.Result.from_host(rec), V.COVERAGE_QUERY,
                 V.COVERAGE_DATABASE)
    assert np.array_equal(twice.bits(), both.bits())
    assert not np.array_equal(a.bits(), both.bits())
    a.merge(b)
    assert np.array_equal(a.bits(), both.bits())
    t = M.Table(n, ssp)
    M.model_mark(t, np.concatenate([r1, r2]), M.QUERY, M.DATABASE)
    assert np.array_equal(both.bits(), t.words())
    st = both.stats()
    assert (st.positions, st.marked, st.separators) == (n - 2, t.count(), 2)
    assert 0 < st.marked < st.positions
    other = V.Coverage.over_queries(
        V.Queries.from_host(np.zeros(10, np.uint8), [0], [10]))
    with pytest.raises(V.VsaError):
        a.merge(other)


def test_forms_that_are_not_covered_leave_the_table_alone(V):
    gi = gpu_index(V, "micro")
    q = H.load_case("micro")[1]
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    dbcov, qcov = V.Coverage.over_index(gi), V.Coverage.over_queries(gq)
    db0, q0 = dbcov.bits(), qcov.bits()
    c1q = H.load_case("c1")[1]
    packed = V.findmumcandidates_packed(
        gpu_index(V, "c1"),
        V.Queries.from_host(c1q.symbols, c1q.start, c1q.length), 20)
    assert packed.count > 0 and packed.packbits
    mem = V.findquerymatches(gi, gq, 3)
    complete = V.findcompletematches(gi, gq)
    approx = V.findapproxcompletematches(gi, gq, 1, 1)
    for cov, r, kw in (
            (dbcov, packed, dict(side=V.COVERAGE_DATABASE)),
            (dbcov, mem, dict(side=V.COVERAGE_DATABASE, selfpalindromic=True)),
            (qcov, complete, dict(side=V.COVERAGE_QUERIES, complete=True)),
            (qcov, approx, dict(layout=V.COVERAGE_APPROX,
                                side=V.COVERAGE_QUERIES))):
        with pytest.raises(V.VsaError) as err:
            cov.mark(r, **kw)
        assert err.value.code == V.NOT_COVERED
    # the same-sequence keywords with -q: the reference's error
    with pytest.raises(V.VsaError) as err:
        dbcov.mark(mem, side=V.COVERAGE_DATABASE,
                   markleftifdifferentsequence=0)
    assert err.value.code == -2 and "keepleftifsamesequence" in \
        err.value.message
    # a table of the wrong Multiseq
    with pytest.raises(V.VsaError):
        qcov.mark(mem, side=V.COVERAGE_DATABASE)
    assert np.array_equal(dbcov.bits(), db0)
    assert np.array_equal(qcov.bits(), q0)
    # the database side of the same complete lists is covered
    dbcov.mark(complete, side=V.COVERAGE_DATABASE, complete=True)
    assert not np.array_equal(dbcov.bits(), db0)

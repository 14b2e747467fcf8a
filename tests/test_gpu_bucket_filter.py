"""The MUM filter inside the bucket sort (candidate_sort.inc: k_cs_filter):
every bucket is sorted and filtered in LDS by one workgroup that knows of the
buckets in front of it only what the scatter left in bcarry[] -- the largest
right end that reaches in.  The cases here are built around what can go wrong
there: a candidate covered from another bucket only (by one symbol more, by
exactly its right end, by one symbol less: not covered), a cover that spans
many buckets and a stretch of empty ones, a bucket whose staging region is
rewritten in place while almost full, a list of which nothing survives, and
the same call twice.

Every case gives the oracle's list under VSA_TUNE 0 (default choice), 4
(rocPRIM and the tiled filter) and 8 (buckets whatever the size), and asserts
on the candidate list and the oracle's list that the situation it was built
for occurred.  A random text of 300 kbp with some 40 k reads of 100 bp around
the constructed ones: more than VSA_CS_MINPAIRS candidates, so the default
takes the buckets, 37 of 2^13 positions (with 66 k reads: 74 of 2^12).
Constructed reads lie at multiples of 2^16, bucket boundaries for every shift
up to 16."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

N = 300_000
L = 20
M = 100
CAP = 4096              # VSA_CS_CAP
MINPAIRS = 1 << 14      # VSA_CS_MINPAIRS
B = 1 << 16
TUNES = (0, 4, 8)


def sort_counters(V):
    out = (C.c_uint64 * 5)()
    V.lib.vsa_debug_candidate_sort(out)
    return dict(zip(("runs", "overflows", "longruns", "shift", "buckets"),
                    [int(x) for x in out]))


@pytest.fixture(scope="module")
def text(V):
    tis = np.random.default_rng(1212).integers(0, 4, N).astype(np.uint8)
    gi = V.Index.build(tis, 4, 0)
    t = gi.download()
    pl = gi.info().prefixlength
    host = H.Index(N, pl, 4, t["tis"], t["suf"], t["lcp"], t["llv"],
                   t["bck"], t["bwt"], None)
    gi.close()
    return dict(tis=tis, tables=t, pl=pl, host=host, gpu={}, cases={})


def index_for(V, monkeypatch, text, tune):
    """the text's index created under VSA_TUNE=tune (the library reads the
    switches when an index is created)"""
    if tune not in text["gpu"]:
        monkeypatch.setenv("VSA_TUNE", str(tune))
        t = text["tables"]
        text["gpu"][tune] = V.Index.from_tables(
            N, text["pl"], 4, t["tis"], t["suf"], t["lcp"], t["llv"],
            t["bck"], t["bwt"])
    return text["gpu"][tune]


def background(tis, rng, nreads, windows, mutate=4):
    """nreads reads of M symbols from random places, every `mutate`-th with
    one substitution, none of them touching one of the windows [lo, hi)"""
    starts = rng.integers(0, N - M, 2 * nreads)
    ok = np.ones(len(starts), bool)
    for lo, hi in windows:
        ok &= (starts + M <= lo) | (starts >= hi)
    starts = starts[ok][:nreads]
    assert len(starts) == nreads
    reads = tis[starts[:, None] + np.arange(M)[None, :]].copy()
    hit = np.arange(0, nreads, mutate)
    col = rng.integers(0, M, len(hit))
    reads[hit, col] = (reads[hit, col] + rng.integers(1, 4, len(hit))) % 4
    return [r for r in reads.astype(np.uint8)]


def cut(tis, p, length, subst=()):
    r = tis[p:p + length].copy()
    for at in subst:
        r[at] = (r[at] + 1) % 4
    return r


def case(text, name, make):
    """(queries, the oracle's MUMs) of a case, made once for the three tunes"""
    if name not in text["cases"]:
        q = make()
        text["cases"][name] = (q, H.oracle_querymatches(
            text["host"], q, L, mum=True, speedup=0))
    return text["cases"][name]


def run(V, gi, q):
    """-> (MUMs, candidates, counters before and after the -mum call, the
    -mum call's statistics)"""
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    before = sort_counters(V)
    r = V.findquerymatches(gi, gq, L, mum=True)
    got = r.fetch()
    after = sort_counters(V)
    cand = V.findquerymatches(gi, gq, L, mum=True, cand=True).fetch()
    gq.close()
    return got, cand, before, after, r.stats()


def check_buckets(tune, stats, before, after, longruns=0):
    """the call went through the buckets unless VSA_TUNE=4, none gave up, and
    multiples of 2^16 are bucket boundaries"""
    assert stats.candidates >= MINPAIRS
    if tune == 4:
        assert after == before
        return None
    assert after["runs"] == before["runs"] + 1
    assert after["overflows"] == before["overflows"]
    assert after["longruns"] == before["longruns"] + longruns
    assert after["buckets"] > 1 and after["shift"] <= 16
    return after["shift"]


def find(m, dbstart, length):
    return m[(m["dbstart"] == dbstart) & (m["length"] == length)]


def right(m):
    return m["dbstart"] + m["length"] - np.uint64(1)


def coverers(cand, one):
    """the candidates in front of `one` that reach its right end or beyond"""
    return cand[(cand["dbstart"] < one["dbstart"]) & (right(cand) >=
                                                      right(one))]


SITES = ((1 * B, 100, True), (2 * B, 90, True), (3 * B, 89, False))


def one_boundary_reads(tis):
    """test_cover_across_one_boundary: (boundary X, length of the read cut at
    X - 50, does it cover the piece X+6 .. X+39) for SITES"""
    rng = np.random.default_rng(21)
    reads = background(tis, rng, 40_000,
                       [(x - 300, x + 300) for x, _, _ in SITES])
    for x, length, _ in SITES:
        reads.append(cut(tis, x - 50, length))
        reads.append(cut(tis, x, M, (5, 40)))
    order = rng.permutation(len(reads))
    return H.Queries.from_list([reads[i] for i in order])


@pytest.mark.parametrize("tune", TUNES)
def test_cover_across_one_boundary(V, text, monkeypatch, tune):
    """At three boundaries X a read of M symbols cut at X with substitutions
    at 5 and 40: its piece X+6 .. X+39 is the first candidate of the bucket
    that starts at X.  The only candidate in front that can cover it comes
    from the bucket before: a read cut at X-50 that ends at X+49 (covers), at
    X+39 (its very right end: covers) or at X+38 (one short: does not)."""
    q, want = case(text, "one-boundary",
                   lambda: one_boundary_reads(text["tis"]))
    got, cand, before, after, stats = run(V, index_for(V, monkeypatch, text,
                                                       tune), q)
    assert np.array_equal(got, want)
    shift = check_buckets(tune, stats, before, after)
    for x, length, covered in SITES:
        inner = find(cand, x + 6, 34)
        outer = find(cand, x - 50, length)
        assert len(inner) == 1 and len(outer) == 1
        assert int(right(outer)[0]) - int(right(inner)[0]) == length - 90
        # nothing but the read from the bucket before reaches so far
        over = coverers(cand, inner[0])
        assert len(over) == (1 if covered else 0)
        assert len(find(want, x + 6, 34)) == (0 if covered else 1)
        assert len(find(want, x - 50, length)) == 1
        if shift is not None:
            assert (x + 6) >> shift != (x - 50) >> shift
            assert ((x + 6) >> shift) << shift == x   # first of its bucket


@pytest.mark.parametrize("tune", TUNES)
def test_cover_across_many_buckets_and_an_empty_stretch(V, text, monkeypatch,
                                                        tune):
    """A read of 20 000 symbols cut at P covers five stretches of 2^12
    positions.  Short reads inside it, in the fifth, are all dropped -- the
    last of them ends with the long read's very last symbol --; those that
    end one symbol and more behind it, and the one that starts in front of it,
    are kept.  No other read touches [P + 2^12, P + 5 * 2^12): the buckets from
    P + 2^12 up to the short reads' are empty, three of them and more.

    A second read of 33 000 symbols elsewhere makes 16 length bits, and with
    66 000 reads query number and offset no longer fit into 32 bits: 8-byte
    values, so 16-byte staging entries, and shift < 16 = lenbits: a candidate
    reaches several later buckets in the scatter's loop."""
    tis = text["tis"]
    P, LONG, OTHER = 1 * B, 20_000, 3 * B
    lo, hi = P + 4096, P + 5 * 4096
    inside = (P + 4 * 4096 + 10, P + 4 * 4096 + 500, P + 4 * 4096 + 3000,
              P + LONG - M)
    outside = (P - 1, P + LONG - M + 1, P + LONG - 50)

    def make():
        rng = np.random.default_rng(22)
        reads = background(tis, rng, 66_000,
                           [(lo, hi), (P - 300, P + 300)])
        reads.append(cut(tis, P, LONG))
        reads.append(cut(tis, OTHER, 33_000, (700, 16_000, 16_040)))
        for p in inside + outside:
            reads.append(cut(tis, p, M))
        order = rng.permutation(len(reads))
        q = H.Queries.from_list([reads[i] for i in order])
        assert (q.nq << 16) >= (1 << 32)    # 8-byte values
        return q

    q, want = case(text, "many-buckets", make)
    got, cand, before, after, stats = run(V, index_for(V, monkeypatch, text,
                                                       tune), q)
    assert np.array_equal(got, want)
    shift = check_buckets(tune, stats, before, after)
    long_one = find(cand, P, LONG)
    assert len(long_one) == 1 and len(find(want, P, LONG)) == 1
    for p in inside:
        assert len(find(cand, p, M)) == 1 and len(find(want, p, M)) == 0
        over = coverers(cand, find(cand, p, M)[0])
        assert len(over) == 1 and over[0] == long_one[0]
    for p in outside:
        assert len(find(cand, p, M)) == 1 and len(find(want, p, M)) == 1
    assert int(right(find(cand, inside[-1], M))[0]) == P + LONG - 1
    if shift is not None:
        assert shift <= 12 < 16     # lo is a bucket boundary
        fill = np.bincount((cand["dbstart"] >> np.uint64(shift))
                           .astype(np.int64), minlength=after["buckets"])
        first, last = lo >> shift, inside[0] >> shift
        # at least three empty buckets between the coverer and the covered
        assert first > P >> shift
        assert last - first >= 3 and not fill[first:last].any()
        assert fill[P >> shift] > 0 and fill[last] > 0
        assert fill.max() <= CAP


@pytest.mark.parametrize("tune", TUNES)
def test_nearly_full_bucket(V, text, monkeypatch, tune):
    """3 300 reads spread evenly over the 8 192 positions of one bucket, every
    eighth with a substitution (its pieces are covered by its neighbours):
    the bucket holds more than 3 400 of VSA_CS_CAP = 4 096 pairs, about two
    per bin, and its survivors are written back over a staging region almost
    completely in use."""
    tis = text["tis"]
    X, W, NR = 2 * B, 1 << 13, 3300

    def make():
        rng = np.random.default_rng(23)
        reads = background(tis, rng, 40_000, [(X, X + W)])
        starts = X + (np.arange(NR) * W) // NR
        dense = tis[starts[:, None] + np.arange(M)[None, :]].copy()
        hit = np.arange(0, NR, 8)
        col = rng.integers(25, M - 25, len(hit))
        dense[hit, col] = (dense[hit, col] + 1) % 4
        reads += [r for r in dense.astype(np.uint8)]
        order = rng.permutation(len(reads))
        return H.Queries.from_list([reads[i] for i in order])

    q, want = case(text, "full-bucket", make)
    got, cand, before, after, stats = run(V, index_for(V, monkeypatch, text,
                                                       tune), q)
    assert np.array_equal(got, want)
    shift = check_buckets(tune, stats, before, after)
    inbucket = (cand["dbstart"] >= X) & (cand["dbstart"] < X + W)
    kept = (want["dbstart"] >= X) & (want["dbstart"] < X + W)
    assert 3400 < inbucket.sum() <= CAP
    assert 2500 < kept.sum() < inbucket.sum() - 400   # a real compaction
    if shift is not None:
        assert shift == 13      # [X, X + W) is one bucket
        fill = np.bincount((cand["dbstart"] >> np.uint64(shift))
                           .astype(np.int64))
        assert fill.argmax() == X >> shift and fill.max() == inbucket.sum()
        # (a bin: 2^(shift - 11) positions) no bin near 256
        assert np.bincount((cand["dbstart"][inbucket] - np.uint64(X))
                           .astype(np.int64) >> (shift - 11)).max() < 64


@pytest.mark.parametrize("tune", TUNES)
def test_nothing_survives(V, text, monkeypatch, tune):
    """every read twice: equal starts and equal lengths drop both copies"""
    tis = text["tis"]

    def make():
        rng = np.random.default_rng(24)
        once = background(tis, rng, 20_000, [], mutate=20_001)[1:]
        reads = once + once
        order = rng.permutation(len(reads))
        return H.Queries.from_list([reads[i] for i in order])

    q, want = case(text, "nothing", make)
    assert len(want) == 0
    got, cand, before, after, stats = run(V, index_for(V, monkeypatch, text,
                                                       tune), q)
    assert len(cand) >= MINPAIRS
    assert len(got) == 0 and np.array_equal(got, want)
    assert stats.count == 0 and stats.sumlength == 0
    check_buckets(tune, stats, before, after)
    assert after["overflows"] == before["overflows"]
    assert after["longruns"] == before["longruns"]


@pytest.mark.parametrize("tune", TUNES)
def test_same_call_twice(V, text, monkeypatch, tune):
    """the per-bucket words are zeroed for every call: a second call gives
    the same list and moves the counters as the first did"""
    q, want = case(text, "one-boundary",
                   lambda: one_boundary_reads(text["tis"]))
    gi = index_for(V, monkeypatch, text, tune)
    got1, _, before1, after1, stats1 = run(V, gi, q)
    got2, _, before2, after2, stats2 = run(V, gi, q)
    assert np.array_equal(got1, want) and np.array_equal(got2, got1)
    assert (stats1.count, stats1.sumlength, stats1.candidates) == (
        stats2.count, stats2.sumlength, stats2.candidates)
    assert stats1.count == len(want)
    assert stats1.sumlength == int(want["length"].sum())
    check_buckets(tune, stats1, before1, after1)
    check_buckets(tune, stats2, before2, after2)
    assert before2 == after1
    for k in ("overflows", "longruns", "shift", "buckets"):
        if tune != 4:
            assert after2[k] == after1[k]

"""The MUM filter (kurtz/cleanMUMcand.c:55-118) driven directly: synthetic
candidates, no index and no search, every sorter in front of the one tiled
filter -- packed keys, and wide records that fit no key and go through the
same tiles as sorted records -- sizes around its tile of 1024 candidates.
Expected: the CPU oracle.

The oracle itself was checked once, on the CPU, on every list used here (both
carries, the wide lists included) against a rendering of the rule in numpy --
sort by (dbstart, length descending), exclusive running maximum of the right
ends starting at the carry, keep a candidate iff that maximum is below its
right end and the next candidate does not have its dbstart and length --
and agreed record for record; test_oracle_is_the_rule keeps that check."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H

SIZES = (1, 2, 1023, 1024, 1025, 5000)
LENGTHBITS = 9
PLANTED = 200 + 150 + 91


@functools.lru_cache(maxsize=None)
def candidates(n, planted=True, dbbase=0, lenbase=0):
    """the synthetic list of the module's docstring: dbstarts from [0, n // 3)
    (runs of equal dbstarts are the rule), lengths from [20, 300); planted on
    top (lists that have the room): a dbstart with 200 members of distinct
    lengths, one with 150 of which the two longest are equal, one with 90 equal
    members and a single longer one -- placed so that in a list of 5000 each
    of them lies across a tile boundary; shuffled.  planted=False: every
    dbstart once."""
    rng = np.random.default_rng(21)
    planted = planted and n >= 1000
    nr = n - PLANTED if planted else n
    c = np.zeros(n, H.MATCH_DTYPE)
    if planted:
        c["dbstart"][:nr] = rng.integers(0, max(1, n // 3), nr)
    else:
        c["dbstart"][:nr] = rng.permutation(3 * n)[:n]
    c["length"][:nr] = rng.integers(20, 300, nr)
    if planted:
        # sorted, run k begins about 100 keys in front of tile boundary k
        order = np.sort(c["dbstart"][:nr])
        ranks = ((1024 - 100, 2048 - 275, 3072 - 395) if nr > 3072
                 else (nr // 4, nr // 2, 3 * nr // 4))
        spots = [int(order[r]) for r in ranks]
        assert len(set(spots)) == 3
        c["dbstart"][:nr][np.isin(c["dbstart"][:nr], spots)] += 1
        runs = (rng.permutation(np.arange(100, 300)),
                np.concatenate([np.arange(40, 189), [188]]),
                np.array([100] * 90 + [150]))
        at = nr
        for spot, lengths in zip(spots, runs):
            c["dbstart"][at:at + len(lengths)] = spot
            c["length"][at:at + len(lengths)] = lengths
            at += len(lengths)
        assert at == n
    c["dbstart"] += np.uint64(dbbase)
    c["length"] += np.uint64(lenbase)
    c["querystart"] = rng.integers(0, 500, n)
    c = c[rng.permutation(n)]
    c["queryseq"] = np.arange(n)
    c.setflags(write=False)
    return c


def carries(cand):
    return (0, int(np.median(cand["dbstart"] + cand["length"]
                             - np.uint64(1))))


@functools.lru_cache(maxsize=None)
def expected(n, planted, whichcarry, dbbase=0, lenbase=0):
    cand = candidates(n, planted, dbbase, lenbase)
    want = H.oracle_mumfilter(cand, carries(cand)[whichcarry])
    want.setflags(write=False)
    return want


def rule(cand, carry):
    """the filter's rule in numpy"""
    s = cand[np.lexsort((-cand["length"].astype(np.int64), cand["dbstart"]))]
    end = s["dbstart"] + s["length"] - np.uint64(1)
    before = np.maximum.accumulate(
        np.concatenate([[np.uint64(carry)], end[:-1]]))
    twin = np.zeros(len(s), bool)
    twin[:-1] = ((s["dbstart"][1:] == s["dbstart"][:-1]) &
                 (s["length"][1:] == s["length"][:-1]))
    return s[(before < end) & ~twin]


WIDE = dict(n=3000, planted=True, dbbase=1 << 40, lenbase=(1 << 30) - 20)
WIDES = [WIDE] + [dict(WIDE, n=n) for n in (5000, 1, 2, 1023, 1024, 1025)]
LISTS = ([dict(n=n, planted=True) for n in SIZES] +
         [dict(n=5000, planted=False)] + WIDES)


def test_lists_are_what_they_claim():
    for c in (candidates(5000), candidates(**WIDES[1])):
        d = np.sort(c["dbstart"])
        for b in (1024, 2048, 3072):
            assert d[b - 1] == d[b] and (d == d[b]).sum() >= 91
    assert np.unique(candidates(5000, False)["dbstart"]).size == 5000
    for kw in WIDES:
        w = candidates(**kw)
        assert len(w) == kw["n"]
        assert w["dbstart"].min() >= 1 << 40 and w["length"].min() >= 1 << 30
        assert w["length"].max() < (1 << 30) + 300


@pytest.mark.parametrize("which", range(len(LISTS)))
def test_oracle_is_the_rule(which):
    kw = LISTS[which]
    cand = candidates(**kw)
    for whichcarry, carry in enumerate(carries(cand)):
        want = expected(kw["n"], kw["planted"], whichcarry,
                        kw.get("dbbase", 0), kw.get("lenbase", 0))
        assert np.array_equal(want, rule(cand, carry)), (kw, carry)


def check(res, want, n):
    assert np.array_equal(res.fetch(), want)
    assert res.stats().sumlength == int(want["length"].sum())
    assert res.stats().candidates == n


GRID = [(n, whichcarry) for n in SIZES for whichcarry in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,whichcarry", GRID)
def test_records(V, n, whichcarry):
    """composite keys + index sorted on all bits, the sorted form of the
    filter, the survivors gathered from the records"""
    cand = candidates(n)
    dp = V.device_malloc(cand.nbytes)
    V.device_upload(dp, cand)
    try:
        check(V.mumuniqueinquery_range(dp, n, carries(cand)[whichcarry]),
              expected(n, True, whichcarry), n)
    finally:
        V.device_free(dp)


def pairs_case(V, cand, want, carry):
    n = len(cand)
    rows = np.zeros((n, 2), np.uint64)
    rows[:, 0] = ((cand["dbstart"] << np.uint64(LENGTHBITS)) |
                  (np.uint64(511) - cand["length"]))
    rows[:, 1] = (cand["queryseq"] << np.uint64(16)) | cand["querystart"]
    total = int(cand["dbstart"].max()) + 300
    dp = V.device_malloc(rows.nbytes)
    V.device_upload(dp, rows)
    try:
        check(V.mumuniqueinquery_range_packed(dp, n, LENGTHBITS, total,
                                              carry), want, n)
        cut = n // 3
        check(V.mumuniqueinquery_range_packed2(
            dp, cut, C.c_void_p(dp.value + 16 * cut), n - cut, LENGTHBITS,
            total, carry), want, n)
    finally:
        V.device_free(dp)


@pytest.mark.gpu
@pytest.mark.parametrize("n,whichcarry", GRID)
def test_pairs(V, n, whichcarry):
    """the same lists as (key, value) rows, in one place and in two: sorted
    on dbstart and filtered by runs; the planted runs of more than 64 make
    that the second attempt, sorted on all bits, across tile boundaries"""
    cand = candidates(n)
    pairs_case(V, cand, expected(n, True, whichcarry),
               carries(cand)[whichcarry])


@pytest.mark.gpu
@pytest.mark.parametrize("whichcarry", (0, 1))
def test_pairs_without_runs(V, whichcarry):
    """every dbstart once: the filter by runs answers alone"""
    cand = candidates(5000, False)
    pairs_case(V, cand, expected(5000, False, whichcarry),
               carries(cand)[whichcarry])


@pytest.mark.gpu
@pytest.mark.parametrize("whichcarry", (0, 1))
@pytest.mark.parametrize("which", range(len(WIDES)))
def test_wide_records(V, which, whichcarry):
    """dbstart of 41 bits and length of 31 do not fit into one key: two sorts
    of the records, the tiled filter on the sorted records (runs across tile
    boundaries in the list of 5000), which sums the lengths itself"""
    kw = WIDES[which]
    cand = candidates(**kw)
    n = len(cand)
    want = expected(n, True, whichcarry, kw["dbbase"], kw["lenbase"])
    dp = V.device_malloc(cand.nbytes)
    try:
        V.device_upload(dp, cand)
        check(V.mumuniqueinquery_range(dp, n, carries(cand)[whichcarry]),
              want, n)
        if whichcarry == 0:
            # (the filter sorts the caller's records in place: any order in)
            V.device_upload(dp, cand)
            check(V.mumuniqueinquery(dp, n), want, n)
    finally:
        V.device_free(dp)

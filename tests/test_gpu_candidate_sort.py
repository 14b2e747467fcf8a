"""The sort of the MUM candidates in front of the filter (candidate_sort.inc):
buckets by the high bits of dbstart, every bucket sorted in LDS, fed from the
kernels' own output; rocPRIM's radix sort behind compact() for short lists,
under VSA_TUNE=4 and when a bucket overflows.  The MUM list is a function of
the candidate set alone, so every case must give the oracle's list under
VSA_TUNE 0 (default choice), 4 (rocPRIM) and 8 (buckets whatever the size).

That a bucket sort ran, that one overflowed and went back to rocPRIM, and the
geometry of the last one are read from vsa_debug_candidate_sort, a counter
function of the library outside the ABI."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

N = 2_000_000
L = 20
M = 100
CAP = 4096              # VSA_CS_CAP
MINPAIRS = 1 << 14      # VSA_CS_MINPAIRS: shorter lists take rocPRIM by default
TUNES = (0, 4, 8)


def sort_counters(V):
    """-> dict(runs, overflows, longruns, shift, buckets)"""
    out = (C.c_uint64 * 5)()
    V.lib.vsa_debug_candidate_sort(out)
    return dict(zip(("runs", "overflows", "longruns", "shift", "buckets"),
                    [int(x) for x in out]))


@pytest.fixture(scope="module")
def text(V):
    """a random 2 Mbp text, its tables (built on the GPU) for the oracle"""
    tis = np.random.default_rng(2024).integers(0, 4, N).astype(np.uint8)
    gi = V.Index.build(tis, 4, 0)
    t = gi.download()
    pl = gi.info().prefixlength
    host = H.Index(N, pl, 4, t["tis"], t["suf"], t["lcp"], t["llv"],
                   t["bck"], t["bwt"], None)
    gi.close()
    return dict(tis=tis, tables=t, pl=pl, host=host, gpu={}, want={})


def index_for(V, monkeypatch, text, tune, wide=False, fresh=False):
    """the text's index created under VSA_TUNE=tune (the library reads the
    switches when an index is created); fresh: one of its own for a test that
    makes the index back off from the bucket sort"""
    key = (tune, wide, object() if fresh else None)
    if key not in text["gpu"]:
        monkeypatch.setenv("VSA_TUNE", str(tune))
        if wide:
            monkeypatch.setenv("VSA_FORCE_WIDE", "1")
        t = text["tables"]
        w = np.uint64 if wide else t["suf"].dtype
        gi = V.Index.from_tables(N, text["pl"], 4, t["tis"],
                                 t["suf"].astype(w), t["lcp"],
                                 t["llv"].astype(w), t["bck"].astype(w),
                                 t["bwt"])
        assert gi.info().device_integersize == (64 if wide else
                                                t["suf"].dtype.itemsize * 8)
        text["gpu"][key] = gi
    return text["gpu"][key]


def oracle(text, name, q):
    if name not in text["want"]:
        text["want"][name] = H.oracle_querymatches(text["host"], q, L,
                                                   mum=True, speedup=0)
    return text["want"][name]


def cut_reads(tis, starts, rng, mutate=4):
    """reads of M symbols from the given starts, every `mutate`-th with one
    substitution"""
    reads = tis[np.asarray(starts)[:, None] + np.arange(M)[None, :]].copy()
    hit = np.arange(0, len(reads), mutate)
    col = rng.integers(0, M, len(hit))
    reads[hit, col] = (reads[hit, col] + rng.integers(1, 4, len(hit))) % 4
    return reads.astype(np.uint8)


def many_reads(text):
    rng = np.random.default_rng(11)
    return cut_reads(text["tis"], rng.integers(0, N - M, 200_000), rng)


def by_buckets(tune, r):
    """does this call's list go through the bucket sort?"""
    return tune == 8 or (tune == 0 and r.stats().candidates >= MINPAIRS)


def check(V, gi, reads_or_q, want, packed=False):
    if packed:
        gq = V.Queries.from_host_packed(reads_or_q.ravel(), M)
    else:
        q = reads_or_q
        gq = V.Queries.from_host(q.symbols, q.start, q.length)
    r = V.findquerymatches(gi, gq, L, mum=True)
    got = r.fetch()
    assert np.array_equal(got, want)
    gq.close()
    return r


@pytest.mark.parametrize("tune", TUNES)
@pytest.mark.parametrize("packed", [False, True], ids=["bytes", "packed"])
def test_many_buckets(V, text, monkeypatch, tune, packed):
    """200 k reads spread over the text, a quarter with one substitution"""
    reads = many_reads(text)
    q = H.Queries.uniform(reads.ravel(), M)
    want = oracle(text, "many", q)
    assert len(want) > 100_000
    gi = index_for(V, monkeypatch, text, tune)
    before = sort_counters(V)
    r = check(V, gi, reads if packed else q, want, packed)
    after = sort_counters(V)
    assert r.stats().candidates >= len(want)
    assert by_buckets(tune, r) == (tune != 4)
    if tune != 4:
        assert after["runs"] == before["runs"] + 1
        assert after["overflows"] == before["overflows"]
        assert after["buckets"] > 50
    else:
        assert after == before


@pytest.mark.parametrize("tune", TUNES)
def test_many_buckets_wide_tables(V, text, monkeypatch, tune):
    """the same on 64-bit device tables (VSA_FORCE_WIDE=1: the search kernels
    that feed the sort in their uint64_t instantiation; the values stay four
    bytes wide -- test_eight_byte_values has the others)"""
    reads = many_reads(text)
    q = H.Queries.uniform(reads.ravel(), M)
    want = oracle(text, "many", q)
    gi = index_for(V, monkeypatch, text, tune, wide=True)
    before = sort_counters(V)
    check(V, gi, q, want)
    check(V, gi, reads, want, packed=True)
    after = sort_counters(V)
    if tune != 4:
        assert after["runs"] == before["runs"] + 2
        assert after["overflows"] == before["overflows"]


@pytest.mark.parametrize("tune", TUNES)
def test_eight_byte_values(V, text, monkeypatch, tune):
    """query number and offset beyond 32 bits -- 70 k reads, one of them
    40 000 symbols long, so 16 bits of offset -- travel as 8-byte values
    (16-byte staging entries)"""
    tis = text["tis"]
    rng = np.random.default_rng(16)
    reads = [r for r in cut_reads(tis, rng.integers(0, N - M, 70_000), rng)]
    long_read = tis[1_200_000:1_240_000].copy()
    for p in (777, 20_000, 20_030, 39_000):
        long_read[p] = (long_read[p] + 1) % 4
    reads.insert(12_345, long_read)
    q = H.Queries.from_list(reads)
    assert (q.nq << 16) >= (1 << 32)
    want = oracle(text, "eight", q)
    assert len(want) > 30_000 and int(want["length"].max()) > 10_000
    gi = index_for(V, monkeypatch, text, tune)
    before = sort_counters(V)
    check(V, gi, q, want)
    after = sort_counters(V)
    if tune != 4:
        assert after["runs"] == before["runs"] + 1
        assert after["overflows"] == before["overflows"]
        assert after["buckets"] > 10


def falls_back(V, text, monkeypatch, tune, name, reads):
    """a batch the bucket sort gives up on: the list is the oracle's every
    time; under VSA_TUNE=8 every call tries the buckets and is counted as an
    overflow; by default the index backs off -- after the first overflow one
    call goes straight to rocPRIM, after the second two"""
    q = H.Queries.uniform(reads.ravel(), M)
    want = oracle(text, name, q)
    gi = index_for(V, monkeypatch, text, tune, fresh=True)
    tried = []
    for call in range(6):
        before = sort_counters(V)
        r = check(V, gi, q, want)
        after = sort_counters(V)
        assert r.stats().candidates >= MINPAIRS
        assert after["overflows"] - before["overflows"] == (
            after["runs"] - before["runs"])
        tried.append(after["runs"] - before["runs"])
    assert tried == {0: [1, 0, 1, 0, 0, 1], 4: [0] * 6, 8: [1] * 6}[tune]
    return sort_counters(V)


@pytest.mark.parametrize("tune", TUNES)
def test_one_window_overflows_a_bucket_and_falls_back(V, text, monkeypatch,
                                                      tune):
    """more than 4 x CAP reads cut from a window narrower than a bucket: the
    bucket sort gives up (counted) and rocPRIM sorts the list"""
    rng = np.random.default_rng(12)
    nreads = 4 * CAP + 3000
    reads = cut_reads(text["tis"], 700_000 + rng.integers(0, 3000, nreads),
                      rng)
    after = falls_back(V, text, monkeypatch, tune, "window", reads)
    if tune != 4:
        assert (3000 + M) < (1 << after["shift"])   # narrower than a bucket


@pytest.mark.parametrize("tune", TUNES)
def test_one_amplicon_overflows_a_bin_and_falls_back(V, text, monkeypatch,
                                                     tune):
    """17 k reads spread over the text and 1 500 from a window of 150
    positions: every bucket fits, but one bin of the sort inside a bucket
    holds thousands of pairs (VSA_CS_BINLIMIT = 256), and the call falls
    back instead of ranking them quadratically"""
    rng = np.random.default_rng(17)
    starts = np.concatenate([rng.integers(0, N - M, 17_000),
                             1_300_000 + rng.integers(0, 150, 1_500)])
    reads = cut_reads(text["tis"], rng.permutation(starts), rng)
    after = falls_back(V, text, monkeypatch, tune, "amplicon", reads)
    if tune != 4:
        # no bucket was over its capacity: it was a bin
        gi = index_for(V, monkeypatch, text, tune)
        gq = V.Queries.from_host_packed(reads.ravel(), M)
        cand = V.findquerymatches(gi, gq, L, mum=True, cand=True).fetch()
        gq.close()
        fill = np.bincount((cand["dbstart"] >> np.uint64(after["shift"]))
                           .astype(np.int64))
        assert after["buckets"] > 1 and len(cand) >= MINPAIRS
        assert fill.max() <= CAP
        assert np.bincount((cand["dbstart"] >> np.uint64(
            max(after["shift"] - 11, 0))).astype(np.int64)).max() > 256


@pytest.mark.parametrize("tune", TUNES)
def test_sixteen_byte_entries_for_four_byte_values(V, text, monkeypatch,
                                                   tune):
    """few reads, one of them 40 000 symbols long: 16 length bits, values of
    four bytes, one bucket as wide as the text (shift = 21), 16 + 21 > 32 --
    the staging entries are {key, value} although the values are narrow"""
    tis = text["tis"]
    rng = np.random.default_rng(18)
    reads = [r for r in cut_reads(tis, rng.integers(0, N - M, 900), rng)]
    for at in (300_000, 1_500_000):
        long_read = tis[at:at + 40_000].copy()
        for p in (555, 21_000, 21_040, 38_000):
            long_read[p] = (long_read[p] + 1) % 4
        reads.insert(100, long_read)
    q = H.Queries.from_list(reads)
    assert (q.nq << 16) < (1 << 32)     # four-byte values
    want = oracle(text, "sixteen", q)
    assert len(want) > 500 and int(want["length"].max()) > 10_000
    gi = index_for(V, monkeypatch, text, tune)
    before = sort_counters(V)
    check(V, gi, q, want)
    after = sort_counters(V)
    assert after["runs"] - before["runs"] == (1 if tune == 8 else 0)
    if tune == 8:
        assert after["overflows"] == before["overflows"]
        assert after["buckets"] == 1 and after["shift"] + 16 > 32


@pytest.mark.parametrize("tune", TUNES)
def test_runs_of_equal_dbstart_across_bucket_boundaries(V, text, monkeypatch,
                                                        tune):
    """the run situations of test_mum_filter_runs_of_equal_dbstart -- a
    unique longest member, the longest twice, a run of more than 64 that
    forces the second attempt -- with the starts at k << shift and
    (k << shift) - 1, so that runs and the matches that cover them lie on
    both sides of a bucket boundary; 200 k reads around them make the
    buckets"""
    tis = text["tis"]
    rng = np.random.default_rng(13)
    B = 1 << 15     # a multiple of every bucket width up to 2^15

    def read(p, length):
        # ends in a foreign symbol so that the match stops at `length`
        r = np.concatenate([tis[p:p + length],
                            [(int(tis[p + length]) + 1) % 4]])
        return r.astype(np.uint8)

    background = [r for r in cut_reads(
        tis, rng.integers(0, N - M, 200_000), rng)]
    for name, runs in (
            ("short", [(3 * B, [30, 40, 50, 35]), (3 * B - 1, [60, 60, 45]),
                       (7 * B - 1, [25]), (7 * B, [80, 70, 80, 30]),
                       (9 * B, list(range(30, 40))), (9 * B - 1, [95, 33])]),
            # (a run goes to the second attempt when its survivor has more
            # than 64 members on one side: certain from 130 members on)
            ("long", [(5 * B, list(range(30, 131))), (5 * B - 1, [50, 40]),
                      (11 * B - 1, [50, 140]),
                      (13 * B, list(range(30, 161)))]),
            ("twice", [(4 * B, [90] * 70 + [95]),
                       (6 * B - 1, [90] * 70 + [95, 95]),
                       (6 * B, [40] * 3), (8 * B - 1, [150] * 140 + [190])])):
        reads = [read(p, m) for p, ms in runs for m in ms] + background
        order = rng.permutation(len(reads))
        q = H.Queries.from_list([reads[i] for i in order])
        want = oracle(text, "runs-" + name, q)
        gi = index_for(V, monkeypatch, text, tune)
        before = sort_counters(V)
        check(V, gi, q, want)
        after = sort_counters(V)
        if tune != 4:
            assert after["runs"] == before["runs"] + 1
            assert after["overflows"] == before["overflows"]
            assert after["buckets"] > 1 and after["shift"] <= 15
            # a run of more than 64: the second attempt, on all bits
            assert (after["longruns"] - before["longruns"]) == (
                0 if name == "short" else 1)


@pytest.mark.parametrize("tune", TUNES)
def test_tiny_batches_and_one_without_candidates(V, text, monkeypatch, tune):
    tis = text["tis"]
    rng = np.random.default_rng(14)
    gi = index_for(V, monkeypatch, text, tune)
    for nreads in (1, 2, 300):
        reads = cut_reads(tis, rng.integers(0, N - M, nreads), rng)
        q = H.Queries.uniform(reads.ravel(), M)
        want = oracle(text, "tiny-%d" % nreads, q)
        assert len(want) > 0
        before = sort_counters(V)
        check(V, gi, q, want)
        check(V, gi, reads, want, packed=True)
        after = sort_counters(V)
        assert after["runs"] - before["runs"] == (2 if tune == 8 else 0)
        if tune == 8:
            assert after["buckets"] == 1
    # reads that are nowhere in the text
    foreign = np.random.default_rng(15).integers(0, 4, 5 * M).astype(np.uint8)
    q = H.Queries.uniform(foreign, M)
    want = oracle(text, "foreign", q)
    assert len(want) == 0
    r = check(V, gi, q, want)
    assert r.stats().candidates == 0

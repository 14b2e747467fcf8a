"""The tile queue of the planned MUM search (k_mum_walk_tiles,
mum_workplan.inc): wavefronts take tiles of 64 entries of the list of planned
reads from one counter, and the free lanes of a wavefront take the next chunks
of its tile in front of every locate.  A scheduling change only: the chunks,
the locates and the candidates are those of the workgroup tiles of
k_query_search_planned, which VSA_TUNE=32 brings back.

Every case: -mum cand and -mum against the CPU oracle; count, candidates,
sumlength, searches and kernel_searches EQUAL between an index made by default
and one made under VSA_TUNE=32; the lists also equal under VSA_TUNE=16 (every
planned offset a work-item).  The library reads the switches when an index is
created."""
import numpy as np
import pytest

import helpers as H
from test_gpu_mum_walk import host_index, other, random_text, substituted

pytestmark = pytest.mark.gpu

M = 100
SWITCHES = ("VSA_TUNE", "VSA_WALK_CHUNK", "VSA_WALK_GRID", "VSA_NO_ESA8",
            "VSA_FORCE_WIDE", "VSA_DEEP_PREFIX")
COUNTERS = ("count", "candidates", "sumlength", "searches", "kernel_searches")


def build(V, monkeypatch, tis, tune=0, env=()):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    if tune:
        monkeypatch.setenv("VSA_TUNE", str(tune))
    return V.Index.build(tis, 4, 0)


def check(V, monkeypatch, tis, hq, L, env=(), packed=None, counters=True,
          tune=0, calls=1):
    """packed: the length of the reads if the batch goes as packed rows as
    well; counters: rows and bytes must then make the same searches (asked
    where check() of test_gpu_mum_walk.py asks it: not of reads with special
    symbols); tune: VSA_TUNE bits every index is made under; calls: how often
    the tile queue's index answers each call.  Returns the statistics of the
    default index by form."""
    stats = {}
    want = None
    for name, bits in (("queue", 0), ("workgroup", 32), ("items", 16)):
        gi = build(V, monkeypatch, tis, tune | bits, env)
        if want is None:
            L = max(L, gi.info().prefixlength)
            host = host_index(gi, len(tis))
            want = (H.oracle_querymatches(host, hq, L, mum=True, cand=True,
                                          speedup=0),
                    H.oracle_querymatches(host, hq, L, mum=True, speedup=0))
        forms = [("bytes", V.Queries.from_host(hq.symbols, hq.start,
                                               hq.length))]
        if packed is not None:
            forms.append(("rows", V.Queries.from_host_packed(hq.symbols,
                                                             packed)))
        for form, gq in forms:
            for call in range(calls if name == "queue" else 1):
                cand = V.findquerymatches(gi, gq, L, mum=True, cand=True)
                assert np.array_equal(cand.fetch(), want[0]), (name, form)
                mum = V.findquerymatches(gi, gq, L, mum=True)
                assert np.array_equal(mum.fetch(), want[1]), (name, form)
                got = (cand.stats(), mum.stats())
                if call > 0:
                    for k in (0, 1):
                        for c in COUNTERS:
                            assert getattr(got[k], c) == \
                                getattr(stats[name, form][k], c), (call, c)
                stats[name, form] = got
    forms = ("bytes", "rows")[:1 + (packed is not None)]
    for form in forms:
        for k in (0, 1):
            a, b = stats["queue", form][k], stats["workgroup", form][k]
            print(form, "-mum" + " cand" * (1 - k),
                  {c: (getattr(a, c), getattr(b, c)) for c in COUNTERS})
            assert a.count == len(want[k])
            for c in COUNTERS:
                assert getattr(a, c) == getattr(b, c), (form, k, c)
    if packed is not None and counters:
        for k in (0, 1):
            b, r = stats["queue", "bytes"][k], stats["queue", "rows"][k]
            assert b.searches == r.searches
            assert b.kernel_searches == r.kernel_searches
    return {form: stats["queue", form] for form in forms}


def chimera(rng, tis, m):
    """the first half from one place of the text, the second from another:
    the offset at the joint is a candidate the SEARCH kernel finds (the plan
    answers only the fresh start behind the first mismatch)"""
    a, b = (int(p) for p in rng.integers(0, len(tis) - m, 2))
    q = np.concatenate([tis[a:a + m // 2], tis[b:b + m - m // 2]])
    q[q >= 4] = rng.integers(0, 4)
    return q


def planned_and_exact(rng, tis, nq, planned):
    """nq reads, `planned` of them with a substitution or a joint (the others
    match end to end: the first pass finishes them, the list leaves them out)"""
    which = set(rng.choice(nq, planned, replace=False).tolist())
    reads = []
    for i in range(nq):
        p = int(rng.integers(0, len(tis) - M))
        if i not in which:
            reads.append(tis[p:p + M].copy())
        elif i % 3 == 0:
            reads.append(chimera(rng, tis, M))
        else:
            reads.append(substituted(rng, tis, p, M,
                                     [int(rng.integers(0, M))]))
    return np.concatenate(reads)


@pytest.mark.parametrize("planned", [0, 1, 63, 64, 65, 129])
def test_tile_edges(V, monkeypatch, planned):
    """no planned read at all (an empty list: every wavefront finds the
    counter run out), one, a tile short of one lane, a full tile, one read in
    a second tile, one in a third"""
    rng = np.random.default_rng(1600 + planned)
    tis = random_text(rng, 40000)
    block = planned_and_exact(rng, tis, 2400, planned)
    stats = check(V, monkeypatch, tis, H.Queries.uniform(block, M), 20,
                  packed=M)
    if planned == 0:
        assert stats["rows"][0].kernel_searches == \
            stats["bytes"][0].kernel_searches


def multi_substitution_reads(rng, tis, nq, m):
    return np.concatenate(
        [substituted(rng, tis, int(rng.integers(0, len(tis) - m)), m,
                     rng.choice(m, 2 + i % 5, replace=False))
         if i % 4 else chimera(rng, tis, m) for i in range(nq)])


@pytest.mark.parametrize("chunk", ["1", "2", "4", "32"])
def test_tiles_with_far_more_chunks_than_lanes(V, monkeypatch, chunk):
    """two to six substitutions in reads of 200 symbols: up to four ranges
    and dozens of chunks per read, a tile handed out over many rounds, chunk
    edges on range edges; bytes and rows"""
    rng = np.random.default_rng(1610)
    m = 200
    tis = random_text(rng, 50000)
    block = multi_substitution_reads(rng, tis, 1200, m)
    check(V, monkeypatch, tis, H.Queries.uniform(block, m), 16,
          env=(("VSA_WALK_CHUNK", chunk),), packed=m)


@pytest.mark.parametrize("env", [(("VSA_FORCE_WIDE", "1"),),
                                 (("VSA_NO_ESA8", "1"),)],
                         ids=["wide", "reference_walk"])
def test_wide_tables_and_no_deep_tables(V, monkeypatch, env):
    rng = np.random.default_rng(1611)
    m = 200
    tis = random_text(rng, 30000, wild=0.0003, seps=1)
    block = multi_substitution_reads(rng, tis, 800, m)
    check(V, monkeypatch, tis, H.Queries.uniform(block, m), 16,
          env=env + (("VSA_WALK_CHUNK", "4"),), packed=m)


def test_bucket_sort_behind_the_queue(V, monkeypatch):
    """VSA_TUNE=8: the candidates go from the cursor regions straight into
    the bucket sort, whose scatter reads the cursors (the tile counter lies
    behind them)"""
    rng = np.random.default_rng(1612)
    tis = random_text(rng, 60000)
    block = planned_and_exact(rng, tis, 2400, 1500)
    check(V, monkeypatch, tis, H.Queries.uniform(block, M), 20, packed=M,
          tune=8)


def test_one_long_walk_beside_many_short_ones(V, monkeypatch):
    """a ragged byte batch: a few reads of 5 000 symbols with many
    substitutions among reads of 100 -- a lane stays busy through many tiles;
    the wavefront must neither leave early nor fetch behind the list"""
    rng = np.random.default_rng(1613)
    n = 60000
    tis = random_text(rng, n)
    reads = []
    for i in range(900):
        if i in (5, 300, 301, 899):
            p = int(rng.integers(0, n - 5000))
            reads.append(substituted(rng, tis, p, 5000,
                                     rng.choice(5000, 150, replace=False)))
        elif i % 3 == 0:
            reads.append(chimera(rng, tis, M))
        else:
            p = int(rng.integers(0, n - M))
            reads.append(substituted(rng, tis, p, M,
                                     [int(rng.integers(0, M))][:i % 2]))
    for chunk in ("32", "4"):
        check(V, monkeypatch, tis, H.Queries.from_list(reads), 20,
              env=(("VSA_WALK_CHUNK", chunk),))


def test_one_workgroup_takes_every_tile(V, monkeypatch):
    """VSA_WALK_GRID=1: four wavefronts, about 3 000 planned reads, one
    cursor region for every candidate of the search kernel -- more than its
    first capacity (256 records for a batch of this size; two of three reads
    have a joint, about three quarters of those a candidate there), so the
    search runs a second time, from a tile counter that was zeroed again"""
    rng = np.random.default_rng(1614)
    tis = random_text(rng, 60000)
    block = np.concatenate(
        [chimera(rng, tis, M) if i % 3 else
         substituted(rng, tis, int(rng.integers(0, len(tis) - M)), M,
                     [int(rng.integers(0, M))]) for i in range(3000)])
    stats = check(V, monkeypatch, tis, H.Queries.uniform(block, M), 20,
                  env=(("VSA_WALK_GRID", "1"),), packed=M, calls=2)
    # (candidates of the first pass and of the plan are not the kernel's: the
    # reads with a joint alone are enough)
    assert stats["rows"][0].candidates > 1000


def test_far_more_workgroups_than_tiles(V, monkeypatch):
    """most wavefronts find the counter run out at once"""
    rng = np.random.default_rng(1615)
    tis = random_text(rng, 40000)
    block = planned_and_exact(rng, tis, 2400, 100)
    check(V, monkeypatch, tis, H.Queries.uniform(block, M), 20,
          env=(("VSA_WALK_GRID", "4096"),), packed=M)


@pytest.mark.parametrize("chunk", ["32", "1"])
def test_reads_with_wildcards_in_a_packed_batch(V, monkeypatch, chunk):
    """every read is planned, so tile t holds reads 64 t ... 64 t + 63: the
    first tile has 64 reads with a wildcard of their own (all set aside; with
    chunks of 1 more chunks than the list holds at once), the second one, the
    third none; the lists equal those of the byte batch (both equal the
    oracle's)"""
    rng = np.random.default_rng(1616)
    tis = random_text(rng, 40000, wild=0.0003)
    reads = []
    for i in range(192):
        p = int(rng.integers(0, len(tis) - M))
        q = substituted(rng, tis, p, M, [int(rng.integers(30, M - 10))]) \
            if i % 4 else chimera(rng, tis, M)
        if i <= 64:
            q[int(rng.integers(5, M - 5))] = H.WILDCARD
        reads.append(q)
    check(V, monkeypatch, tis, H.Queries.uniform(np.concatenate(reads), M),
          20, env=(("VSA_WALK_CHUNK", chunk),), packed=M, counters=False)


def test_two_calls_in_a_row(V, monkeypatch):
    """the tile counter is zeroed per call: the second call on one index
    makes the same searches and returns the same lists"""
    rng = np.random.default_rng(1617)
    tis = random_text(rng, 40000)
    block = planned_and_exact(rng, tis, 2400, 700)
    check(V, monkeypatch, tis, H.Queries.uniform(block, M), 20, packed=M,
          calls=3)

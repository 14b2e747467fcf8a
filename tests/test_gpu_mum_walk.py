"""The walk of the planned MUM search (mum_workplan.inc, mum_walk.inc): a lane
takes a chunk of a plan range from its last offset down and leaves out the
offsets whose match cannot reach the least length l any more, because
e(j) = j + (longest match at j) never decreases: after offset h, every j with
e(h) - l < j < h.

Every case: -mum cand and -mum against the CPU oracle, and against the same
call on an index made under VSA_TUNE=16 (no walk: every planned offset
located) and under VSA_TUNE=2 (no plan either: every offset) -- lists equal,
`candidates` equal, kernel_searches in the order walk <= no walk <=
exhaustive.  The library reads the switches when an index is created."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

M, NQ = 100, 2400


def random_text(rng, n, wild=0.0, seps=0):
    t = rng.integers(0, 4, n).astype(np.uint8)
    if wild:
        t[rng.random(n) < wild] = H.WILDCARD
    for p in rng.choice(np.arange(100, n - 100), seps, replace=False):
        t[p] = H.SEPARATOR
    return t


def other(rng, sym):
    """a regular symbol that differs from sym"""
    return (int(sym) + 1 + int(rng.integers(0, 3))) % 4 if sym < 4 else 1


def substituted(rng, tis, p, m, places):
    q = tis[p:p + m].copy()
    q[q >= 4] = rng.integers(0, 4)
    for x in places:
        q[x] = other(rng, q[x])
    return q


def build(V, monkeypatch, tis, tune=None, env=()):
    for k in ("VSA_TUNE", "VSA_WALK_CHUNK", "VSA_NO_ESA8", "VSA_FORCE_WIDE",
              "VSA_DEEP_PREFIX"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    if tune is not None:
        monkeypatch.setenv("VSA_TUNE", tune)
    return V.Index.build(tis, 4, 0)


def host_index(gi, n):
    t = gi.download()
    return H.Index(n, gi.info().prefixlength, 4, t["tis"], t["suf"], t["lcp"],
                   t["llv"], t["bck"], t["bwt"], None)


def check(V, monkeypatch, tis, hq, least, env=(), packed=None, ratio=None,
          counters=True):
    """least: l, or a function (prefixlength, D) -> l.  packed: the length of
    the reads if the batch is to go as packed rows as well; counters: rows
    and bytes must then make the same number of searches (not asked of a
    batch with special symbols in its reads: the plan kernel takes such a read
    of a packed batch through the reference walk and may plan other offsets
    than for its bytes, with or without the walk).  Returns the statistics
    by switch and form, l, and the oracle's lists (-mum cand, -mum)."""
    stats = {}
    want = None
    for name, tune in (("walk", None), ("nowalk", "16"), ("all", "2")):
        gi = build(V, monkeypatch, tis, tune, env)
        if want is None:
            info = gi.info()
            L = least(info.prefixlength, info.deepprefix) if callable(least) \
                else max(least, info.prefixlength)
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
            cand = V.findquerymatches(gi, gq, L, mum=True, cand=True)
            assert np.array_equal(cand.fetch(), want[0]), (name, form)
            mum = V.findquerymatches(gi, gq, L, mum=True)
            assert np.array_equal(mum.fetch(), want[1]), (name, form)
            stats[name, form] = (cand.stats(), mum.stats())
    for form in ("bytes", "rows")[:1 + (packed is not None)]:
        for k in (0, 1):
            w, o, a = (stats[name, form][k] for name in
                       ("walk", "nowalk", "all"))
            print(form, "-mum" + " cand" * (1 - k), "kernel_searches walk",
                  w.kernel_searches, "no walk", o.kernel_searches,
                  "exhaustive", a.kernel_searches)
            assert w.candidates == o.candidates == a.candidates
            assert w.count == o.count == a.count == len(want[k])
            assert w.sumlength == o.sumlength
            assert w.kernel_searches <= o.kernel_searches <= a.kernel_searches
            if ratio is not None:
                assert w.kernel_searches < o.kernel_searches * ratio
    if packed is not None and counters:
        for name in ("walk", "nowalk", "all"):
            for k in (0, 1):
                b, r = stats[name, "bytes"][k], stats[name, "rows"][k]
                assert b.searches == r.searches, name
                assert b.kernel_searches == r.kernel_searches, name
    return stats, L, want


def test_matches_planted_around_the_skip_boundary(V, monkeypatch):
    """a read with one substitution at x has the range (x + 1 - l, x]; for
    h = x, x - 1 and the first offset of the range, read[h : h + k] stands a
    second time in the text, followed by another symbol, for k = l - 2 ...
    l + 1: the walk must reach h when k >= l whatever it skipped above it"""
    rng = np.random.default_rng(1301)
    L, n = 20, 60000
    tis = random_text(rng, n)
    reads, planted = [], []
    for i in range(40):     # (480 copies 60 symbols apart: none on another)
        x = int(rng.integers(L + 4, M - L - 1))
        for h in (x, x - 1, x + 2 - L):
            for k in (L - 2, L - 1, L, L + 1):
                # sources in the first third, copies in the last: a copy never
                # lands on a source
                p = (len(reads) * 97) % (n // 3 - M) + 1
                q = substituted(rng, tis, p, M, [x])
                at = n // 3 + 200 + len(reads) * 60 % (n // 2)
                tis[at:at + k] = q[h:h + k]
                tis[at + k] = other(rng, q[h + k])
                tis[at - 1] = other(rng, q[h - 1])
                planted.append((len(reads), h, k, at))
                reads.append(q)
    assert n // 3 + 200 + len(reads) * 60 + L + 2 < n
    hq = H.Queries.uniform(np.concatenate(reads), M)
    stats, _, want = check(V, monkeypatch, tis, hq, L, packed=M)
    # every copy of l and more symbols is a candidate at its offset, with its
    # length, at its place (the lists of all three indexes equal this one)
    cand = want[0]
    have = set(zip(cand["queryseq"].tolist(), cand["querystart"].tolist(),
                   cand["length"].tolist(), cand["dbstart"].tolist()))
    for i, h, k, at in planted:
        assert ((i, h, k, at) in have) == (k >= L), (i, h, k)


def test_one_substitution_at_the_ends_of_a_read(V, monkeypatch):
    """at 0, 1, m - l - 1, m - l and m - 1: ranges clipped by the last offset
    that can be searched, and empty ranges"""
    rng = np.random.default_rng(1302)
    L, n = 20, 50000
    tis = random_text(rng, n)
    places = (0, 1, M - L - 1, M - L, M - 1)
    reads = [substituted(rng, tis, int(rng.integers(0, n - M)), M,
                         [places[i % 5]]) for i in range(NQ)]
    check(V, monkeypatch, tis, H.Queries.uniform(np.concatenate(reads), M), L,
          packed=M)


@pytest.mark.parametrize("chunk", ["32", "4"])
def test_two_to_six_substitutions(V, monkeypatch, chunk):
    """more ranges than a plan has slots: a last range stretched over dead
    offsets, and ranges longer than a chunk (reads of 200 symbols)"""
    rng = np.random.default_rng(1303)
    L, n, m = 16, 50000, 200
    tis = random_text(rng, n)
    reads = [substituted(rng, tis, int(rng.integers(0, n - m)), m,
                         rng.choice(m, 2 + i % 5, replace=False))
             for i in range(NQ // 2)]
    check(V, monkeypatch, tis, H.Queries.uniform(np.concatenate(reads), m), L,
          env=(("VSA_WALK_CHUNK", chunk),), packed=m)


def slow_path_batch(rng):
    """a text of three sequences with wildcards and copies of a 400-symbol
    unit (ties on all key symbols: the reference walk), reads from it with
    substitutions, a wildcard inside a range, reads across a boundary, reads
    of random symbols (no deep bucket) and whole copies of the unit (matches
    end to end at every offset)"""
    unit = rng.integers(0, 4, 400).astype(np.uint8)
    seqs = []
    for s in range(3):
        t = random_text(rng, 20000, wild=0.0005)
        for r in range(6):
            p = int(rng.integers(0, 20000 - 400))
            u = unit.copy()
            for e in range(int(rng.integers(0, 3))):
                u[int(rng.integers(0, 400))] = rng.integers(0, 4)
            t[p:p + 400] = u
        seqs.append(t)
    tis = np.concatenate([seqs[0], [H.SEPARATOR], seqs[1], [H.SEPARATOR],
                          seqs[2]]).astype(np.uint8)
    reads = []
    for i in range(NQ):
        kind = i % 8
        p = int(rng.integers(0, len(tis) - M))
        if kind == 0:
            q = rng.integers(0, 4, M).astype(np.uint8)
        elif kind == 1:
            at = int(rng.integers(0, 300))
            q = unit[at:at + M].copy()
            if i % 16 == 1:
                q[int(rng.integers(0, M))] ^= 1
        else:
            # (wildcards and separators of the text stay under the read's
            # match: the read carries a regular symbol there)
            q = tis[p:p + M].copy()
            q[q >= 4] = rng.integers(0, 4)
            for x in rng.choice(M, kind - 2, replace=False):
                q[x] = other(rng, q[x])
        if kind in (2, 3, 5):
            # a wildcard of the read's own, next to a substitution
            x = int(rng.integers(30, M - 10))
            q[x] = other(rng, q[x])
            q[x - int(rng.integers(1, 19))] = H.WILDCARD
        reads.append(q)
    return tis, np.concatenate(reads)


def test_slow_paths(V, monkeypatch):
    rng = np.random.default_rng(1304)
    tis, block = slow_path_batch(rng)
    check(V, monkeypatch, tis, H.Queries.uniform(block, M), 20, packed=M,
          counters=False)


@pytest.mark.parametrize("which", ["prefixlength", "D-1", "D", "D+1"])
def test_least_lengths_around_the_deep_prefix(V, monkeypatch, which):
    """l <= D: the bound of a locate that finds no deep bucket, D - 1, skips
    nothing; l = D + 1 is the first length at which it does"""
    rng = np.random.default_rng(1305)
    n = 40000
    tis = random_text(rng, n, wild=0.0003, seps=2)
    reads = [substituted(rng, tis, int(rng.integers(0, n - M)), M,
                         rng.choice(M, i % 4, replace=False))
             for i in range(NQ // 2)]

    def least(pl, D):
        return {"prefixlength": pl, "D-1": max(pl, D - 1), "D": max(pl, D),
                "D+1": max(pl, D + 1)}[which]
    stats, L, _ = check(V, monkeypatch, tis,
                        H.Queries.uniform(np.concatenate(reads), M), least,
                        packed=M)
    if which in ("prefixlength", "D"):
        # nothing may be skipped.  l = prefixlength: a bucket means a match of
        # l symbols, none a bound of l - 1.  l = D: a deep bucket means D
        # symbols, none the bound D - 1, and no suffix of these reads (no
        # special symbol, l symbols left at every offset) is shorter than D.
        for form in ("bytes", "rows"):
            for k in (0, 1):
                assert stats["walk", form][k].kernel_searches == \
                    stats["nowalk", form][k].kernel_searches, (form, k)


@pytest.mark.parametrize("env", [(("VSA_FORCE_WIDE", "1"),),
                                 (("VSA_NO_ESA8", "1"),)],
                         ids=["wide", "reference_walk"])
def test_wide_tables_and_the_index_without_deep_tables(V, monkeypatch, env):
    rng = np.random.default_rng(1306)
    tis, block = slow_path_batch(rng)
    check(V, monkeypatch, tis, H.Queries.uniform(block, M), 20, env=env,
          packed=M, counters=False)
    # rows and bytes with equal counters: reads without a special symbol
    tis = random_text(rng, 40000, wild=0.0003, seps=1)
    reads = [substituted(rng, tis, int(rng.integers(0, len(tis) - M)), M,
                         rng.choice(M, i % 4, replace=False))
             for i in range(NQ // 2)]
    check(V, monkeypatch, tis, H.Queries.uniform(np.concatenate(reads), M),
          20, env=env, packed=M)


def test_ragged_batch(V, monkeypatch):
    """reads shorter than l, of exactly l and of l + 1 symbols among longer
    ones"""
    rng = np.random.default_rng(1307)
    L, n = 20, 40000
    tis = random_text(rng, n, wild=0.0003, seps=1)
    reads = []
    for i in range(NQ):
        m = (L - 3, L, L + 1, 0, 40, 64, 100, 257)[i % 8]
        q = tis[int(rng.integers(0, n - 300)):][:m].copy()
        q[q == H.SEPARATOR] = rng.integers(0, 4)
        for x in rng.choice(max(m, 1), min(m, i % 3), replace=False):
            q[x] = other(rng, q[x])
        reads.append(q)
    check(V, monkeypatch, tis, H.Queries.from_list(reads), L)


def test_random_text_one_substitution_halves_the_searches(V, monkeypatch):
    """l >= D + 4 on a random text, one substitution per read: a match of
    about log4 n symbols disposes of l - log4 n offsets per locate, the walk
    makes fewer than half of the planned searches"""
    rng = np.random.default_rng(1308)
    n = 100000
    tis = random_text(rng, n)
    reads = [substituted(rng, tis, int(rng.integers(0, n - M)), M,
                         [int(rng.integers(0, M))]) for i in range(NQ)]
    stats, L, _ = check(V, monkeypatch, tis,
                     H.Queries.uniform(np.concatenate(reads), M),
                     lambda pl, D: max(pl, D + 4), packed=M, ratio=0.5)
    assert L >= 13

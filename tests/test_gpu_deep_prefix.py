"""Deep prefixes D = 13..16 (index_derive.hip: ceil(log4 n), at most 16) on
the data where they matter: repeat-rich genome-like texts of 64 and 200 Mbp
built on the GPU (D = 13 and 14 by themselves), and small texts with D forced
far above log4 n (VSA_DEEP_PREFIX), where almost every bucket is empty.
Reads of four families -- from the text, with several substitutions and
indels, from an unrelated genome, with wildcards at offset 0, D - 1, inside
the key window and elsewhere -- as bytes and as packed rows; every mode
against the CPU oracle on the same tables, in order, at search lengths below,
at and above D.  Set VSA_DEEP_PREFIX_BP to run other text sizes (comma
separated)."""
import os

import numpy as np
import pytest

import helpers as H
from test_gpu_parity import mum_hard_batch

pytestmark = pytest.mark.gpu

SIZES = [int(float(x)) for x in
         os.environ.get("VSA_DEEP_PREFIX_BP", "64e6,2e8").split(",")]


def repeat_rich_text(n, seed):
    """24 sequences of random DNA in which ~45 % is covered by copies of ten
    repeat families (consensus 300..6000 symbols, each copy 5..20 %
    substituted), tandem satellites (units of 2..180 symbols repeated over
    1..20 kbp) and runs of 10^3..10^5 wildcards"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, n).astype(np.uint8)
    fams = [rng.integers(0, 4, int(rng.integers(300, 6001))).astype(np.uint8)
            for _ in range(10)]
    covered = 0
    while covered < 0.45 * n:
        c = fams[int(rng.integers(0, 10))].copy()
        d = rng.uniform(0.05, 0.2)
        hit = rng.random(len(c)) < d
        c[hit] = (c[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        p = int(rng.integers(0, n - len(c)))
        t[p:p + len(c)] = c
        covered += len(c)
    for _ in range(max(4, n // 2000000)):
        u = rng.integers(0, 4, int(rng.integers(2, 181))).astype(np.uint8)
        span = int(rng.integers(1000, 20001))
        p = int(rng.integers(0, n - span))
        t[p:p + span] = np.resize(u, span)
    for _ in range(max(4, n // 4000000)):
        span = int(10 ** rng.uniform(3, 5))
        p = int(rng.integers(0, n - span))
        t[p:p + span] = H.WILDCARD
    for p in np.sort(rng.choice(np.arange(1000, n - 1000), 23,
                                replace=False)):
        t[p] = H.SEPARATOR
    return t


def family_reads(rng, tis, nq, m, D):
    """nq reads of m symbols, families interleaved: (a) exact copies and one
    substitution, (b) 4 % substitutions and 0.5 % indels per symbol, (c) an
    unrelated random genome, (d) 1..3 wildcards at 0, D - 1, D .. D + 9 or
    anywhere.  Reads that would cross a separator are cut elsewhere."""
    other = rng.integers(0, 4, 10 * m * nq).astype(np.uint8)
    out = np.zeros((nq, m), np.uint8)
    n = len(tis)
    for i in range(nq):
        fam = i % 4
        if fam == 2:
            p = int(rng.integers(0, len(other) - m))
            out[i] = other[p:p + m]
            continue
        while True:
            p = int(rng.integers(0, n - 2 * m))
            src = tis[p:p + 2 * m]
            if not (src == H.SEPARATOR).any():
                break
        if fam == 1:
            q = []
            k = 0
            while len(q) < m:
                r = rng.random()
                if r < 0.0025:
                    k += 1                       # deletion
                elif r < 0.005:
                    q.append(int(rng.integers(0, 4)))   # insertion
                else:
                    c = int(src[k])
                    if rng.random() < 0.04 and c < 4:
                        c = (c + int(rng.integers(1, 4))) % 4
                    q.append(c)
                    k += 1
            out[i] = q[:m]
        else:
            out[i] = src[:m]
            if fam == 0 and i % 8 == 4:
                x = int(rng.integers(0, m))
                out[i, x] = (out[i, x] + 1) % 4 if out[i, x] < 4 else 0
            if fam == 3:
                places = [0, D - 1, D + int(rng.integers(0, 10)),
                          int(rng.integers(0, m))]
                for k in range(int(rng.integers(1, 4))):
                    x = places[(i // 4 + k) % 4] if k == 0 else \
                        places[int(rng.integers(0, 4))]
                    out[i, x] = H.WILDCARD
    return out.ravel()


def host_index(gi, n):
    t = gi.download()
    return H.Index(n, gi.info().prefixlength, 4, t["tis"], t["suf"],
                   t["lcp"], t["llv"], t["bck"], t["bwt"], None)


def wide_copy(V, host, monkeypatch):
    i = host.as_width(64)
    monkeypatch.setenv("VSA_FORCE_WIDE", "1")
    try:
        gi = V.Index.from_tables(i.n, i.prefixlength, 4, i.tis, i.suf, i.lcp,
                                 i.llv, i.bck, i.bwt)
    finally:
        monkeypatch.delenv("VSA_FORCE_WIDE")
    assert gi.info().device_integersize == 64
    return gi


MODES = [({}, 0), ({}, 2), (dict(mum=True, cand=True), 2),
         (dict(mum=True), 2)]


def check_all_modes(V, gis, host, sym, m, Ls, cache):
    """every index of gis, bytes and packed reads, -complete and the four
    -l modes at every L, == the oracle (computed once per (m, L, mode))"""
    hq = H.Queries.uniform(sym, m)
    nq = hq.nq
    forms = [V.Queries.from_host(sym, hq.start, hq.length),
             V.Queries.from_host_packed(sym, m)]
    assert forms[1].nq == nq
    key = (m, "complete")
    if key not in cache:
        cache[key] = H.oracle_complete(host, hq)
    for gi in gis:
        for gq in forms:
            assert np.array_equal(V.findcompletematches(gi, gq).fetch(),
                                  cache[key])
    for L in Ls:
        for kw, sp in MODES:
            key = (m, L, tuple(sorted(kw)), sp)
            if key not in cache:
                cache[key] = H.oracle_querymatches(host, hq, L, speedup=sp,
                                                   **kw)
            for gi in gis:
                for f, gq in zip(("bytes", "packed"), forms):
                    got = V.findquerymatches(gi, gq, L, speedup=sp,
                                             **kw).fetch()
                    assert np.array_equal(got, cache[key]), \
                        (m, L, kw, sp, f, gi.info().device_integersize)


@pytest.mark.parametrize("n", SIZES, ids=lambda n: "%dMbp" % (n // 10 ** 6))
def test_repeat_rich_text_at_its_own_deep_prefix(V, n, monkeypatch):
    """D = 13 (64 Mbp) and 14 (200 Mbp): buckets of thousands of suffixes
    (families, satellites), empty ones, wildcards in the first D symbols and
    in the key window; 32-bit and wide device tables"""
    tis = repeat_rich_text(n, 300 + n % 997)
    gi = V.Index.build(tis, 4, 0)
    D = gi.info().deepprefix
    want = 1
    while want < 16 and 4 ** want < n:
        want += 1
    assert D == want
    if n >= 60 * 10 ** 6:
        assert D in (13, 14)
    host = host_index(gi, n)
    host.sti1 = H.sti1_from_tables(host.suf, host.lcp, host.prefixlength)
    gis = [gi, wide_copy(V, host, monkeypatch)]
    assert gis[1].info().deepprefix == D
    rng = np.random.default_rng(310 + n % 991)
    cache = {}
    for m in (100, 150):
        sym = family_reads(rng, host.tis, 3000, m, D)
        check_all_modes(V, gis, host, sym, m, [D - 1, D, D + 1, 20, 40],
                        cache)
    for g in gis:
        g.close()


@pytest.mark.parametrize("seed", [0, 2])
def test_forced_deep_prefix_above_log4_n(V, seed, monkeypatch):
    """VSA_DEEP_PREFIX = 13..16 on the hard-batch texts of
    test_mum_work_plan_on_hard_batches (90 kbp: log4 n is about 8): nearly
    every bucket empty, the deep path taken at search lengths the text alone
    would never give it.  Reads with a wildcard at every offset 0, 12..25 join
    the hard batch (offset D - 1: the deep locate must step aside).  Each
    index is closed before the next (D = 16 holds about 100 GB of slot and
    bucket tables); the forced D must have been taken."""
    tis, qb, m, L0, nq = mum_hard_batch(seed)
    rng = np.random.default_rng(77 + seed)
    extra = np.zeros((600, m), np.uint8)
    for i in range(600):
        p = int(rng.integers(0, len(tis) - m))
        q = tis[p:p + m].copy()
        q[q == H.SEPARATOR] = H.WILDCARD
        w = [0] + list(range(12, 26))
        q[w[i % len(w)]] = H.WILDCARD
        extra[i] = q
    qb = np.concatenate([qb[:1500 * m], extra.ravel()])
    cache, host = {}, None
    for D in (13, 14, 15, 16):
        monkeypatch.setenv("VSA_DEEP_PREFIX", str(D))
        try:
            gi = V.Index.build(tis, 4, 0)
        finally:
            monkeypatch.delenv("VSA_DEEP_PREFIX")
        assert gi.info().deepprefix == D
        if host is None:
            host = host_index(gi, len(tis))
            host.sti1 = H.sti1_from_tables(host.suf, host.lcp,
                                           host.prefixlength)
        check_all_modes(V, [gi], host, qb, m,
                        sorted({D - 1, D, D + 1, max(L0, 20)}), cache)
        gi.close()

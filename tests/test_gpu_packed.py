"""Reads at two bits per symbol (vsa_pack_reads, vsa_queries_from_host_packed):
a packed batch must answer every engine call exactly like the byte batch of
the same reads -- -complete, -mum, -mum cand straight from the rows (first
pass, work plan, search kernel), MEM / approximate matching / the reverse
complement through the bytes made on the device -- including reads with
wildcards (side list), reads that end in a repeat (ties: the reference walk
through QSrc), 32- and 64-bit device tables.  Symbol map: the reference's DNA
map (kurtz-basic/alphabet.c:369); wildcard semantics kurtz/maxpref.c:30-41."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


def unpack(V, rows, special, nq, m):
    W = int(V.lib.vsa_packed_words(m))
    rows = rows.reshape(nq, W)
    out = np.zeros((nq, m), np.uint8)
    for j in range(m):
        out[:, j] = (rows[:, j // 32] >> np.uint64(62 - 2 * (j % 32))) & \
            np.uint64(3)
    flagged = np.flatnonzero(rows[:, W - 1] & np.uint64(0xFF))
    for i in flagged:
        k = int(rows[i, 0]) >> 8
        out[i] = special[k * m:(k + 1) * m]
    return out.ravel(), flagged


def gpu_index(V, idx, bits=32):
    i = idx.as_width(bits)
    return V.Index.from_tables(i.n, i.prefixlength, i.numofchars, i.tis,
                               i.suf, i.lcp, i.llv, i.bck, i.bwt,
                               i.querysepposition, i.hasqueries)


def both(V, sym, m):
    nq = len(sym) // m
    byte = V.Queries.from_host(sym, np.arange(nq, dtype=np.uint64) * m,
                               np.full(nq, m, np.uint64))
    packed = V.Queries.from_host_packed(sym, m)
    return byte, packed


@pytest.mark.parametrize("bits", [32, 64])
def test_packed_batch_reproduces_the_golden_lists(V, bits):
    idx, q = H.load_case("c1")
    m = int(q.length[0])
    assert (q.length == m).all() and (q.start == np.arange(q.nq) * m).all()
    gi = gpu_index(V, idx, bits)
    byte, packed = both(V, q.symbols, m)
    assert packed.info().numofqueries == q.nq
    got = H.matches_as_ref(idx, V.findcompletematches(gi, packed).fetch())
    assert np.array_equal(got, H.expected("c1", "complete"))
    for key, kw in (("mum20", dict(mum=True)),
                    ("mumcand20", dict(mum=True, cand=True)),
                    ("mem20_sp2", dict())):
        r = V.findquerymatches(gi, packed, 20, **kw)
        got = H.matches_as_ref(idx, r.fetch())
        assert np.array_equal(got, H.expected("c1", key)), key
        rb = V.findquerymatches(gi, byte, 20, **kw)
        sb, sp = rb.stats(), r.stats()
        assert (sb.count, sb.sumlength, sb.candidates) == \
            (sp.count, sp.sumlength, sp.candidates), key
        if kw:      # (MEM counts the plan's own locates by an upper bound)
            assert sb.searches == sp.searches, key
    # approximate matching and the reverse complement go through the bytes
    for key in sorted(H.manifest()["c1"]["runs"]):
        if key.startswith("approx_"):
            spec = key[len("approx_"):]
            doedist, k, pct = spec[0] == "e", int(spec[1:].rstrip("pb")), \
                1 if spec.endswith("p") else (2 if spec.endswith("b") else 0)
            got = V.findapproxcompletematches(gi, packed, doedist, k,
                                              pct).fetch()
            assert np.array_equal(H.matches_as_ref(idx, got),
                                  H.expected("c1", key)), key
    rc = packed.reverse_complement()
    rcb = byte.reverse_complement()
    assert np.array_equal(V.findquerymatches(gi, rc, 20).fetch(),
                          V.findquerymatches(gi, rcb, 20).fetch())


@pytest.mark.parametrize("seed", range(8))
def test_wildcards_repeats_and_short_reads_packed(V, seed):
    """reads with wildcards travel on the side list; reads cut from repeats
    tie on all key symbols (reference walk through QSrc); lengths that are no
    multiple of 4 or 32; a text with wildcards and separators; rows of more
    than four words (150 bp and longer: the first pass looks at them through
    windows) and of more than eight (expanded to bytes on the device)"""
    rng = np.random.default_rng(4200 + seed)
    m = [100, 37, 64, 121, 150, 200, 252, 253][seed]
    L = [20, 12, 16, 25, 20, 30, 18, 22][seed]
    unit = rng.integers(0, 4, 300).astype(np.uint8)
    t = rng.integers(0, 4, 60000).astype(np.uint8)
    for r in range(12):
        p = int(rng.integers(0, len(t) - 300))
        u = unit.copy()
        for e in range(int(rng.integers(0, 3))):
            u[int(rng.integers(0, 300))] = rng.integers(0, 4)
        t[p:p + 300] = u
    t[rng.random(len(t)) < 0.0004] = H.WILDCARD
    t[30000] = H.SEPARATOR
    idx = H.oracle_build_index(t, 4)
    idx.sti1 = H.sti1_from_tables(idx.suf, idx.lcp, idx.prefixlength)
    nq = 3000
    reads = np.zeros((nq, m), np.uint8)
    for i in range(nq):
        p = int(rng.integers(0, len(t) - m))
        reads[i] = t[p:p + m]
        if rng.random() < 0.3:
            reads[i, int(rng.integers(0, m))] = rng.integers(0, 4)
        if rng.random() < 0.1:
            reads[i, int(rng.integers(0, m))] = H.WILDCARD
    reads[reads == H.SEPARATOR] = H.WILDCARD
    sym = reads.ravel()
    rows, special, ns = V.pack_reads(sym, nq, m)
    back, flagged = unpack(V, rows, special, nq, m)
    assert np.array_equal(back, sym) and ns == len(flagged) > 0
    hq = H.Queries.uniform(sym, m)
    for bits in (32, 64):
        gi = gpu_index(V, idx, bits)
        byte, packed = both(V, sym, m)
        assert np.array_equal(V.findcompletematches(gi, packed).fetch(),
                              H.oracle_complete(idx, hq))
        for kw in (dict(mum=True), dict(mum=True, cand=True), dict()):
            got = V.findquerymatches(gi, packed, L, **kw).fetch()
            want = H.oracle_querymatches(idx, hq, L, speedup=2, **kw)
            assert np.array_equal(got, want), (seed, bits, kw)


def test_packed_reads_of_a_multiseq_with_separators(V):
    """stride m + 1: the reads of a reference Multiseq, separators between
    them (kurtz-basic/multiseq.c:129-166), packed where they lie"""
    idx, q = H.load_case("c1")
    m = int(q.length[0])
    nq = 500
    ms = np.full(nq * (m + 1), H.SEPARATOR, np.uint8)
    ms.reshape(nq, m + 1)[:, :m] = q.symbols[:nq * m].reshape(nq, m)
    gi = gpu_index(V, idx)
    packed = V.Queries.from_host_packed(ms[:-1], m, stride=m + 1)
    assert packed.nq == nq
    want = V.findquerymatches(
        gi, V.Queries.from_host(q.symbols[:nq * m], q.start[:nq],
                                q.length[:nq]), 20, mum=True).fetch()
    assert np.array_equal(V.findquerymatches(gi, packed, 20,
                                             mum=True).fetch(), want)
    # a flagged row that names no entry of the side list is refused
    rows, special, ns = V.pack_reads(q.symbols[:nq * m], nq, m)
    W = int(V.lib.vsa_packed_words(m))
    rows[5 * W + W - 1] |= np.uint64(1)
    rows[5 * W] = np.uint64(7)
    h = H.C.c_void_p()
    rc = V.lib.vsa_queries_from_host_packed(V._ptr(rows), nq, m,
                                            V._ptr(special), ns, 0,
                                            H.C.byref(h))
    assert rc == -2 and "side list" in V.messagespace()


# ---------------------------------------------------------------------------
# The MEM work plan (mem_workplan.inc) on batches built to exhaust it: the
# -l L counterpart of test_gpu_parity.py::test_mum_work_plan_on_hard_batches
# ---------------------------------------------------------------------------

def mem_hard_text(rng):
    """three sequences of random DNA with a family of 500-symbol units planted
    eight times each with 0..3 substitutions (stretches whose rep bits are
    set), one 700-symbol stretch planted twice exactly (matches of 255 symbols
    and more, which the plan cannot locate), wildcards -> (tis, unit starts,
    long-repeat start)"""
    unit = rng.integers(0, 4, 500).astype(np.uint8)
    long = rng.integers(0, 4, 700).astype(np.uint8)
    seqs, units = [], []
    off = 0
    for s in range(3):
        t = rng.integers(0, 4, 30000).astype(np.uint8)
        for r in range(8):
            p = 3600 * r + int(rng.integers(0, 3000))
            u = unit.copy()
            for e in range(int(rng.integers(0, 4))):
                u[int(rng.integers(0, len(u)))] = rng.integers(0, 4)
            t[p:p + len(u)] = u
            units.append(off + p)
        if s != 1:
            t[29000 - len(long):29000] = long
        t[rng.random(30000) < 0.0005] = H.WILDCARD
        seqs.append(t)
        off += 30001
    tis = np.concatenate([np.concatenate([s, [H.SEPARATOR]])
                          for s in seqs])[:-1].astype(np.uint8)
    return tis, np.array(units), 29000 - len(long)


def mem_hard_reads(rng, tis, units, longstart, lengths, D):
    """one read per entry of lengths, ten families: 7..12 substitutions (four
    of ten), exact copies, cut from a planted unit, cut from the long repeat,
    random, a deletion and an insertion, wildcards at offset 0, D - 1, inside
    the key window D .. D + 9 and at random"""
    reads = []
    for i, m in enumerate(lengths):
        m = int(m)
        kind = i % 10
        if kind == 5:
            p = int(units[i // 10 % len(units)]) + int(rng.integers(0, 100))
        elif kind == 6:
            p = longstart + int(rng.integers(0, 60))
        else:
            p = int(rng.integers(0, len(tis) - m - 2))
        q = tis[p:p + m + 1].copy()
        q[q == H.SEPARATOR] = rng.integers(0, 4)   # read across a boundary
        if kind < 4:
            for x in rng.choice(m, min(m, int(rng.integers(7, 13))),
                                replace=False):
                q[x] = (q[x] + 1 + rng.integers(0, 3)) % 4 if q[x] < 4 else 1
        elif kind == 7:
            q = rng.integers(0, 4, m + 1).astype(np.uint8)
        elif kind == 8 and m > 4:
            x, y = sorted(rng.choice(m - 1, 2, replace=False))
            q = np.concatenate([q[:x], q[x + 1:y], [rng.integers(0, 4)],
                                q[y:]]).astype(np.uint8)
        elif kind == 9 and m > 0:
            pos = [0, D - 1, D + int(rng.integers(0, 10)),
                   int(rng.integers(0, m))][i // 10 % 4]
            q[min(pos, m - 1)] = H.WILDCARD
            if i % 3 == 0:
                q[int(rng.integers(0, m))] = H.WILDCARD
        reads.append(q[:m])
    return reads


# (name, read length or None for ragged lengths, packed): every first-pass
# variant esa_search.hip picks for the MEM plan -- dense bytes staged in LDS
# (m <= 128, m % 4 == 0), unstaged bytes (m % 4 != 0, m > 128), ragged bytes,
# rows of up to four words, rows of five to eight words
MEM_VARIANTS = [("staged100", 100, False), ("odd102", 102, False),
                ("long300", 300, False), ("ragged", None, False),
                ("rows100", 100, True), ("rows150", 150, True),
                ("rows252", 252, True)]


@pytest.mark.parametrize("name,m,packed", MEM_VARIANTS,
                         ids=[v[0] for v in MEM_VARIANTS])
def test_mem_work_plan_on_hard_batches(V, name, m, packed, monkeypatch):
    """-l L on reads with 7..12 mismatches (the plan's rounds and ranges run
    out), repeats whose rep bits are set, matches of 255 symbols and more,
    wildcards where the deep locate must step aside; both -qspeedup
    algorithms against the oracle in order, and against the unplanned run
    (VSA_TUNE=2) of the same index.  L = 255 is the last search length with
    a plan, 256 the first without."""
    seed = [v[0] for v in MEM_VARIANTS].index(name)
    rng = np.random.default_rng(9100 + seed)
    tis, units, longstart = mem_hard_text(rng)
    idx = H.oracle_build_index(tis, 4)
    idx.sti1 = H.sti1_from_tables(idx.suf, idx.lcp, idx.prefixlength)
    gi = gpu_index(V, idx, 32)
    D = gi.info().deepprefix
    assert D >= idx.prefixlength and D > 0
    monkeypatch.setenv("VSA_TUNE", "2")
    plain = gpu_index(V, idx, 32)
    monkeypatch.delenv("VSA_TUNE")
    nq = 2000
    lengths = (rng.integers(0, 400, nq) if m is None else np.full(nq, m))
    if m is None:
        lengths[17] = 0
    reads = mem_hard_reads(rng, tis, units, longstart, lengths, D)
    # (uniform reads lie back to back: the dense batch the staged first pass
    # wants)
    hq = (H.Queries.from_list(reads) if m is None else
          H.Queries.uniform(np.concatenate(reads), m))
    if packed:
        gq = V.Queries.from_host_packed(hq.symbols, m)
        assert gq.nq == nq
    else:
        gq = V.Queries.from_host(hq.symbols, hq.start, hq.length)
    Ls = [D, 20, 31]
    if int(lengths.max()) >= 256:
        Ls += [255, 256]
    for L in Ls:
        full = int(np.maximum(hq.length.astype(np.int64) - L + 1, 0).sum())
        for sp in (0, 2):
            r = V.findquerymatches(gi, gq, L, speedup=sp)
            got = r.fetch()
            want = H.oracle_querymatches(idx, hq, L, speedup=sp)
            assert np.array_equal(got, want), (name, L, sp)
            u = V.findquerymatches(plain, gq, L, speedup=sp)
            assert np.array_equal(u.fetch(), want), (name, L, sp)
            assert u.stats().kernel_searches == full
            assert r.stats().kernel_searches <= full
        if L == 20:
            assert len(want) > nq // 2
            assert (want["length"] >= 255).any() == (m is None or m >= 255)


def test_mem_rep_bits_follow_the_search_length(V):
    """the rep-bit table is kept per (index, L) (index->repleast): changing L
    on one index, back and forth and through -mum, must rebuild it"""
    rng = np.random.default_rng(9200)
    tis, units, longstart = mem_hard_text(rng)
    idx = H.oracle_build_index(tis, 4)
    gi = gpu_index(V, idx, 32)
    m, nq = 100, 2000
    reads = mem_hard_reads(rng, tis, units, longstart, np.full(nq, m),
                           gi.info().deepprefix)
    hq = H.Queries.uniform(np.concatenate(reads), m)
    gq = V.Queries.from_host(hq.symbols, hq.start, hq.length)
    for L, kw in ((20, {}), (25, {}), (20, {}), (20, dict(mum=True)),
                  (20, {}), (21, {})):
        got = V.findquerymatches(gi, gq, L, speedup=0, **kw).fetch()
        assert np.array_equal(got, H.oracle_querymatches(idx, hq, L,
                                                         speedup=0, **kw)), \
            (L, kw)


def test_empty_packed_batch(V):
    """Queries.from_host_packed of no reads: every entry point answers with
    an empty list (the bytes of an empty packed batch were sized by a
    division by its read length, 0)"""
    idx, q = H.load_case("c1")
    gi = gpu_index(V, idx, 32)
    for m in (100, 150):
        empty = V.Queries.from_host_packed(np.zeros(0, np.uint8), m)
        assert empty.nq == 0 and empty.info().numofqueries == 0
        assert V.findcompletematches(gi, empty).count == 0
        for kw in (dict(speedup=0), dict(speedup=2), dict(mum=True),
                   dict(mum=True, cand=True)):
            assert V.findquerymatches(gi, empty, 20, **kw).count == 0, kw
        assert V.findapproxcompletematches(gi, empty, True, 2).count == 0
        assert V.findapproxcompletematches(gi, empty, False, 1).count == 0
        rc = empty.reverse_complement()
        assert rc.info().numofqueries == 0
        assert V.findcompletematches(gi, rc).count == 0
        assert V.findquerymatches(gi, rc, 20).count == 0
        assert V.findmumcandidates_packed(gi, empty, 20).count == 0
        assert V.findmumcandidates_packed(gi, empty, 20, 8).count == 0
        # and the index still answers a real batch afterwards
        got = V.findcompletematches(gi, V.Queries.from_host_packed(
            q.symbols, int(q.length[0]))).fetch()
        assert np.array_equal(H.matches_as_ref(idx, got),
                              H.expected("c1", "complete"))

"""The edges of the driver of the scan without an index, without a GPU: the
host code at 1, 3 and 16 threads against the literal model on the texts that
test_gpu_online_edges.py scans on the device -- borders of the workgroups of
the edit scan, batches of more reads than a group, dense hits, tiny texts --;
each of those texts shown to hold what it was made for, on the model's list;
and the plan of the driver (vsa_online_plan: tile, tiles, queries per chunk,
chunks) at its defaults, under both hooks of the environment and at its
caps."""
import numpy as np
import pytest

import online_cases as OC
import online_model as OM

THREADS = (1, 3, 16)
# thresholds of a tiny text that only the host code takes under -e: not below
# the read of one symbol
TINY_HOST_KS = ((1, False), (2, False))

_compared = {"cases": 0, "records": 0}


def host(V, edge, mode, K, percent, remred, threads, offset=0):
    q = edge.queries()
    return V.findcompletematches_online_host(
        edge.text, q.symbols, q.start, q.length, mode=mode, distvalue=K,
        percent=percent, removeredundant=remred, offset=offset,
        threads=threads)


def agree(V, edge, Ks=None):
    total = 0
    for K, percent in edge.Ks if Ks is None else Ks:
        for mode, remred in OC.MODES:
            want = OC.model(edge, mode, K, percent, remred, offset=7)
            for threads in THREADS:
                got = host(V, edge, mode, K, percent, remred, threads, 7)
                assert np.array_equal(got, want), (edge.name, mode, K,
                                                   percent, remred, threads)
            total += len(want)
            _compared["cases"] += 1
            _compared["records"] += len(want) * len(THREADS)
    return total


def starts(edge, mode, K, percent=False, remred=False, read=None):
    rec = OC.model(edge, mode, K, percent, remred)
    if read is not None:
        rec = rec[rec["queryseq"] == read]
    return rec["dbstart"].astype(np.int64)


@pytest.mark.parametrize("tile", (64, None))
def test_workgroup_borders(V, tile):
    T = tile or OC.H_TILE
    border = T * OC.WG_TILES
    for edge in OC.wg_edges(tile):
        n, p = len(edge.text), edge.planted
        assert p["border"] == border and agree(V, edge) > 0
        # the deletion: -e alone finds it
        assert p["indel"] in starts(edge, OC.EDIST, OC.WG_K, read=1)
        for mode in (OC.EXACT, OC.HAMMING):
            assert p["indel"] not in starts(edge, mode, OC.WG_K, read=1)
        nosep = not (edge.text[border - 2:border + 1] == OC.SEP).any() \
            if n > border else True
        for i, a in enumerate(p["starts"]):
            m = OC.WG_LENGTHS[i]
            assert a + m <= n
            # the window the read was cut from: there unless a separator
            # was put into it
            whole = np.array_equal(edge.text[a:a + m], edge.reads[i])
            assert whole or not nosep
            for mode, remred in OC.MODES:
                found = a in starts(edge, mode, OC.WG_K, remred=remred,
                                    read=i)
                assert found or not whole
                assert whole or not found or mode == OC.EDIST
        if n > border + 8 and nosep:
            # a start on both sides of the border, one exactly on it, and a
            # match that lies across it
            s = starts(edge, OC.HAMMING, OC.WG_K)
            assert (s < border).any() and (s >= border).any()
            assert any(a < border < a + m for a, m in
                       zip(p["starts"], OC.WG_LENGTHS))
        if "onborder" in p:
            i, a = p["onborder"]
            assert edge.text[a - 1] == OC.SEP and a in (border, border + 1)
            assert edge.text[a + OC.WG_LENGTHS[i] + OC.WG_K] == OC.SEP
            for mode, remred in OC.MODES:
                assert a in starts(edge, mode, OC.WG_K, remred=remred, read=i)
    # between them: a read that starts on the border, at border - 1, at
    # border - m / 2 and at border - m + 1; texts that end one before, on and
    # one behind the border
    offs = {(border - a, m) for e in OC.wg_edges(tile)
            if len(e.text) > border + 8
            for a, m in zip(e.planted["starts"], OC.WG_LENGTHS)}
    assert {o for o, _ in offs} >= {0, 1} and \
        any(o == m // 2 for o, m in offs) and any(o == m - 1 for o, m in offs)
    if tile == 64:
        assert {len(e.text) - border for e in OC.wg_edges(tile)} >= {-1, 0, 1}


@pytest.mark.parametrize("nq", OC.GROUP_NQ)
def test_batches_of_more_reads_than_a_group(V, nq):
    edge = OC.groups_edge(nq)
    assert len(edge.reads) == nq and agree(V, edge) > 1000
    # K = 0 as a number: exact and -h on the whole batch (-e with a fixed K
    # needs reads of 2 symbols and more)
    for mode in (OC.EXACT, OC.HAMMING):
        want = OC.model(edge, mode, 0)
        assert np.array_equal(host(V, edge, mode, 0, False, False, 3), want)
    lengths = [len(q) for q in edge.reads]
    assert set(lengths) >= set(OC.GROUP_LENGTHS) - {lengths[OC.GROUP_EMPTY]} \
        or nq < 32
    for K, percent in edge.Ks:
        # k = 0 and k > 0 in one percent batch, in one instantiation (W = 8)
        ks = {OM.threshold_of(m, K, percent) for m in lengths if m}
        assert 0 in ks and max(ks) > 0 and max(lengths) == 300
        for mode, remred in OC.MODES:
            rec = OC.model(edge, mode, K, percent, remred)
            seen = set(rec["queryseq"].tolist())
            # (a planted read of more than 12 symbols has a substitution)
            assert {i for i in edge.planted["planted"]
                    if mode != OC.EXACT or lengths[i] <= 12} <= seen
            # the read without a symbol yields nothing
            assert lengths[OC.GROUP_EMPTY] == 0 and \
                OC.GROUP_EMPTY not in seen
            # a full group of 32 reads without a hit
            if nq == 97:
                assert edge.planted["silent"] == tuple(range(64, 96))
            assert not seen & set(edge.planted["silent"])
            # a wildcard facing a wildcard: equal under -h, and under -e
            # beyond 64 symbols only
            for i, a in edge.planted["facing"].items():
                at = rec[(rec["queryseq"] == i) & (rec["dbstart"] == a)]
                assert len(at) == (mode != OC.EXACT) or remred
                if len(at):
                    # (the longest match counts it for every m)
                    assert at["querystart"][0] == (mode == OC.EDIST)
    if nq == 33:
        # 1 percent: threshold 0 up to 99 symbols
        rec = OC.model(edge, OC.EDIST, *OC.GROUP_K0)
        for i, a in edge.planted["facing"].items():
            assert (a in rec["dbstart"][rec["queryseq"] == i]) == \
                (lengths[i] > 64)
        assert agree(V, edge, [OC.GROUP_K0]) > 0


def test_a_batch_with_a_read_of_512_symbols(V):
    edge = OC.groups_edge(33, 512)
    assert max(len(q) for q in edge.reads) == 512
    assert agree(V, edge, edge.Ks[1:2]) > 1000


def test_batches_whose_hits_lie_in_few_reads(V):
    for edge in (OC.groups_edge(97, hitters=(40, 45)),
                 OC.groups_edge(97, hitters=(0, 96)),
                 OC.groups_edge(33, hitters=(15, 16)),
                 OC.groups_edge(33, hitters=(0, 32))):
        assert agree(V, edge, edge.Ks[:1]) > 0
        for mode, remred in OC.MODES:
            rec = OC.model(edge, mode, 5, True, remred)
            assert set(rec["queryseq"].tolist()) <= \
                set(edge.planted["planted"])
    for nq in (33, 97):
        edge = OC.uniform_edge(nq)
        assert agree(V, edge) > 0 and \
            len({len(q) for q in edge.reads}) == 1
        assert OC.WILD in edge.reads[1]


@pytest.mark.parametrize("kind", OC.DENSE_KINDS)
def test_dense_hits(V, kind):
    for n in OC.DENSE_SIZES:
        edge = OC.dense_edge(kind, n)
        assert agree(V, edge) > 10 * n
        assert OM.threshold_of(66, *OC.DENSE_KS[0]) == 0
        plain = OC.model(edge, OC.EDIST, 1)
        pos = plain["dbstart"][plain["queryseq"] == 1].astype(np.int64)
        # a run of adjacent start positions over more than 10 tiles of 64
        # symbols, and of the default
        run = best = 1
        for a, b in zip(pos[:-1], pos[1:]):
            run = run + 1 if a - b == 1 else 1
            best = max(best, run)
        assert best > 10 * 64 and (n < 4200 or kind == "period3sep" or
                                   best > 10 * OC.H_TILE)
        info = {}
        rem = OM.findcompletematches(edge.text, edge.reads, OC.EDIST, 1, False,
                                     True, info=info)
        assert info["dropped"] > n // 2 and len(rem) < len(plain)
        if kind == "homopolymer":
            # a (query, window tile) pair in which every start position hits
            for mode in (OC.EXACT, OC.HAMMING):
                rec = OC.model(edge, mode, 1, mode == OC.EXACT)
                first = rec[(rec["queryseq"] == 0) &
                            (rec["dbstart"] < OC.WTILE)]
                assert (len(first) == OC.WTILE) == (n >= OC.WTILE + 3)
        # the read out of phase: one hit in two under exact, none in a
        # homopolymer
        rec = OC.model(edge, OC.EXACT, 1, True)
        out = rec[rec["queryseq"] == 4]
        assert (len(out) == 0) == (kind == "homopolymer")


@pytest.mark.parametrize("n", OC.TINY_SIZES)
def test_tiny_texts(V, n):
    longer = 0
    for sep in (False, True):
        edge = OC.tiny_edge(n, sep)
        agree(V, edge)
        agree(V, edge, TINY_HOST_KS)
        assert len(edge.text) == n and \
            (edge.text == OC.SEP).sum() == int(sep)
        for K, percent in edge.Ks + list(TINY_HOST_KS):
            for remred in (False, True):
                rec = OC.model(edge, OC.EDIST, K, percent, remred)
                for q in set(rec["queryseq"].tolist()):
                    m = len(edge.reads[q])
                    k = OM.threshold_of(m, K, percent)
                    assert m - k <= n
                    longer += m > n
            for mode in (OC.EXACT, OC.HAMMING):
                rec = OC.model(edge, mode, K, percent)
                assert all(len(edge.reads[q]) <= n
                           for q in rec["queryseq"].tolist())
        # the foreign symbol occurs nowhere
        assert len(edge.reads[-1]) == 1 and all(
            len(edge.reads) - 1 not in
            OC.model(edge, mode, 0, False, r)["queryseq"]
            for mode, r in OC.MODES)
    # a match found only because m - k <= n < m
    assert longer > 0
    for K, percent in OC.TINY_KS[1:]:
        rec = OC.model(OC.tiny_edge(n), OC.EDIST, K, percent)
        assert n < 7 and percent and K < 50 or \
            any(len(OC.tiny_edge(n).reads[q]) > n
                for q in rec["queryseq"].tolist())


def test_the_empty_text_and_the_empty_batch(V):
    for edge in OC.empty_edges():
        assert len(edge.text) == 0 or len(edge.reads) == 0
        assert agree(V, edge) == 0


def test_the_plan_of_the_driver(V, monkeypatch):
    monkeypatch.delenv("VSA_ONLINE_TILE", raising=False)
    monkeypatch.delenv("VSA_ONLINE_COUNTERS", raising=False)
    E, X, Hm = OC.EDIST, OC.EXACT, OC.HAMMING
    C = V.ONLINE_COUNTERS_DEFAULT
    assert C == 1 << 26 and OC.H_TILE == 296 and OC.WTILE == 2048
    # the defaults
    assert V.online_plan(3000, 97, E) == (296, 11, 2097120, 1)
    assert V.online_plan(3000, 97, X) == (2048, 2, 2097120, 1)
    assert V.online_plan(3000, 97, Hm) == (2048, 2, 2097120, 1)
    assert V.online_plan(296 * 128 + 600, 3, E) == (296, 131, C // 131, 1)
    assert V.online_plan(296, 1, E)[1] == 1 and \
        V.online_plan(297, 1, E)[1] == 2
    assert V.online_plan(2048, 1, Hm)[1] == 1 and \
        V.online_plan(2049, 1, Hm)[1] == 2
    p = V.online_plan(1 << 20, 19000, E)
    assert p.tile == 296 and p.ntiles == 3543 and \
        p.queries_per_chunk == 18941 and p.numofchunks == 2
    # the tile hook: a multiple of 8 from 64 to the default, for -e only
    for value, tile in (("64", 64), ("256", 256), ("100", 96), ("296", 296),
                        ("63", 296), ("297", 296), ("0", 296), ("", 296),
                        ("x", 296), ("-64", 296)):
        monkeypatch.setenv("VSA_ONLINE_TILE", value)
        p = V.online_plan(8193, 3, E)
        assert p.tile == tile and p.ntiles == -(-8193 // tile)
        assert V.online_plan(8193, 3, X)[:2] == (2048, 5)
    monkeypatch.setenv("VSA_ONLINE_TILE", "64")
    assert V.online_plan(8192, 3, E).ntiles == 128 and \
        V.online_plan(8193, 3, E).ntiles == 129
    # the counters hook: from 1 to the default
    for value, counters in (("1", 1), ("47", 47), ("94", 94),
                            (str(C), C), (str(C + 1), C), ("0", C),
                            ("-5", C), ("", C), ("many", C),
                            (str(1 << 40), C)):
        monkeypatch.setenv("VSA_ONLINE_COUNTERS", value)
        p = V.online_plan(3000, 97, E)
        step = min(max(1, counters // 47), 2097120)
        assert p == (64, 47, step, -(-97 // step)), value
    monkeypatch.setenv("VSA_ONLINE_COUNTERS", "94")
    assert V.online_plan(3000, 97, E)[2:] == (2, 49)
    assert V.online_plan(3000, 97, Hm)[2:] == (47, 3)
    monkeypatch.delenv("VSA_ONLINE_TILE")
    monkeypatch.delenv("VSA_ONLINE_COUNTERS")
    # more tiles than counters: one query per chunk
    for mode in (E, X, Hm):
        p = V.online_plan(1 << 40, 5, mode)
        assert p.ntiles == -(-(1 << 40) // p.tile) > C
        assert p.queries_per_chunk == 1 and p.numofchunks == 5
    # the y dimension of a grid: 65535 groups of 32 queries
    for mode in (E, X, Hm):
        p = V.online_plan(100, 3000000, mode)
        assert p.ntiles == 1 and p.queries_per_chunk == 2097120 == \
            65535 * OC.GROUP and p.numofchunks == 2
    assert V.online_plan(100, 2097120, E).numofchunks == 1
    assert V.online_plan(100, 2097121, E).numofchunks == 2
    # nothing to scan
    for mode in (E, X, Hm):
        assert V.online_plan(0, 5, mode)[1:] == (0, 2097120, 0)
        assert V.online_plan(100, 0, mode)[1:] == (1, 2097120, 0)
    for mode in (-1, 3):
        with pytest.raises(V.VsaError) as e:
            V.online_plan(100, 1, mode)
        assert e.value.code == -2 and "mode %d" % mode in e.value.message


def test_how_much_was_compared():
    """(the figures of profiles/r25; runs last in this module)"""
    print("host cases %(cases)d, records %(records)d" % _compared)
    assert _compared["cases"] > 0

"""The scan without an index on the device at the edges of its driver
(vstree_amd/csrc/online.hip), on the texts of online_cases.py that
test_online_edges_host.py shows to hold what they were made for: the borders
of the workgroups of the edit scan (128 tiles), batches of more reads than a
group of 32 with a partial last group, a group of one and a group without a
hit, the loop over chunks of queries (VSA_ONLINE_COUNTERS) with its
concatenation, its single-chunk shortcut and its release of the chunks,
dense hits (every lane of a window tile in every round, every position of an
edit tile, runs of start positions over many tiles), and tiny texts down to
one symbol, the empty text and the empty batch.

Every list is compared with the literal model for equality, order included,
and every scan asserts the four counters of its stats: count and sumlength
of the model's list, candidates = the model's start positions before remred,
searches = the distinct (query, tile) pairs they lie in.  What a test claims
to cross -- workgroups, groups, chunks -- it asserts on V.online_plan, the
arithmetic the driver itself uses.

A packed batch holds reads of one length: the batches of mixed lengths run
as ragged ones, the packed, uniform and dense forms on uniform_edge."""
import gc

import numpy as np
import pytest

import batch_forms as BF
import online_cases as OC
from test_gpu_online import index_of, settile

pytestmark = pytest.mark.gpu

BIG = (1 << 32) + 5
compared = {"scans": 0, "records": 0}


def plan_of(V, edge, mode):
    return V.online_plan(len(edge.text), len(edge.reads), mode)


def check(V, edge, where, gq, mode, K, percent, remred, tile, offset=0):
    """one scan under the hooks as they are set: the list and the stats"""
    res = V.findcompletematches_online(where, gq, mode, K, percent, remred)
    got, st = res.fetch(), res.stats()
    want = OC.model(edge, mode, K, percent, remred, offset=offset)
    what = (edge.name, mode, K, percent, remred, tile, offset)
    assert np.array_equal(got, want), what
    candidates, searches = OC.expected_stats(edge, mode, K, percent, tile)
    assert (st.count, st.sumlength, st.candidates, st.searches) == \
        (len(want), int(want["length"].sum()), candidates, searches), what
    compared["scans"] += 1
    compared["records"] += len(want)
    return got


def ragged(V, edge, offset=0):
    q = edge.queries()
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    if offset:
        gq.set_offset(offset)
    return gq


def sweep(V, monkeypatch, edge, places, gq, tiles, Ks=None, offset=0):
    """every threshold of the edge in every mode it goes with, on every
    place, with every tile"""
    total = 0
    for K, percent in edge.Ks if Ks is None else Ks:
        for mode, remred in OC.modes_of(edge, K, percent):
            for tile in tiles:
                settile(monkeypatch, tile)
                for where in places:
                    total += len(check(V, edge, where, gq, mode, K, percent,
                                       remred, tile, offset))
    return total


# ---- workgroups of the edit scan ------------------------------------------------

WORKGROUPS = {8191: 1, 8192: 1, 8193: 2, 8192 + 67: 2, 2 * 8192 + 5: 3,
              OC.H_TILE * OC.WG_TILES + 600: 2}


@pytest.mark.parametrize("tile", (64, None))
def test_occurrences_and_separators_at_workgroup_borders(V, monkeypatch,
                                                         tile):
    OC.setcounters(monkeypatch, None)
    for edge in OC.wg_edges(tile):
        n = len(edge.text)
        settile(monkeypatch, tile)
        p = plan_of(V, edge, OC.EDIST)
        assert p.tile == (tile or OC.H_TILE) and p.numofchunks == 1
        assert -(-p.ntiles // OC.WG_TILES) == WORKGROUPS[n]
        assert (p.ntiles > OC.WG_TILES) == (n > edge.planted["border"])
        places = (V.Text.from_host(edge.text),
                  index_of(V, edge.name, edge.text))
        assert sweep(V, monkeypatch, edge, places, ragged(V, edge),
                     (tile,)) > 0
    assert max(len(e.text) for e in OC.wg_edges(None)) == 38488


# ---- groups of queries ----------------------------------------------------------

@pytest.mark.parametrize("nq", OC.GROUP_NQ)
def test_batches_of_more_reads_than_a_group(V, monkeypatch, nq):
    OC.setcounters(monkeypatch, None)
    edge = OC.groups_edge(nq)
    groups = -(-nq // OC.GROUP)
    for mode in (OC.EXACT, OC.EDIST, OC.HAMMING):
        p = plan_of(V, edge, mode)
        assert p.numofchunks == 1 and p.queries_per_chunk >= nq
    assert groups == {31: 1, 32: 1, 33: 2, 65: 3, 97: 4}[nq]
    gt = V.Text.from_host(edge.text)
    Ks = edge.Ks + ([OC.GROUP_K0] if nq == 33 else [])
    for offset in (0, BIG):
        gq = ragged(V, edge, offset)
        assert sweep(V, monkeypatch, edge, (gt,), gq, (64, None), Ks,
                     offset) > 1000
        # K = 0 as a number: -e refuses it next to reads of one symbol
        for mode in (OC.EXACT, OC.HAMMING):
            for tile in (64, None):
                settile(monkeypatch, tile)
                check(V, edge, gt, gq, mode, 0, False, False, tile, offset)
        with pytest.raises(V.VsaError) as e:
            V.findcompletematches_online(gt, gq, OC.EDIST, 0)
        assert e.value.code == V.NOT_COVERED


def test_a_batch_with_a_read_of_512_symbols(V, monkeypatch):
    OC.setcounters(monkeypatch, None)
    edge = OC.groups_edge(33, 512)
    gt = V.Text.from_host(edge.text)
    assert sweep(V, monkeypatch, edge, (gt,), ragged(V, edge), (64, None),
                 edge.Ks[1:2]) > 1000


# ---- chunks of queries ----------------------------------------------------------

def chunked(V, monkeypatch, edge, gq, step, K, percent, offset=0, tile=64,
            least=3):
    """all four scans with `step` queries per chunk, asserted on the plan;
    each list against the model and against the call without the hook"""
    gt = V.Text.from_host(edge.text)
    nq = len(edge.reads)
    for mode, remred in OC.modes_of(edge, K, percent):
        settile(monkeypatch, tile)
        OC.setcounters(monkeypatch, None)
        whole = plan_of(V, edge, mode)
        assert whole.numofchunks == 1
        plain = check(V, edge, gt, gq, mode, K, percent, remred, tile, offset)
        OC.setcounters(monkeypatch, step * whole.ntiles)
        p = plan_of(V, edge, mode)
        assert p.ntiles == whole.ntiles and p.queries_per_chunk == step
        assert p.numofchunks == -(-nq // step) >= least
        got = check(V, edge, gt, gq, mode, K, percent, remred, tile, offset)
        assert np.array_equal(got, plain)
    OC.setcounters(monkeypatch, None)


@pytest.mark.parametrize("step", (1, 2, 31, 32, 33))
def test_chunks_of_queries(V, monkeypatch, step):
    edge = OC.groups_edge(97)
    K, percent = edge.Ks[1]
    chunked(V, monkeypatch, edge, ragged(V, edge), step, K, percent)
    chunked(V, monkeypatch, edge, ragged(V, edge, BIG), step, K, percent,
            BIG, tile=None)
    edge = OC.groups_edge(33)
    chunked(V, monkeypatch, edge, ragged(V, edge), step, K, percent,
            least={1: 33, 2: 17, 31: 2, 32: 2, 33: 1}[step])


def test_hits_in_one_chunk_of_several_and_in_the_outer_ones(V, monkeypatch):
    for nq, step, hitters, inchunks in (
            (97, 32, (40, 45), {1}), (97, 32, (0, 96), {0, 3}),
            (33, 2, (15, 16), {7, 8}), (33, 2, (14, 15), {7}),
            (33, 1, (16,), {16}), (33, 32, (0, 32), {0, 1})):
        edge = OC.groups_edge(nq, hitters=hitters)
        K, percent = edge.Ks[0]
        for mode, remred in OC.MODES:
            rec = OC.model(edge, mode, K, percent, remred)
            # (a planted read of more than 12 symbols has a substitution)
            seen = {int(q) // step for q in rec["queryseq"]}
            assert seen <= inchunks and (seen == inchunks or
                                         mode == OC.EXACT)
        chunked(V, monkeypatch, edge, ragged(V, edge), step, K, percent,
                least=2)


@pytest.mark.parametrize("form", ("uniform", "packed", "dense"))
def test_chunks_of_the_forms_addressed_by_query_number(V, monkeypatch, form):
    edge = OC.uniform_edge(97)
    K, percent = edge.Ks[0]
    q = edge.queries()
    for offset in (0, BIG):
        gq = BF.device_batch(V, q, form, offset)
        for step in (1, 32, 33):
            chunked(V, monkeypatch, edge, gq, step, K, percent, offset)


def test_chunks_are_released(V, monkeypatch):
    edge = OC.groups_edge(97)
    K, percent = edge.Ks[1]
    gq = ragged(V, edge)
    gt = V.Text.from_host(edge.text)
    settile(monkeypatch, 64)
    for mode, remred in OC.MODES:
        ntiles = plan_of(V, edge, mode).ntiles
        OC.setcounters(monkeypatch, 2 * ntiles)
        assert plan_of(V, edge, mode).numofchunks == 49
        check(V, edge, gt, gq, mode, K, percent, remred, 64)   # warms up
        gc.collect()
        free = []
        for _ in range(2):
            check(V, edge, gt, gq, mode, K, percent, remred, 64)
            gc.collect()
            free.append(V.device_meminfo()[0])
        # (memory a chunk kept would lower the figure from call to call)
        assert free[1] >= free[0], (mode, remred, free)


# ---- dense hits -----------------------------------------------------------------

@pytest.mark.parametrize("n", OC.DENSE_SIZES)
@pytest.mark.parametrize("kind", OC.DENSE_KINDS)
def test_dense_hits(V, monkeypatch, kind, n):
    OC.setcounters(monkeypatch, None)
    edge = OC.dense_edge(kind, n)
    gt = V.Text.from_host(edge.text)
    assert sweep(V, monkeypatch, edge, (gt,), ragged(V, edge),
                 (64, 256, None)) > 10 * n
    if kind == "homopolymer" and n > OC.WTILE + 3:
        # every lane of a window tile in every round
        candidates, searches = OC.expected_stats(edge, OC.HAMMING, 3, False,
                                                 None)
        assert candidates >= 4 * OC.WTILE and searches == 4 * 3


# ---- tiny texts -----------------------------------------------------------------

def from_device(V, text):
    d = V.device_malloc(max(1, len(text)))
    try:
        if len(text):
            V.device_upload(d, text)
        return V.Text.from_device(d, len(text))
    finally:
        V.device_free(d)


@pytest.mark.parametrize("n", OC.TINY_SIZES)
def test_tiny_texts(V, monkeypatch, n):
    OC.setcounters(monkeypatch, None)
    for sep in (False, True):
        edge = OC.tiny_edge(n, sep)
        settile(monkeypatch, 64)
        for mode in (OC.EXACT, OC.EDIST):
            assert plan_of(V, edge, mode).ntiles == (2 if n == 65 and
                                                     mode == OC.EDIST else 1)
        places = (V.Text.from_host(edge.text), from_device(V, edge.text),
                  index_of(V, edge.name, edge.text))
        total = sweep(V, monkeypatch, edge, places, ragged(V, edge),
                      (64, None))
        assert total > 0 or (sep and n == 1)
        # -e with a fixed K that is not below the read of one symbol
        for where in places:
            with pytest.raises(V.VsaError) as e:
                V.findcompletematches_online(where, ragged(V, edge),
                                             OC.EDIST, 1)
            assert e.value.code == V.NOT_COVERED


def test_the_empty_text_and_the_empty_batch(V, monkeypatch):
    OC.setcounters(monkeypatch, None)
    for edge in OC.empty_edges():
        for mode in (OC.EXACT, OC.EDIST, OC.HAMMING):
            assert plan_of(V, edge, mode).numofchunks == 0
        q = edge.queries()
        gq = V.Queries.from_host(q.symbols, q.start, q.length)
        places = (V.Text.from_host(edge.text), from_device(V, edge.text),
                  index_of(V, edge.name, edge.text))
        for K, percent in edge.Ks:
            for mode, remred in OC.MODES:
                for tile in (64, None):
                    settile(monkeypatch, tile)
                    for where in places:
                        got = check(V, edge, where, gq, mode, K, percent,
                                    remred, tile)
                        assert len(got) == 0


def test_how_much_was_compared():
    """(the figures of profiles/r25; runs last in this module)"""
    print("device scans %(scans)d, records %(records)d" % compared)
    assert compared["scans"] > 0

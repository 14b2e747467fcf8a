"""Match clustering on the GPU (vsa_matchcluster_*): the recorded runs of the
real reference on the at1MB and micro indexes, built and searched on the GPU,
with the cluster files formatted from the device's own records and edges; and
the kernels against the pure-Python model (matchcluster_model.py) and
vsa_matchcluster_host on hand-made lists, self lists over one sequence and
one list against queries with a palindromic pass -- the
smallest shapes at which a window, a tie, a tile of the compaction, a pass
of the candidate slots or a round of the forest can go wrong.  Overlap
values are compared as bit patterns."""
import os

import numpy as np
import pytest

import helpers as H
import cluster_model as CM
import matchcluster_cases as MC
import matchcluster_model as MM
from test_gpu_cluster import at1mb, engine_list

pytestmark = pytest.mark.gpu

FAR = 500000  # where the references that shall meet nothing live


def compare(mc, want, rec, pal=None):
    """a finished clustering against what the model says of the list rec
    (pal: its D/P flags)"""
    st = mc.stats().asdict()
    rounds = st.pop("rounds")
    wst = dict(want["stats"])
    wst.pop("rounds")
    assert st == wst
    assert (rounds == 0) == (wst["edges"] == 0) and rounds <= 13
    start, mem = mc.members()
    assert np.array_equal(start, want["clusterstart"])
    assert np.array_equal(mem, want["members"])
    assert np.array_equal(mc.labels(), want["labels"])
    assert mc.format() == want["text"]
    estart, m0, m1, values = mc.edges()
    assert np.array_equal(estart, want["edgestart"])
    assert np.array_equal(m0, want["m0"])
    assert np.array_equal(m1, want["m1"])
    assert np.array_equal(values, want["values"])
    res, flags = mc.records()
    who = want["members"].astype(np.int64)
    assert np.array_equal(res.fetch(), rec[who])
    assert np.array_equal(flags, np.zeros(len(who), np.uint8) if pal is None
                          else np.asarray(pal, np.uint8)[who])


def run(V, rec, mode, value, parts=1):
    """the list through the device (in `parts` add calls), the model and the
    host code"""
    layout = MC.synthetic_layout(V)
    mc = V.MatchCluster(layout, mode, value)
    for part in np.array_split(rec, parts):
        mc.add(V.Result.from_host(part))
    mc.finish()
    want = MC.model(rec, mode, value)
    compare(mc, want, rec)
    host = V.matchcluster_host(layout, mode, value, rec)
    for k in ("clusterstart", "members", "labels", "edgestart", "m0", "m1",
              "values"):
        assert np.array_equal(host[k], want[k]), k
    return mc, want


def isolated(n, first=0):
    """second references that meet nothing: far away, 1000 apart"""
    return FAR + 1000 * (first + np.arange(n))


# --------------------------------------------------------------------------
# the recorded runs through the engine
# --------------------------------------------------------------------------

def rc_of(q):
    """the reverse complements of a query set, sequence by sequence"""
    sym = q.symbols.copy()
    for s, l in zip(q.start, q.length):
        s, l = int(s), int(l)
        seg = q.symbols[s:s + l][::-1]
        sym[s:s + l] = np.where(seg == H.WILDCARD, H.WILDCARD, 3 - seg)
    return sym


def engine_passes(V, r, rec, flags):
    """the lists of the real entry points for the passes of a run against
    queries -> [(list in HBM, palindromic)], in the reference's order of the
    passes and, within a pass, of its records.  The engine finds the same
    matches in an order of its own; the number of a match is its place in
    the reference's buffer, so the records go up in that order once they are
    known to be the engine's."""
    srt = H.sorted_matches
    if r["query"] is not None:
        tis, ssp = MC.db_text(r)
        gi = V.Index.build(tis, 4, H.recommended_prefixlength(4, len(tis)), 0)
        q = H.fasta_queries(os.path.join(H.GOLDEN, r["query"]))
        for f in sorted(set(flags.tolist())):
            sym = rc_of(q) if f else q.symbols
            found = V.findquerymatches(
                gi, V.Queries.from_host(sym, q.start, q.length), r["L"])
            assert np.array_equal(srt(found.fetch()), srt(rec[flags == f]))
    else:
        # -d -p IDX: the self list as records against the index's own
        # sequences; of two mirror images of the P pass one was printed
        qstart, _, _ = MC.query_set(r)
        d = rec[flags == 0].copy()
        d["queryseq"] = qstart[d["queryseq"].astype(np.int64)] + \
            d["querystart"]
        d["querystart"] = 0
        assert np.array_equal(srt(engine_list(V, r["L"], "d").fetch()),
                              srt(d))
        both = engine_list(V, r["L"], "p").fetch()
        p = rec[flags == 1]
        assert len(both) >= len(p) > 0 and \
            len(np.intersect1d(both, p)) == len(np.unique(p))
    assert np.array_equal(flags, np.sort(flags))     # the D pass comes first
    return [(V.Result.from_host(rec[flags == f]), bool(f))
            for f in sorted(set(flags.tolist()))]


@pytest.mark.parametrize("key", MC.keys())
def test_recorded_runs_through_the_engine(V, key):
    r = MC.run_of(key)
    rec, flags = MC.input_of(key)
    mc = V.MatchCluster(V.sink_params(**MC.layout_kwargs(r)), r["mode"],
                        r["value"])
    if MC.queryform(r):
        for lst, pal in engine_passes(V, r, rec, flags):
            mc.add(lst, pal)
    else:
        lst = engine_list(V, r["L"], "d")
        assert np.array_equal(lst.fetch(), rec)
        mc.add(lst)
    mc.finish()
    st = mc.stats().asdict()
    assert (st["matches"], st["edges"], st["clusters"]) == \
        (r["matches"], r["edges"], r["clusters"])
    start, mem = mc.members()
    estart, m0, m1, values = mc.edges()
    got = dict(stats=st, text=mc.format(), clusterstart=start, members=mem,
               edgestart=estart, m0=m0, m1=m1, values=values)
    if not flags.any():
        # one pass: the library prints the files itself
        sink = MC.sink_of(V, r, palindromic=False)
        MC.check_against_manifest(
            key, got, lambda c: mc.format_cluster(
                sink, c, start[c + 1] - start[c], estart[c + 1] - estart[c]))
    res, pal = mc.records()
    who = mem.astype(np.int64)
    assert np.array_equal(res.fetch(), rec[who])
    assert np.array_equal(pal, flags[who])
    # the files from the device's records, each strand through its own sink
    lines = dict(zip(who.tolist(), MC.lines_of(V, r, res.fetch(), pal)))
    MC.check_against_manifest(key, got, MC.text_of(r, got, lines, flags))


# --------------------------------------------------------------------------
# hand-made lists against the model
# --------------------------------------------------------------------------

@pytest.mark.parametrize("G", [0, 7])
def test_a_gap_of_exactly_G_links_and_one_more_does_not(V, G):
    # match 0 ends at 110; match 1 starts G behind it, match 3 G + 1 behind
    # the end of match 2
    rec = MC.records(10, [100, 110 + G, 1000, 1010 + G + 1], isolated(4))
    mc, want = run(V, rec, MM.GAP, G)
    assert want["edges"] == [[(0, 1, G)]]
    assert mc.stats().candidates == 1


def test_a_successor_inside_the_match_ends_the_loop_at_once(V):
    # match 1 starts one symbol inside match 0: the gap wraps, match 0 links
    # nothing, although match 2 lies in reach; match 1 links match 2
    rec = MC.records(10, [100, 109, 121], isolated(3))
    mc, want = run(V, rec, MM.GAP, 15)
    assert want["edges"] == [[(1, 2, 2)]]
    # the same starts without the intruder: match 0 links match 2
    rec = MC.records(10, [100, 5000, 121], isolated(3))
    mc, want = run(V, rec, MM.GAP, 15)
    assert want["edges"] == [[(0, 2, 11)]]


@pytest.mark.parametrize("P, shared, linked", [
    (50, 50, True), (50, 49, False), (0, 0, True), (100, 100, True),
    (100, 99, False)])
def test_overlap_at_the_threshold(V, P, shared, linked):
    rec = MC.records(100, [1000, 1100 - shared], isolated(2))
    mc, want = run(V, rec, MM.OVERLAP, P)
    assert (want["stats"]["edges"] == 1) == linked
    if linked:
        assert want["edges"][0][0][2] == float(shared)


def test_overlap_is_measured_on_the_longer_match(V):
    # the longer one second: 30 shared symbols of 40 and 120 -> 25 percent
    rec = MC.records([40, 120, 120, 40], [1000, 1010, 3000, 3090],
                     isolated(4))
    mc, want = run(V, rec, MM.OVERLAP, 25)
    assert [e[2] for c in want["edges"] for e in c] == [25.0, 25.0]
    mc, want = run(V, rec, MM.OVERLAP, 26)
    assert want["stats"]["edges"] == 0 and want["stats"]["below"] == 2
    # thirds are not exact: the bits must agree all the same
    rec = MC.records([30, 7], [1000, 1029], isolated(2))
    run(V, rec, MM.OVERLAP, 3)


def test_the_second_reference_of_a_match_in_its_own_window(V):
    # match 1: position2 = position1 + length + 3; its neighbours 0 and 2
    # have references on both sides of that pair
    rec = MC.records(10, [95, 100, 112, 116],
                     [FAR, 113, FAR + 1000, FAR + 2000])
    mc, want = run(V, rec, MM.GAP, 8)
    assert want["stats"]["samematch"] == 1
    assert not any(a == b for c in want["edges"] for a, b, _ in c)
    run(V, rec, MM.OVERLAP, 0)


@pytest.mark.parametrize("mode, value", [(MM.GAP, 12), (MM.OVERLAP, 10)])
def test_a_list_against_queries_with_a_palindromic_pass(V, mode, value):
    # position2 is a query coordinate on the axis of position1, counted from
    # the other end of its query for the records of the palindromic pass: 7
    # queries of unequal length over the same stretch of numbers as the
    # database, 1500 D and 1100 P records (more than one block and tile)
    rng = np.random.default_rng(41)
    qlen = np.array([40, 93, 64, 17, 128, 55, 80], np.uint64)
    qstart = np.concatenate(([0], np.cumsum(qlen + np.uint64(1))[:-1])) \
        .astype(np.uint64)
    qtotal = int(qstart[-1] + qlen[-1])
    layout = V.sink_params(kind=V.SINK_QUERY, totallength=600,
                           markpos=np.zeros(0, np.uint64), querystart=qstart,
                           querylength=qlen, querytotallength=qtotal)
    n, nd = 2600, 1500
    rec = np.zeros(n, H.MATCH_DTYPE)
    rec["queryseq"] = rng.integers(0, len(qlen), n)
    room = qlen[rec["queryseq"].astype(np.int64)].astype(np.int64)
    rec["length"] = 1 + rng.integers(0, 16, n) % room
    rec["querystart"] = rng.integers(0, 1 << 20, n) % (
        room - rec["length"].astype(np.int64) + 1)
    rec["dbstart"] = rng.integers(0, 600 - 16, n)
    flags = (np.arange(n) >= nd).astype(np.uint8)
    l1, p1, p2 = MM.view(1, rec, flags, qstart, qlen)
    straight = MM.view(1, rec, None, qstart, qlen)[2]
    assert p2[:nd] == straight[:nd] and p2[nd:] != straight[nd:]
    want = MM.cluster(l1, p1, p2, mode, value)
    assert want["stats"]["edges"] > 2048
    mc = V.MatchCluster(layout, mode, value)
    mc.add(V.Result.from_host(rec[:nd]), False)
    mc.add(V.Result.from_host(rec[nd:]), True)
    mc.finish()
    compare(mc, want, rec, flags)
    host = V.matchcluster_host(layout, mode, value, rec, palindromic=flags)
    for k in ("clusterstart", "members", "labels", "edgestart", "m0", "m1",
              "values"):
        assert np.array_equal(host[k], want[k]), k
    # a record that leaves its query is refused, the state stays
    bad = rec[:3].copy()
    bad["querystart"][1] = 1000
    with pytest.raises(V.VsaError) as e:
        mc.add(V.Result.from_host(bad), True)
    assert e.value.code == -2
    compare(mc, want, rec, flags)


@pytest.mark.parametrize("parts", [1, 2])
def test_a_pile_on_one_start_keeps_the_order_of_the_indices(V, parts):
    # 300 references on start 7000 (both references of 50 matches among
    # them): equal starts stay in the order of their index
    n = 250
    p2 = isolated(n)
    p2[100:150] = 7000
    rec = MC.records(10 + np.arange(n) % 3, np.full(n, 7000), p2)
    mc, want = run(V, rec, MM.OVERLAP, 0, parts)
    assert want["stats"]["candidates"] == 300 * 299 // 2
    assert want["stats"]["samematch"] == 50


def test_a_pair_linked_through_both_of_its_reference_pairs(V):
    rec = MC.records(10, [100, 112], [5000, 5012])
    mc, want = run(V, rec, MM.GAP, 5)
    assert want["edges"] == [[(0, 1, 2), (0, 1, 2)]]
    assert want["stats"]["forestedges"] == 1


@pytest.mark.parametrize("N", [1023, 1024, 1025, 2048, 2049])
def test_tile_boundaries_of_candidates_and_edges(V, N):
    # a hub of one symbol reaches N leaves; every leaf starts inside its
    # predecessor and links nothing, and so does the far run of the second
    # references, which the hub's closes: N candidates, N edges
    rec = MC.records(np.r_[1, np.full(N, 5)], np.r_[0, 10 + np.arange(N)],
                     np.r_[FAR + N, FAR + np.arange(N)])
    mc, want = run(V, rec, MM.GAP, N + 8)
    assert want["stats"]["candidates"] == N == want["stats"]["edges"]
    assert want["stats"]["clusters"] == 1


def test_a_window_across_the_passes_of_the_candidate_slots(V, monkeypatch):
    monkeypatch.setenv("VSA_MATCHCLUSTER_CHUNK", "4096")
    n = 300
    rec = MC.records(20 + np.arange(n) % 7, 9000 + np.arange(n) % 2,
                     isolated(n))
    mc, want = run(V, rec, MM.OVERLAP, 96)
    assert want["stats"]["candidates"] > 44000 > 10 * 4096
    assert 0 < want["stats"]["below"] and want["stats"]["edges"] > 4096


def test_a_path_in_shuffled_order_takes_several_rounds(V):
    # node k: its first reference at place s[k], its second one 20 behind
    # the first reference of node k + 1: the edge numbers along the path are
    # a random permutation
    n = 3000
    rng = np.random.default_rng(9)
    s = rng.permutation(n + 1)
    rec = MC.records(10, 100 * s[:n], 100 * s[1:] + 20)
    order = rng.permutation(n)
    mc, want = run(V, rec[order], MM.GAP, 15)
    st = mc.stats()
    assert (st.edges, st.forestedges, st.clusters, st.inclusters) == \
        (n - 1, n - 1, 1, n)
    assert st.rounds > 1


@pytest.mark.parametrize("flip", [False, True])
def test_two_equal_clusters_merge_into_that_of_the_second_match(V, flip):
    # (0, 1) and (2, 3) first, then 1 and 3 through their second references
    late = (5000, 5012) if not flip else (5012, 5000)
    rec = MC.records(10, [0, 12, 1000, 1012],
                     [FAR, late[0], FAR + 1000, late[1]])
    mc, want = run(V, rec, MM.GAP, 5)
    assert want["clusters"] == ([[2, 3, 0, 1]] if not flip
                                else [[0, 1, 2, 3]])


def test_nothing_to_link(V):
    rec = MC.records(10, [100, 2000, 4000], isolated(3))
    for k in (0, 1, 3):
        for mode in (MM.GAP, MM.OVERLAP):
            mc, want = run(V, rec[:k], mode, 5)
            st = mc.stats()
            assert (st.matches, st.edges, st.clusters, st.rounds) == \
                (k, 0, 0, 0)
            assert mc.format() == b"# cluster %d matches\n" % k


def test_finish_add_more_finish_again(V):
    rng = np.random.default_rng(3)
    layout = MC.synthetic_layout(V)
    mc = V.MatchCluster(layout, MM.GAP, 30)
    rec = np.zeros(0, H.MATCH_DTYPE)
    with pytest.raises(V.VsaError):
        mc.members()                             # not finished yet
    for n in (40, 1, 700):
        places = rng.integers(0, 20000, 300)
        part = MC.records(rng.integers(1, 60, n), rng.choice(places, n),
                          rng.choice(places, n))
        mc.add(V.Result.from_host(part))
        with pytest.raises(V.VsaError) as e:
            mc.labels()
        assert e.value.code == -2
        mc.finish()
        rec = np.concatenate([rec, part])
        compare(mc, MC.model(rec, MM.GAP, 30), rec)
    assert all(v >= 0 for v in mc.times().values())


def test_refusals_leave_the_state_alone(V):
    rec = MC.records(10, [100, 112, 300], [5000, 5012, 7000])
    layout = MC.synthetic_layout(V)
    mc = V.MatchCluster(layout, MM.GAP, 5)
    mc.add(V.Result.from_host(rec))
    mc.finish()
    want = MC.model(rec, MM.GAP, 5)
    compare(mc, want, rec)
    # a record outside the text
    bad = rec.copy()
    bad["queryseq"][1] = 1 << 21
    with pytest.raises(V.VsaError) as e:
        mc.add(V.Result.from_host(bad))
    assert e.value.code == -2 and "1 records do not fit" in e.value.message
    compare(mc, want, rec)                       # still finished, unchanged
    # a packed-pair result
    gi = at1mb(V)
    tis, m = MC.CC.text()[0], MC.CC.model_layout()
    first = m.start[np.flatnonzero(m.seqlen >= 100)[:40]]
    sym = np.concatenate([tis[a:a + 100] for a in first])
    gq = V.Queries.from_host(sym, np.arange(40, dtype=np.uint64) * 100,
                             np.full(40, 100, np.uint64))
    packed = V.findmumcandidates_packed(gi, gq, 20)
    assert packed.packbits != 0
    with pytest.raises(V.VsaError) as e:
        mc.add(packed)
    assert e.value.code == V.NOT_COVERED
    # a palindromic list under a self layout
    with pytest.raises(V.VsaError) as e:
        mc.add(V.Result.from_host(rec), True)
    assert e.value.code == V.NOT_COVERED
    compare(mc, want, rec)
    # lists of vmatch -p IDX; erate
    sp = V.sink_params(kind=V.SINK_QUERY, totallength=1 << 20,
                       markpos=np.zeros(0, np.uint64), selfpalindromic=True)
    for lay, mode in ((sp, MM.GAP), (layout, V.MATCHCLUSTER_ERATE)):
        with pytest.raises(V.VsaError) as e:
            V.MatchCluster(lay, mode, 5)
        assert e.value.code == V.NOT_COVERED
    mc.finish()
    compare(mc, want, rec)
    run(V, rec, MM.GAP, 5)

"""Sequence clustering on the GPU (vsa_cluster_*): the recorded runs of the
real reference on the at1MB index, built and searched on the GPU -- the
direct list, the -d -p pair, a list that went through the selection --; and
the kernels against the pure-Python model (cluster_model.py) on hand-made
lists over 4100 sequences of 10 symbols: the smallest shapes with several
tiles of the compaction, several workgroups of the forest kernels, many
rounds and deep pointer jumping."""
import types

import numpy as np
import pytest

import helpers as H
import cluster_cases as CC
import cluster_model as CM

pytestmark = pytest.mark.gpu

NSEQ, SEQLEN = 4100, 10
# every round at least halves the components that still have an edge
MAXROUNDS = 13
_at = {}


def at1mb(V):
    """the index of at1MB built on the GPU"""
    if "index" not in _at:
        tis, ssp = CC.text()
        pl = H.manifest()["at1mb"]["index"]["prj"]["prefixlength"]
        _at["index"] = V.Index.build(tis, 4, pl, 0)
    return _at["index"]


def engine_list(V, L, strand):
    """a match list of the real entry points (kept: several runs share it)"""
    if (L, strand) not in _at:
        gi = at1mb(V)
        if strand == "d":
            _at[L, strand] = V.findmaximalrepeats(gi, L)
        else:
            tis, ssp = CC.text()
            rq = H.index_as_rc_queries(types.SimpleNamespace(
                tis=tis, ssp=ssp, n=len(tis)))
            gq = V.Queries.from_host(rq.symbols, rq.start, rq.length)
            _at[L, strand] = V.findquerymatches(gi, gq, L)
    return _at[L, strand]


def compare(cl, want, rec, flags, rounds=None):
    """a finished clustering against what the model (or a fixture through
    the model) says of the list rec / flags"""
    st = cl.stats().asdict()
    got_rounds = st.pop("rounds")
    wst = dict(want["stats"])
    wst.pop("rounds")
    assert st == wst
    if rounds is not None:
        assert got_rounds == rounds
    elif wst["edges"] == 0:
        assert got_rounds == 0
    else:
        assert 1 <= got_rounds <= MAXROUNDS
    start, mem = cl.members()
    assert np.array_equal(start, want["clusterstart"])
    assert np.array_equal(mem, want["members"])
    assert np.array_equal(cl.labels(), want["labels"])
    assert cl.format() == want["text"]
    res, eflags, estart = cl.edges()
    order = want["edgerecord"].astype(np.int64)
    assert np.array_equal(estart, want["edgestart"])
    assert np.array_equal(res.fetch(), rec[order])
    assert np.array_equal(eflags, np.asarray(flags, np.uint8)[order])
    assert res.count == wst["edges"]


# --------------------------------------------------------------------------
# the recorded runs through the engine
# --------------------------------------------------------------------------

@pytest.mark.parametrize("key", CC.keys())
def test_golden_runs_through_the_engine(V, key):
    r, e = CC.run_of(key), CC.manifest()[key]
    rec, flags = CC.input_of(key)
    want = CM.cluster(CC.model_layout(), rec, flags, r["percsmall"],
                      r["perclarge"])
    assert want["stats"] == e["stats"] and \
        CC.md5(want["text"]) == e["md5_text"]
    layout = V.sink_params(**CC.layout_kwargs(r))
    cl = V.Cluster(layout, r["percsmall"], r["perclarge"])
    for strand in r["strands"]:
        lst = engine_list(V, r["L"], strand)
        if r["select"]:
            sel = V.Select(layout, None, **r["select"])
            sel.add(lst, False)
            lst = sel.finish()
        if strand == "d":
            # the clusterer sees the list in the reference's order
            assert np.array_equal(lst.fetch(), rec[flags == 0])
        cl.add(lst, strand == "p")
    cl.finish()
    st = cl.stats()
    assert st.forestedges == e["stats"]["forestedges"]
    if r["forest"] is not None:
        assert st.forestedges == r["forest"]
    if "p" in r["strands"]:
        # seen, samesequence and mirrordropped count the engine's list, which
        # still holds both mirror images of every palindromic match
        assert st.mirrordropped > 0 and st.seen > e["stats"]["seen"]
        for k in ("rejected", "edges", "forestedges", "clusters",
                  "inclusters", "singlets"):
            assert getattr(st, k) == e["stats"][k], k
        want["stats"] = dict(st.asdict())
    compare(cl, want, rec, flags)
    assert CC.md5(cl.format()) == e["md5_text"]
    if r["edgefiles"]:
        res, eflags, estart = cl.edges()
        assert np.array_equal(CC.rows_of(res.fetch(), eflags),
                              CC.array(key + "__edgerows"))
        assert np.array_equal(estart, CC.array(key + "__edgestart"))


# --------------------------------------------------------------------------
# hand-made lists against the model
# --------------------------------------------------------------------------

def run_synthetic(V, pairs, length=5, percsmall=50, perclarge=50,
                  rounds=None):
    layout, lay = CC.synthetic_layout(V, NSEQ, SEQLEN)
    rec = CC.self_records(SEQLEN, pairs)
    rec["length"] = length
    flags = np.zeros(len(rec), np.uint8)
    cl = V.Cluster(layout, percsmall, perclarge)
    cl.add(V.Result.from_host(rec))
    cl.finish()
    compare(cl, CM.cluster(lay, rec, flags, percsmall, perclarge), rec,
            flags, rounds)
    return cl


def path_edges():
    return [(i, i + 1) for i in range(NSEQ - 1)]


def test_a_path_in_ascending_order_is_one_round_of_deep_jumping(V):
    # every sequence but the first picks the edge to its left: one chain of
    # 4099 hooks
    cl = run_synthetic(V, path_edges(), rounds=1)
    st = cl.stats()
    assert (st.clusters, st.inclusters, st.forestedges) == (1, NSEQ, NSEQ - 1)


def test_a_path_in_shuffled_order_takes_several_rounds(V):
    rng = np.random.default_rng(5)
    edges = [path_edges()[i] for i in rng.permutation(NSEQ - 1)]
    cl = run_synthetic(V, edges)
    assert cl.stats().rounds > 1 and cl.stats().forestedges == NSEQ - 1


def test_a_star(V):
    for edges in ([(0, i) for i in range(1, NSEQ)],
                  [(i, 7) for i in range(NSEQ - 1, 7, -1)]):
        cl = run_synthetic(V, edges, rounds=1)
        assert cl.stats().clusters == 1


def test_disjoint_pairs_listed_twice(V):
    pairs = [(2 * i, 2 * i + 1) for i in range(NSEQ // 2)]
    cl = run_synthetic(V, pairs + [p[::-1] for p in pairs], rounds=1)
    st = cl.stats()
    assert (st.clusters, st.edges, st.forestedges) == (2050, 4100, 2050)


@pytest.mark.parametrize("late", [(5, 2010), (2010, 5)])
def test_two_equal_clusters_joined_by_a_late_edge(V, late):
    a = [(i, i + 1) for i in range(0, 1024)]
    b = [(i, i + 1) for i in range(2000, 3024)]
    mixed = [e for pair in zip(a, b) for e in pair]
    cl = run_synthetic(V, mixed + [late])
    start, mem = cl.members()
    # the cluster of the second sequence takes the other one in
    assert mem[0] == (2000 if late[1] == 2010 else 0)
    assert cl.stats().clusters == 1 and cl.stats().inclusters == 2050


@pytest.mark.parametrize("accepted", [1023, 1024, 1025, 2048, 2049])
def test_accepted_edges_among_rejected_ones_at_the_tile_boundary(V, accepted):
    rng = np.random.default_rng(accepted)
    n = accepted + 3000
    pairs = np.stack([rng.integers(0, NSEQ - 1, n),
                      np.zeros(n, np.int64)], 1)
    pairs[:, 1] = pairs[:, 0] + 1 + rng.integers(0, 3, n)
    pairs[:, 1] = np.minimum(pairs[:, 1], NSEQ - 1)
    length = np.full(n, 4)                       # 10 * 50 / 100 = 5
    length[rng.permutation(n)[:accepted]] = 5
    cl = run_synthetic(V, pairs, length=length)
    st = cl.stats()
    assert (st.edges, st.rejected) == (accepted, 3000)


def test_lists_without_an_edge(V):
    layout, lay = CC.synthetic_layout(V, NSEQ, SEQLEN)
    same = CC.self_records(SEQLEN, [(i, i) for i in range(1500)], length=3)
    same["queryseq"] += np.uint64(4)
    low = CC.self_records(SEQLEN, [(1, 2), (3, 4)], length=2)
    for rec in (same[:0], same, low, np.concatenate([same, low])):
        cl = V.Cluster(layout, 50, 50)
        cl.add(V.Result.from_host(rec))
        cl.finish()
        flags = np.zeros(len(rec), np.uint8)
        compare(cl, CM.cluster(lay, rec, flags, 50, 50), rec, flags, 0)
        assert cl.stats().singlets == NSEQ and cl.format() == (
            "# 0 clusters\n# 0 elements out of 4100 (0.00%) are in clusters\n"
            "# 4100 elements out of 4100 (100.00%) are singlets\n").encode()
    # nothing added at all
    cl = V.Cluster(layout, 50, 50)
    cl.finish()
    assert cl.stats().asdict() == dict(
        seen=0, samesequence=0, mirrordropped=0, rejected=0, edges=0,
        forestedges=0, rounds=0, clusters=0, inclusters=0, singlets=NSEQ)
    assert cl.edges()[0].count == 0


def test_finish_add_more_finish_again(V):
    layout, lay = CC.synthetic_layout(V, NSEQ, SEQLEN)
    rng = np.random.default_rng(9)
    pairs = rng.integers(0, NSEQ // 2, (6000, 2)) * 2
    pairs[:, 1] += 1                             # never the same sequence
    rec = CC.self_records(SEQLEN, pairs)
    pal = np.zeros(700, H.MATCH_DTYPE)
    pal["length"] = 6
    pal["dbstart"] = rng.integers(0, NSEQ, 700) * (SEQLEN + 1) + 2
    pal["queryseq"] = rng.integers(0, NSEQ, 700)
    pal["querystart"] = rng.integers(0, 5, 700)
    cl = V.Cluster(layout, 50, 50)
    parts = [(rec[:2500], 0), (rec[2500:], 0), (pal, 1)]
    allrec = np.zeros(0, H.MATCH_DTYPE)
    allflags = np.zeros(0, np.uint8)
    with pytest.raises(V.VsaError):
        cl.members()                             # not finished yet
    for part, flag in parts:
        cl.add(V.Result.from_host(part), bool(flag))
        with pytest.raises(V.VsaError) as e:
            cl.labels()
        assert e.value.code == -2
        cl.finish()
        allrec = np.concatenate([allrec, part])
        allflags = np.concatenate([allflags, np.full(len(part), flag,
                                                     np.uint8)])
        compare(cl, CM.cluster(lay, allrec, allflags, 50, 50), allrec,
                allflags)
    assert cl.stats().mirrordropped > 100
    a, f, e = cl.times()
    assert a > 0 and f > 0 and e > 0


def test_percentages_accept_on_equal_and_reject_one_below(V):
    markpos = np.array([30], np.uint64)
    layout = V.sink_params(kind=V.SINK_SELF, totallength=81, markpos=markpos)
    rec = np.zeros(1, H.MATCH_DTYPE)
    rec["dbstart"], rec["queryseq"] = 2, 33
    for length, small, large, edges in ((20, 67, 41, 1), (19, 67, 41, 0),
                                        (20, 70, 0, 0), (20, 0, 42, 0),
                                        (21, 70, 42, 1), (20, 69, 41, 1)):
        rec["length"] = length
        cl = V.Cluster(layout, small, large)
        cl.add(V.Result.from_host(rec))
        cl.finish()
        st = cl.stats()
        assert (st.edges, st.rejected, st.clusters) == (edges, 1 - edges,
                                                        edges)


def test_refused_lists_leave_the_state_untouched(V):
    layout, lay = CC.synthetic_layout(V, NSEQ, SEQLEN)
    rec = CC.self_records(SEQLEN, [(i, i + 1) for i in range(0, 3000, 2)])
    flags = np.zeros(len(rec), np.uint8)
    cl = V.Cluster(layout, 50, 50)
    cl.add(V.Result.from_host(rec))
    cl.finish()
    want = CM.cluster(lay, rec, flags, 50, 50)
    for field, value in (("length", 11), ("queryseq", NSEQ * 11), ("length",
                                                                   0)):
        bad = rec.copy()
        bad[field][1200] = value
        with pytest.raises(V.VsaError) as e:
            cl.add(V.Result.from_host(bad))
        assert e.value.code == -2 and "1 records do not fit" in e.value.message
        compare(cl, want, rec, flags)            # still finished, unchanged
    # a packed-pair result
    gi = at1mb(V)
    tis, ssp = CC.text()
    m = CC.model_layout()
    first = m.start[np.flatnonzero(m.seqlen >= 100)[:40]]
    sym = np.concatenate([tis[a:a + 100] for a in first])
    gq = V.Queries.from_host(sym, np.arange(40, dtype=np.uint64) * 100,
                             np.full(40, 100, np.uint64))
    packed = V.findmumcandidates_packed(gi, gq, 20)
    assert packed.packbits != 0
    with pytest.raises(V.VsaError) as e:
        cl.add(packed)
    assert e.value.code == V.NOT_COVERED
    compare(cl, want, rec, flags)
    # a direct list under the layout of vmatch -p IDX; other kinds
    sp, _ = CC.synthetic_layout(V, NSEQ, SEQLEN, kind=V.SINK_QUERY,
                                selfpalindromic=True)
    c2 = V.Cluster(sp, 50, 50)
    with pytest.raises(V.VsaError) as e:
        c2.add(V.Result.from_host(rec))
    assert e.value.code == V.NOT_COVERED and c2.stats().seen == 0
    for kind in (V.SINK_COMPLETE, V.SINK_QUERY, V.SINK_APPROX_EDIST):
        other, _ = CC.synthetic_layout(V, NSEQ, SEQLEN, kind=kind)
        with pytest.raises(V.VsaError) as e:
            V.Cluster(other, 50, 50)
        assert e.value.code == V.NOT_COVERED
    one = V.sink_params(kind=V.SINK_SELF, totallength=50, markpos=[])
    with pytest.raises(V.VsaError) as e:
        V.Cluster(one, 50, 50)
    assert e.value.code == -2 and e.value.message == \
        "option -dbcluster only possible for index with at least two sequences"
    withq, _ = CC.synthetic_layout(V, 4, 10, numofquerysequences=2)
    with pytest.raises(V.VsaError) as e:
        V.Cluster(withq, 50, 50)
    assert e.value.message == \
        "option -dbcluster requires index without query sequences"

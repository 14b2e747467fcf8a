"""vmatch -pp matchcluster erate E on the GPU (vsa_eratecluster_open):
the recorded runs of the real reference on the at1MB index, built and searched
on the GPU, with the cluster files formatted from the device's own records and
edges; and the kernels against vsa_eratecluster_host on hand-made lists
over small texts -- every bound at which the width of a lane group changes,
the cap and one more, the edges of the length test, the order of the cascade,
special symbols, the ends of the text, several passes over the pairs and
several lists.  Every edge, value, member and printed byte is compared."""
import numpy as np
import pytest

import helpers as H
import erate_cases as EC
from test_gpu_cluster import at1mb, engine_list

pytestmark = pytest.mark.gpu

CAP = 127
_made = {}


def index_of(V, name, text):
    """the index of a hand-made text, built once"""
    if name not in _made:
        _made[name] = V.Index.build(
            text, 4, H.recommended_prefixlength(4, len(text)), 0)
    return _made[name]


def compare(V, mc, host, rec, sink):
    """a finished clustering against what the host code says of the list"""
    st = mc.stats().asdict()
    rounds = st.pop("rounds")
    wst = host["stats"].asdict()
    wst.pop("rounds")
    assert st == wst
    assert (rounds == 0) == (wst["edges"] == 0)
    assert st["samematch"] == 0 and \
        st["candidates"] == len(rec) * (len(rec) - 1) // 2 and \
        st["below"] == st["candidates"] - st["edges"]
    start, mem = mc.members()
    assert np.array_equal(start, host["clusterstart"])
    assert np.array_equal(mem, host["members"])
    assert np.array_equal(mc.labels(), host["labels"])
    assert mc.format() == host["text"]
    estart, m0, m1, values = mc.edges()
    assert np.array_equal(estart, host["edgestart"])
    assert np.array_equal(m0, host["m0"])
    assert np.array_equal(m1, host["m1"])
    assert np.array_equal(values, host["values"])
    res, flags = mc.records()
    who = host["members"].astype(np.int64)
    assert np.array_equal(res.fetch(), rec[who])
    assert not flags.any()
    for c in range(len(start) - 1):
        a, b, e0, e1 = int(start[c]), int(start[c + 1]), int(estart[c]), \
            int(estart[c + 1])
        assert mc.format_cluster(sink, c, b - a, e1 - e0) == \
            V.matchcluster_format_host(
                sink, V.MATCHCLUSTER_ERATE, mem[a:b],
                rec[mem[a:b].astype(np.int64)], m0[e0:e1], m1[e0:e1],
                values[e0:e1])


def run(V, name, text, rec, E, parts=1):
    """the list through the device (in `parts` add calls) and the host code
    -> (handle, the host's answer with its edges as (i, j, distance) in the
    order of the clusters)"""
    layout = EC.layout_of(V, text)
    mc = V.MatchCluster.erate(layout, index_of(V, name, text), E)
    for part in np.array_split(rec, parts):
        mc.add(V.Result.from_host(part))
    mc.finish()
    host = V.matchcluster_erate_host(layout, E, text, rec)
    sink = V.Sink(kind=2, totallength=len(text),
                  markpos=np.flatnonzero(text == H.SEPARATOR)
                  .astype(np.uint64))
    compare(V, mc, host, rec, sink)
    host["found"] = sorted(zip(host["m0"].tolist(), host["m1"].tolist(), (
        host["values"] & np.uint64(0xFFFFFFFF)).tolist()))
    return mc, host


# --------------------------------------------------------------------------
# the recorded runs through the engine
# --------------------------------------------------------------------------

@pytest.mark.parametrize("key", EC.keys())
def test_recorded_runs_through_the_engine(V, key):
    r = EC.run_of(key)
    rec = EC.input_of(key)
    lst = engine_list(V, r["L"], "d")
    assert np.array_equal(lst.fetch(), rec)
    mc = V.MatchCluster.erate(V.sink_params(**EC.layout_kwargs(r)), at1mb(V),
                              r["erate"])
    mc.add(lst)
    mc.finish()
    st = mc.stats().asdict()
    assert (st["matches"], st["edges"], st["clusters"]) == \
        (r["matches"], r["edges"], r["clusters"])
    start, mem = mc.members()
    estart, m0, m1, values = mc.edges()
    assert int((values & np.uint64(0xFFFFFFFF)).max()) == r["largest"]
    got = dict(stats=st, text=mc.format(), clusterstart=start, members=mem,
               edgestart=estart, m0=m0, m1=m1, values=values)
    sink = EC.sink_of(V, r)
    EC.check_against_manifest(
        key, got, lambda c: mc.format_cluster(
            sink, c, start[c + 1] - start[c], estart[c + 1] - estart[c]))
    res, pal = mc.records()
    assert np.array_equal(res.fetch(), rec[mem.astype(np.int64)])
    assert not pal.any()


# --------------------------------------------------------------------------
# hand-made lists against the host code
# --------------------------------------------------------------------------

BOUNDS = [1, 7, 8, 15, 16, 31, 32, 63, 64, CAP, CAP + 1]


def bounds_text():
    if "bounds" not in _made:
        t = EC.Text(11)
        lists = {m: EC.bound_case(t, m) for m in BOUNDS}
        _made["bounds"] = (t.symbols(), lists)
    return _made["bounds"]


@pytest.mark.parametrize("maxdist", BOUNDS[:-1])
def test_a_distance_of_exactly_the_bound_links_and_one_more_does_not(
        V, maxdist):
    text, lists = bounds_text()
    mc, host = run(V, "boundsindex", text, lists[maxdist], 10)
    assert host["found"] == [(0, 1, maxdist)]


@pytest.mark.parametrize("maxdist", [7, 16, 63, CAP])
def test_the_wide_rows_of_long_lists_give_the_same_answers(
        V, monkeypatch, maxdist):
    # lists with a match of 2^30 symbols or more keep their rows in 64 bits;
    # no test text is that long, so the environment asks for them
    monkeypatch.setenv("VSA_ERATE_WIDE_ROWS", "1")
    text, lists = bounds_text()
    mc, host = run(V, "boundsindex", text, lists[maxdist], 10)
    assert host["found"] == [(0, 1, maxdist)]
    text, rec = EC.planted_list(31, n=70)
    run(V, "planted31", text, rec, 30)


def test_a_bound_above_the_cap_is_refused_and_the_state_stays(V):
    text, lists = bounds_text()
    mc, host = run(V, "boundsindex", text, lists[CAP], 10)
    assert host["found"] == [(0, 1, CAP)]
    # three more matches, one pair of them with a bound of CAP + 1: the
    # finish is refused, as often as it is asked; the counts stay those of
    # the last finish, and the list added stays unfinished
    mc.add(V.Result.from_host(lists[CAP + 1]))
    before = mc.stats().asdict()
    assert before["matches"] == 3 and before["edges"] == 1
    for again in range(2):
        with pytest.raises(V.VsaError) as e:
            mc.finish()
        assert e.value.code == V.NOT_COVERED
        assert mc.stats().asdict() == before
        with pytest.raises(V.VsaError) as e:
            mc.members()
        assert e.value.code == -2
    # ... and the host code takes the list
    both = np.concatenate([lists[CAP], lists[CAP + 1]])
    far = V.matchcluster_erate_host(EC.layout_of(V, text), 10, text, both)
    assert sorted(zip(far["m0"].tolist(), far["m1"].tolist(), (
        far["values"] & np.uint64(0xFFFFFFFF)).tolist())) == \
        [(0, 1, CAP), (3, 4, CAP + 1)]


def edge_text():
    """one text for the hand-made pairs below -> (symbols, places)"""
    if "edge" not in _made:
        t = EC.Text(23)
        a = t.random(100)
        b = t.random(60)
        w = t.random(50)
        w[20] = H.WILDCARD
        p = {}
        p["first"] = t.put(b, gap=0)               # starts at position 0
        assert p["first"] == 0
        p["a"] = t.put(a)
        p["a_copy"] = t.put(a)
        p["a_plus5"] = t.put(np.concatenate([a, t.random(5)]))
        p["a_plus6"] = t.put(np.concatenate([a, t.random(6)]))
        p["a_sub1"] = t.put(EC.substituted(a, 1))
        p["a_sub3"] = t.put(EC.substituted(a, 3))
        for k in range(4):
            p["x%d" % k] = t.put(t.random(106))
        p["w"] = t.put(w)
        p["w_copy"] = t.put(w)
        p["sep"] = t.put(np.concatenate([t.random(20), [H.SEPARATOR],
                                         t.random(20)]))
        p["last"] = t.put(b, gap=0)                # ends on the last position
        _made["edge"] = (t.symbols(), p)
    return _made["edge"]


def test_lengths_that_differ_by_the_bound_and_by_one_more(V):
    text, p = edge_text()
    # E = 5, minlen 100: the bound is 5
    rec = EC.records([100, 105, 106], [p["a"], p["a_plus5"], p["a_plus6"]],
                     [p["x0"], p["x1"], p["x2"]])
    mc, host = run(V, "edgeindex", text, rec, 5)
    # 105 against 106: minlen 105, bound 5, one symbol apart -- but the
    # appended symbols differ
    assert (0, 1, 5) in host["found"] and \
        not any(e[:2] == (0, 2) for e in host["found"])


def test_only_the_last_instance_pair_is_within_the_bound(V):
    text, p = edge_text()
    rec = EC.records(100, [p["x0"], p["x1"]], [p["a"], p["a_sub1"]])
    mc, host = run(V, "edgeindex", text, rec, 5)
    assert host["found"] == [(0, 1, 1)]


def test_the_first_instance_pair_within_the_bound_is_stored(V):
    text, p = edge_text()
    # (1,1) is 3 apart, (1,2) only 1: the 3 is stored
    rec = EC.records(100, [p["a"], p["a_sub3"]], [p["x0"], p["a_sub1"]])
    mc, host = run(V, "edgeindex", text, rec, 5)
    assert host["found"] == [(0, 1, 3)]
    # ... and with the instances of match 1 the other way round, the 1
    rec = EC.records(100, [p["a"], p["a_sub1"]], [p["x0"], p["a_sub3"]])
    mc, host = run(V, "edgeindex", text, rec, 5)
    assert host["found"] == [(0, 1, 1)]


@pytest.mark.parametrize("E", [0, 4])
def test_wildcards(V, E):
    text, p = edge_text()
    # matches 0 and 1 share their first instance, a wildcard inside: 0
    # without a look at the text.  Match 2 is an exact copy elsewhere: the
    # wildcard does not equal its copy, the distance is 1 (bound 2 with E =
    # 4, 0 with E = 0)
    rec = EC.records(50, [p["w"], p["w"], p["w_copy"]],
                     [p["x0"], p["x1"], p["x2"]])
    mc, host = run(V, "edgeindex", text, rec, E)
    assert host["found"] == ([(0, 1, 0)] if E == 0 else
                             [(0, 1, 0), (0, 2, 1), (1, 2, 1)])


@pytest.mark.parametrize("E", [0, 10])
def test_instances_at_both_ends_of_the_text(V, E):
    text, p = edge_text()
    assert p["last"] + 60 == len(text)
    rec = EC.records(60, [p["first"], p["x0"]], [p["x1"], p["last"]])
    mc, host = run(V, "edgeindex", text, rec, E)
    assert host["found"] == [(0, 1, 0)]


def test_an_error_rate_of_100(V):
    text, p = edge_text()
    # unrelated instances, bounds of 40, 60 and 90: a pair is linked if its
    # lengths pass and the distance stays below the shorter length
    rec = EC.records([40, 60, 90, 106], [p["x0"], p["x1"], p["x2"], p["x3"]],
                     [p["x3"] + 40, p["a"], p["a_sub3"], p["a_plus6"]])
    mc, host = run(V, "edgeindex", text, rec, 100)
    assert (0, 2) not in [e[:2] for e in host["found"]]
    assert len(host["found"]) >= 3 and all(e[2] > 15 for e in host["found"])


def test_matches_that_overlap_in_the_text(V):
    text, p = edge_text()
    # the first instances are the same text, shifted by 1, 2 and 3 symbols:
    # the diagonal on which the reference's front does not slide
    rec = EC.records(90, [p["a"], p["a"] + 1, p["a"] + 2, p["a"] + 3,
                          p["a_copy"] + 1],
                     [p["x0"], p["x1"], p["x2"], p["x3"], p["a_sub1"] + 2])
    mc, host = run(V, "edgeindex", text, rec, 8)
    assert len(host["found"]) >= 4


def test_refusals_leave_the_state_alone(V):
    text, p = edge_text()
    layout = EC.layout_of(V, text)
    index = index_of(V, "edgeindex", text)
    rec = EC.records(100, [p["a"], p["a_sub1"]], [p["a_copy"], p["x0"]])
    mc, host = run(V, "edgeindex", text, rec, 5)
    sink = V.Sink(kind=2, totallength=len(text),
                  markpos=np.flatnonzero(text == H.SEPARATOR)
                  .astype(np.uint64))
    # a record across a separator; one that leaves the text
    for bad in (EC.records(30, [p["sep"] + 5], [p["x0"]]),
                EC.records(30, [p["x0"]], [len(text) - 10])):
        with pytest.raises(V.VsaError) as e:
            mc.add(V.Result.from_host(np.concatenate([rec[:1], bad])))
        assert e.value.code == -2 and "1 records do not fit" in \
            e.value.message
        compare(V, mc, host, rec, sink)
    # a palindromic list; a length of 2^32
    with pytest.raises(V.VsaError) as e:
        mc.add(V.Result.from_host(rec), True)
    assert e.value.code == V.NOT_COVERED
    long = rec.copy()
    long["length"][1] = 1 << 32
    with pytest.raises(V.VsaError) as e:
        mc.add(V.Result.from_host(long))
    assert e.value.code == V.NOT_COVERED
    mc.finish()
    compare(V, mc, host, rec, sink)
    # layouts the open refuses; the plain open still refuses the mode
    q = dict(querystart=np.array([0], np.uint64),
             querylength=np.array([40], np.uint64), querytotallength=40)
    for lay, code in (
            (V.sink_params(kind=V.SINK_QUERY, totallength=len(text),
                           markpos=np.zeros(0, np.uint64), **q),
             V.NOT_COVERED),
            (V.sink_params(kind=V.SINK_QUERY, totallength=len(text),
                           markpos=np.zeros(0, np.uint64),
                           selfpalindromic=True), V.NOT_COVERED),
            (V.sink_params(kind=2, totallength=len(text) + 1,
                           markpos=np.zeros(0, np.uint64)), -2)):
        with pytest.raises(V.VsaError) as e:
            V.MatchCluster.erate(lay, index, 5)
        assert e.value.code == code
    with pytest.raises(V.VsaError) as e:
        V.MatchCluster.erate(layout, index, 101)
    assert e.value.code == -2
    with pytest.raises(V.VsaError) as e:
        V.MatchCluster(layout, V.MATCHCLUSTER_ERATE, 5)
    assert e.value.code == V.NOT_COVERED


def test_nothing_to_link(V):
    text, p = edge_text()
    rec = EC.records(100, [p["a"], p["x0"]], [p["x1"], p["x2"]])
    for k in (0, 1, 2):
        mc, host = run(V, "edgeindex", text, rec[:k], 5)
        st = mc.stats()
        assert (st.matches, st.edges, st.clusters, st.rounds) == (k, 0, 0, 0)
        assert mc.format() == b"# cluster %d matches\n" % k
    # two matches that are linked
    mc, host = run(V, "edgeindex", text,
                   EC.records(100, [p["a"], p["a_copy"]], [p["x1"], p["x2"]]),
                   5)
    assert host["found"] == [(0, 1, 0)]


@pytest.mark.parametrize("E", [0, 10, 30])
def test_pairs_and_survivors_across_several_passes(V, monkeypatch, E):
    monkeypatch.setenv("VSA_MATCHCLUSTER_CHUNK", "300")
    text, rec = EC.planted_list(31, n=70)
    mc, host = run(V, "planted31", text, rec, E, parts=2)
    st = mc.stats()
    assert st.candidates == 70 * 69 // 2 > 8 * 300
    if E > 0:
        assert st.edges > 300 // 4


def test_finish_add_more_finish_again(V):
    text, rec = EC.planted_list(32, n=1500)
    layout = EC.layout_of(V, text)
    mc = V.MatchCluster.erate(layout, index_of(V, "planted32", text), 10)
    sink = V.Sink(kind=2, totallength=len(text),
                  markpos=np.zeros(0, np.uint64))
    with pytest.raises(V.VsaError):
        mc.members()                             # not finished yet
    seen = 0
    for n in (40, 1, 1459):
        mc.add(V.Result.from_host(rec[seen:seen + n]))
        seen += n
        with pytest.raises(V.VsaError) as e:
            mc.labels()
        assert e.value.code == -2
        mc.finish()
        compare(V, mc, V.matchcluster_erate_host(layout, 10, text,
                                                 rec[:seen]), rec[:seen],
                sink)
    # more than a tile of pairs, of survivors and of edges
    st = mc.stats()
    assert st.candidates > 1 << 20 and st.edges > 2048
    assert all(v >= 0 for v in mc.times().values())

"""vmatch -pp matchcluster erate E without a GPU: vsa_eratecluster_host
and the pure-Python model (erate_model.py) against the recorded runs of the
real reference (members, edges in file order, values, the md5 of the printed
text and of every cluster file), against each other on random lists over
small texts with planted near-copies, the front against the plain DP where
both must agree, and the refusals."""
import numpy as np
import pytest

import helpers as H
import cluster_model as CM
import erate_cases as EC
import erate_model as EM
import vstree_amd as V


def host_as_model(layout, text, rec, E):
    got = V.matchcluster_erate_host(layout, E, text, rec)
    got["stats"] = got["stats"].asdict()
    return got


def same(got, want):
    gs, ws = dict(got["stats"]), dict(want["stats"])
    gs.pop("rounds"), ws.pop("rounds")
    assert gs == ws
    for k in ("clusterstart", "members", "labels", "edgestart", "m0", "m1",
              "values"):
        assert np.array_equal(got[k], want[k]), k
    assert got["text"] == want["text"]


@pytest.mark.parametrize("key", EC.keys())
def test_recorded_runs(key):
    r = EC.run_of(key)
    rec = EC.input_of(key)
    layout = V.sink_params(**EC.layout_kwargs(r))
    host = host_as_model(layout, EC.text(), rec, r["erate"])
    st = host["stats"]
    assert (st["matches"], st["edges"], st["clusters"]) == \
        (r["matches"], r["edges"], r["clusters"])
    assert int((host["values"] & np.uint64(0xFFFFFFFF)).max()) == r["largest"]
    sink = EC.sink_of(V, r)
    lines = sink.format(rec).decode().splitlines()
    EC.check_against_manifest(key, host, EC.text_of(host, lines))

    # the library's own formatter prints the same files
    def host_text(c):
        a, b = (int(x) for x in host["clusterstart"][c:c + 2])
        e0, e1 = (int(x) for x in host["edgestart"][c:c + 2])
        mem = host["members"][a:b]
        return V.matchcluster_format_host(
            sink, V.MATCHCLUSTER_ERATE, mem, rec[mem.astype(np.int64)],
            host["m0"][e0:e1], host["m1"][e0:e1], host["values"][e0:e1])
    EC.check_against_manifest(key, host, host_text)


# (the generator runs the model on all five; the other three take minutes)
@pytest.mark.parametrize("key", ["l60_erate5", "l60_erate0"])
def test_the_model_on_the_recorded_runs(key):
    r = EC.run_of(key)
    rec = EC.input_of(key)
    sink = EC.sink_of(V, r)
    lines = sink.format(rec).decode().splitlines()
    for replay in (CM.full_replay, CM.forest_replay):
        want = EC.model_of(r, rec, replay=replay)
        EC.check_against_manifest(key, want, EC.text_of(want, lines))


@pytest.mark.parametrize("seed, E", [(1, 0), (2, 5), (3, 10), (4, 20),
                                     (5, 100)])
def test_random_lists_agree_with_the_model(seed, E):
    text, rec = EC.planted_list(seed)
    layout = EC.layout_of(V, text)
    got = host_as_model(layout, text, rec, E)
    view = EC.view(rec)
    same(got, EM.cluster(text, *view, E, answer=EM.front_answer))
    same(got, EM.cluster(text, *view, E))                  # batch_answers
    same(got, EM.cluster(text, *view, E, replay=CM.forest_replay))
    assert got["stats"]["edges"] > 0 or E == 0


def test_the_front_is_the_plain_distance_away_from_the_same_text():
    # instance pairs that start more than the bound apart never meet the
    # shortcut of the reference's front: there it is the textbook distance
    text, rec = EC.planted_list(7, n=24)
    l1, p1, p2 = EC.view(rec)
    checked = within = apart = 0
    for E in (10, 25):
        for i in range(len(l1)):
            for j in range(i + 1, len(l1)):
                md = EM.maxdist(min(l1[i], l1[j]), E)
                for pu in (p1[i], p2[i]):
                    for pv in (p1[j], p2[j]):
                        f = EM.front_answer(text, pu, l1[i], pv, l1[j], md)
                        if EM.may_differ(pu, pv, md):
                            apart += f != EM.dp_answer(text, pu, l1[i], pv,
                                                       l1[j], md)
                            continue
                        if abs(l1[i] - l1[j]) <= md:
                            assert f == EM.dp_answer(text, pu, l1[i], pv,
                                                     l1[j], md)
                            checked += 1
                            within += f >= 0
    assert checked > 200 and within > 20
    assert apart > 0        # ... and on the same text it is not


def test_the_bound_is_one_multiplication_and_one_division():
    for minlen, E, want in ((20, 10, 2), (29, 10, 2), (30, 10, 3),
                            (517, 20, 103), (7, 15, 1), (1270, 10, 127),
                            (100, 0, 0), (33, 100, 33), (57, 7, 3)):
        assert EM.maxdist(minlen, E) == want


def test_small_lists():
    text, rec = EC.planted_list(1)
    layout = EC.layout_of(V, text)
    for k in (0, 1):
        got = host_as_model(layout, text, rec[:k], 10)
        assert got["stats"]["edges"] == 0 and got["stats"]["clusters"] == 0
        assert got["text"] == b"# cluster %d matches\n" % k


def test_refusals():
    text, rec = EC.planted_list(1)
    layout = EC.layout_of(V, text)
    n = len(text)

    def refused(code, lay=layout, E=5, r=rec, t=text):
        with pytest.raises(V.VsaError) as e:
            V.matchcluster_erate_host(lay, E, t, r)
        assert e.value.code == code, e.value.message

    # the plain entry still has no text to look at
    with pytest.raises(V.VsaError) as e:
        V.matchcluster_host(layout, V.MATCHCLUSTER_ERATE, 5, rec)
    assert e.value.code == V.NOT_COVERED
    # layouts against queries, with indexed queries, selfpalindromic
    q = dict(querystart=np.array([0], np.uint64),
             querylength=np.array([40], np.uint64), querytotallength=40)
    refused(V.NOT_COVERED, V.sink_params(
        kind=V.SINK_QUERY, totallength=n, markpos=np.zeros(0, np.uint64), **q))
    refused(V.NOT_COVERED, V.sink_params(
        kind=V.SINK_QUERY, totallength=n, markpos=np.zeros(0, np.uint64),
        selfpalindromic=True))
    # an error rate above 100, a text of another length
    refused(-2, E=101)
    refused(-2, t=text[:-1])
    # a length of 2^32
    long = rec.copy()
    long["length"][3] = 1 << 32
    refused(V.NOT_COVERED, r=long)
    # a record that leaves the text; one that holds a separator
    out = rec.copy()
    out["queryseq"][2] = n - 5
    refused(-2, r=out)
    sep = text.copy()
    sep[int(rec["dbstart"][4]) + 3] = H.SEPARATOR
    refused(-2, lay=EC.layout_of(V, sep), t=sep)
